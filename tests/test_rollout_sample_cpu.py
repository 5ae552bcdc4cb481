"""CPU: the sampling closed-loop rollouts and the returns kernel without a GPU -- the symbols and the header's statement of
the sampling rule, every documented refusal in its order of precedence (answered before any device call), the launch the
describe call names (where the threshold table lives, LDS with the staged table counted), the host's conversion of
probabilities into thresholds, the rule itself restated in numpy on 2^20 Philox draws, and what the new kernels need per
wave."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from closed_loop_ref import (bare_grid_env, explore_draw, fields as _fields, grid_params as _params, perenv_lds as _perenv_lds,
                             shared_lds as _shared_lds, u8_lds as _u8_lds)
from closed_loop_ref import test_numpy_philox_known_answers  # noqa: F401  (collected here: the draws below are philox's)
from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_rollout_sample", "lmaze_rollout_sample_u8", "lmaze_describe_rollout_sample", "lmaze_returns")
TOP = 2 ** 32 - 1


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in NAMES:
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4
    assert C.sizeof(abi.LmazeParams) == 32
    pkg = importlib.import_module("gym-lmaze_amd")
    assert callable(pkg.discounted_returns) and "discounted_returns" in pkg.__all__
    assert hasattr(pkg.LmazeVecEnv, "rollout_sample")
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("uint32[S, 4]", "16-byte aligned", "c0 <= c1 <= c2", "word 3 is reserved", "one 128-bit read",
                   "(r >= c0) + (r >= c1) + (r >= c2)", "ep_hi ^ 0x80000000", "Always in 0..3", "not validated",
                   "a0 = p0, a1 = a0 + p1, a2 = a1 + p2, s = a2 + p3", "min(floor(a_k / s 2^32 + 0.5), 2^32 - 1)", "1 - 2^-32",
                   "advances its epoch by T", "table=lds", "table=global", "G <= 32", "never a fused multiply-add",
                   "returns_t may be reward_t"):
        assert phrase in flat, phrase


def _call(abi, u8=False, variant="v0", G=11, mode=None, T=6, n=100, table=64, key_mode=0, obs_t=None, every=0, params=True,
          layout=64, ball=64, goal=None, obs=None):
    """Fabricated device addresses: every refusal is returned before anything is dereferenced or queued."""
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else (abi.VARIANT_V0 if variant == "v0" else variant), G,
                        abi.LAYOUT_SHARED if mode is None else mode, 100, -1.0, -0.01, 100.0)
    fn = abi.lib.lmaze_rollout_sample_u8 if u8 else abi.lib.lmaze_rollout_sample
    return fn(C.byref(p) if params else None, layout, table, key_mode, T, ball, goal, 64, 64, 64, None, obs, None, None, None,
              None, n, 1, 1, 0, 0, obs_t, every, None)


@pytest.mark.parametrize("u8", [False, True])
def test_refusals_in_order_of_precedence(abi, u8):
    """lmaze_rollout_policy's refusals in its order, the thresholds in the table's place; a table off a 16-byte boundary
    joins the alignment refusals."""
    kw = dict(u8=u8)
    # 1. the recording request, before anything else -- even NULL params or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, n=-1, params=False, **kw) == E_NULL
    assert _call(abi, every=-1, table=None, key_mode=7, **kw) == E_COUNT
    # 2. params, variant (u8: layout mode, grid), T -- before the key mode
    assert _call(abi, params=False, key_mode=7, **kw) == E_NULL
    assert _call(abi, G=2, key_mode=7, **kw) == E_GRID
    assert _call(abi, mode=5, key_mode=7, **kw) == E_LAYOUT
    assert _call(abi, n=-1, key_mode=7, **kw) == E_COUNT
    assert _call(abi, variant=2, key_mode=0, **kw) == E_VARIANT
    if u8:
        assert _call(abi, mode=abi.LAYOUT_PER_ENV, key_mode=7, **kw) == E_LAYOUT
        assert _call(abi, G=3, key_mode=7, **kw) == E_GRID
    assert _call(abi, T=-1, key_mode=1, **kw) == E_COUNT
    # 3. the key mode: outside {0, 1}, then goal-conditioned on v0 -- both before "nothing to do" and before the pointers
    for km in (-1, 2, 7):
        assert _call(abi, key_mode=km, table=None, **kw) == E_COUNT
        assert _call(abi, key_mode=km, T=0, **kw) == E_COUNT
        assert _call(abi, variant="v3", key_mode=km, goal=64, **kw) == E_COUNT
    assert _call(abi, key_mode=1, table=None, **kw) == E_VARIANT
    assert _call(abi, key_mode=1, n=0, **kw) == E_VARIANT
    # 4. pointers: the table among them; then alignment, the table's 16 bytes among them
    assert _call(abi, table=None, **kw) == E_NULL
    assert _call(abi, variant="v3", key_mode=1, table=None, goal=64, **kw) == E_NULL
    assert _call(abi, variant="v3", key_mode=1, goal=None, **kw) == E_NULL
    assert _call(abi, layout=None, **kw) == E_NULL
    assert _call(abi, table=None, ball=68, **kw) == E_NULL           # NULL before alignment
    assert _call(abi, layout=None, table=64 + 8, **kw) == E_NULL
    assert _call(abi, ball=68, **kw) == E_ALIGN
    assert _call(abi, obs=4096 + 8, **kw) == E_ALIGN
    for off in (4, 8, 12):
        assert _call(abi, table=64 + off, **kw) == E_ALIGN
        assert _call(abi, variant="v3", key_mode=1, goal=64, table=4096 + off, **kw) == E_ALIGN
    if not u8:
        assert _call(abi, layout=72, **kw) == E_ALIGN


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("variant,key_mode", [("v0", 0), ("v3", 0), ("v3", 1)])
@pytest.mark.parametrize("T,n", [(0, 100), (6, 0), (0, 0)])
def test_nothing_to_do_reads_no_pointer(abi, u8, variant, key_mode, T, n):
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, 11, abi.LAYOUT_SHARED, 100, -1.0, -0.01, 100.0)
    fn = abi.lib.lmaze_rollout_sample_u8 if u8 else abi.lib.lmaze_rollout_sample
    none = (None,) * 11
    assert fn(C.byref(p), None, None, key_mode, T, *none, n, 1, 1, 0, 0, None, 0, None) == 0
    assert fn(C.byref(p), None, 68, key_mode, T, *none, n, 1, 1, 0, 0, None, 0, None) == 0           # not even its alignment
    assert fn(C.byref(p), None, None, key_mode, T, *none, n, 1, 1, 0, 0, None, 3 if T < 3 else 7, None) == 0   # T / k == 0 slots
    assert fn(C.byref(p), None, None, key_mode, -1, *none, n, 1, 1, 0, 0, None, 0, None) == E_COUNT


def test_returns_refusals_and_nothing_to_do(abi):
    """NULL, then the counts; T == 0 or n == 0 returns 0 on fabricated pointers: nothing is read or queued."""
    f = abi.lib.lmaze_returns
    assert f(None, 64, None, 0.99, 64, 5, 10, None) == E_NULL
    assert f(64, None, None, 0.99, 64, 5, 10, None) == E_NULL
    assert f(64, 64, None, 0.99, None, 5, 10, None) == E_NULL
    assert f(None, 64, 64, 0.99, 64, -1, -1, None) == E_NULL         # NULL before the counts
    assert f(64, 64, None, 0.99, 64, -1, 10, None) == E_COUNT
    assert f(64, 64, None, 0.99, 64, 5, -1, None) == E_COUNT
    assert f(64, 64, 64, 0.99, 64, 5, (1 << 30) + 1, None) == E_COUNT
    assert f(64, 64, None, 0.99, 64, -1, 0, None) == E_COUNT         # a bad count is refused with nothing to do, too
    for T, n in ((0, 10), (5, 0), (0, 0), (0, 1 << 30)):
        assert f(64, 64, None, 0.99, 64, T, n, None) == 0
        assert f(68, 65, 66, 0.99, 72, T, n, None) == 0


def _up16(x):                                               # the thresholds start on a 16-byte boundary
    return (x + 15) & ~15


def _staged(G, key):
    """The rule: ball-keyed and G <= 32 (at most 16 KiB) in LDS, everything else read from global memory."""
    return 16 * G * G if key == "ball" and G <= 32 else 0


def _where(G, key):
    return "lds" if _staged(G, key) else "global"


@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "ball"), ("v3", "goal")])
def test_describe_shared(abi, variant, key):
    """Shared layouts: rollout_shared_kernel's sampling form at the closed-loop forms' envs per workgroup (on-die 8x8, T == 1
    and launch_hint bit 8 included); table=lds at G = 11 and 32, table=global at G = 33 and 64 and for the goal key."""
    S = abi.LAYOUT_SHARED
    for G, n, T, hint, epb in [(11, 65536, 64, 0, 64), (11, 1 << 20, 64, 0, 64), (12, 16384, 64, 0, 32), (11, 777, 9, 0, 16),
                               (8, 65536, 16, 0, 64), (11, 65536, 1, 0, 64), (11, 65536, 16, 0x100, 64), (32, 4099, 5, 0, 16),
                               (33, 4099, 5, 0, 16), (64, 16384, 64, 0, 32), (64, 777, 7, 0, 16)]:
        line = abi.describe_rollout_sample(_params(abi, variant, G, S, hint), n, T, obs_every=3 if T >= 3 else 0, key=key)
        head = "rollout_shared_kernel<v%s, sample=%s, table=%s%s> T=%d every=%d " % (
            variant[1], key, _where(G, key), ", obs_t" if T >= 3 else "", T, 3 if T >= 3 else 0)
        assert line.startswith(head), line
        f = _fields(line)
        assert f["envs_per_workgroup"] == epb and f["grid"] == -(-n // epb) and f["block"] == 256, line
        assert f["lds"] == _up16(_shared_lds(G, epb)) + _staged(G, key), line
    assert _where(11, "ball") == _where(32, "ball") == "lds" and _where(33, "ball") == _where(64, "ball") == "global"
    # launch_hint bits 12-14: every value; bit 15: the slots' other store policy
    for k in range(1, 8):
        f = _fields(abi.describe_rollout_sample(_params(abi, variant, 11, S, k << 12), 4099, 8, key=key))
        assert f["envs_per_workgroup"] == 4 << (k - 1) and f["lds"] == _up16(_shared_lds(11, 4 << (k - 1))) + _staged(11, key)
    line = abi.describe_rollout_sample(_params(abi, variant, 11, S, 1 << 15), 4099, 8, obs_every=2, key=key)
    assert ", obs_t, nt> " in line


@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "ball"), ("v3", "goal")])
def test_describe_u8(abi, variant, key):
    S = abi.LAYOUT_SHARED
    for G, n, hint, epb in [(11, 65536, 0, 64), (11, 777, 0, 16), (12, 16384, 0, 16), (11, 4099, 1 << 12, 16),
                            (11, 4099, 6 << 12, 128), (11, 4099, 7 << 12, 256), (32, 4099, 7 << 12, 256), (33, 4099, 7 << 12, 256),
                            (64, 4099, 7 << 12, 256)]:
        line = abi.describe_rollout_sample(_params(abi, variant, G, S, hint), n, 16, with_obs="u8", obs_every=0, key=key)
        assert line.startswith("rollout_shared_u8_kernel<v%s, sample=%s, table=%s> T=16 every=0 " % (variant[1], key, _where(G, key))), line
        f = _fields(line)
        assert f["envs_per_workgroup"] == epb and f["grid"] == -(-n // epb), line
        assert f["lds"] == _u8_lds(G, epb) + _staged(G, key) <= 64 << 10, line
    f = _fields(abi.describe_rollout_sample(_params(abi, variant, 11, S), 1 << 20, 16, with_obs="u8", obs_every=1, key=key))
    assert f["envs_per_workgroup"] == 256


@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "ball"), ("v3", "goal")])
def test_describe_per_env_and_the_lds_clamp(abi, variant, key):
    PE = abi.LAYOUT_PER_ENV
    for G, n, hint, epb in [(11, 16384, 0, 16), (11, 777, 0, 16), (11, 65536, 0, 64), (32, 4099, 0, 16), (32, 4099, 5 << 12, 64),
                            (18, 4099, 7 << 12, 64), (33, 4099, 0, 16),
                            (64, 4099, 0, 8),             # 32 KiB of layouts per workgroup
                            (64, 4099, 5 << 12, 32),      # hinted 64: 256 KiB of layouts, halved to what fits 160 KiB
                            (64, 4099, 7 << 12, 32), (51, 4099, 5 << 12, 32), (50, 4099, 5 << 12, 64)]:
        line = abi.describe_rollout_sample(_params(abi, variant, G, PE, hint), n, 16, obs_every=4, key=key)
        assert line.startswith("rollout_perenv_kernel<v%s, sample=%s, table=%s, obs_t> T=16 every=4 " % (variant[1], key, _where(G, key))), line
        f = _fields(line)
        assert f["envs_per_workgroup"] == epb and f["grid"] == -(-n // epb), line
        assert f["lds"] == _up16(_perenv_lds(G, epb)) + _staged(G, key) <= 160 << 10, line
    for k in range(1, 8):                                   # every value of bits 12-14; at most 64 (every lane in wave 0)
        f = _fields(abi.describe_rollout_sample(_params(abi, variant, 11, PE, k << 12), 4099, 8, key=key))
        assert f["envs_per_workgroup"] == min(4 << (k - 1), 64)


@pytest.mark.parametrize("G", [8, 11, 12, 18, 32])
def test_the_staged_table_is_sixteen_g_squared_more_lds(abi, G):
    """The same shape with the table staged (v3, ball key) and read from global memory (v3, goal key): equal envs per
    workgroup, and exactly the table's 16 G^2 bytes apart -- a table read from global memory reserves nothing."""
    for mode, with_obs, hints in ((abi.LAYOUT_SHARED, True, (0, 2 << 12, 5 << 12)), (abi.LAYOUT_SHARED, "u8", (0, 3 << 12, 7 << 12)),
                                  (abi.LAYOUT_PER_ENV, True, (0, 1 << 12, 5 << 12))):
        for hint in hints:
            p = _params(abi, "v3", G, mode, hint)
            lds, glb = (abi.describe_rollout_sample(p, 4099, 12, with_obs=with_obs, obs_every=0, key=k) for k in ("ball", "goal"))
            assert "table=lds" in lds and "table=global" in glb
            a, b = _fields(lds), _fields(glb)
            assert a["envs_per_workgroup"] == b["envs_per_workgroup"] and a["grid"] == b["grid"]
            assert a["lds"] - b["lds"] == 16 * G * G, (lds, glb)


def test_describe_refusals_and_empty_lines(abi):
    p = _params(abi, "v0", 11, abi.LAYOUT_SHARED)
    buf = C.create_string_buffer(256)
    d = abi.lib.lmaze_describe_rollout_sample
    assert d(C.byref(p), 100, 6, 1, 1, -1, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), 100, 6, 1, 1, 0, 0, None, 256) == E_NULL
    assert d(None, 100, 6, 1, 1, 0, 0, buf, 256) == E_NULL
    assert d(C.byref(p), 100, 6, 1, 1, 0, 2, buf, 256) == E_COUNT
    assert d(C.byref(p), 100, 6, 1, 1, 0, 1, buf, 256) == E_VARIANT
    assert d(C.byref(p), 100, -1, 1, 1, 0, 0, buf, 256) == E_COUNT
    assert d(C.byref(_params(abi, "v0", 11, abi.LAYOUT_PER_ENV)), 100, 6, 1, 2, 0, 0, buf, 256) == E_LAYOUT
    assert d(C.byref(_params(abi, "v0", 3, abi.LAYOUT_SHARED)), 100, 6, 1, 2, 0, 0, buf, 256) == E_GRID
    assert abi.describe_rollout_sample(p, 0, 6) == "" and abi.describe_rollout_sample(p, 100, 0) == ""


# ------------------------------------------------------------- the Python surface without a device
def test_python_argument_errors_that_need_no_device(abi, monkeypatch):
    """What LmazeVecEnv.rollout_sample() refuses before it touches the device, in its order of precedence, on an env object
    that never saw one (G = 5, N = 8; its tensors are the host's).  Every call carries what the LATER refusals would object
    to as well, so the one that answers is the earlier one."""
    G, N = 5, 8
    S = G * G
    env = bare_grid_env(monkeypatch)
    probs = torch.ones(S, 4)
    thr = abi.sampling_thresholds(probs)
    junk = dict(probs=object(), logits=object(), temperature=0.0)           # two sources, neither a tensor, a bad temperature
    # 1. stream capture and the online tuner, before T
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="device-resident epoch or while the online tuner runs"):
            env.rollout_sample(-1, key="nope", **junk)
    env._tuner = object()
    with pytest.raises(ValueError, match="device-resident epoch or while the online tuner runs"):
        env.rollout_sample(-1, key="nope", **junk)
    env._tuner = None
    # 2. T, before the key
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_sample(T, key="nope", **junk)
    # 3. the key, before the sources are counted
    for key in ("nope", None, 0):
        with pytest.raises(ValueError, match="key must be 'ball', 'goal' or 'env'"):
            env.rollout_sample(4, key=key, **junk)
    with pytest.raises(ValueError, match="key='goal' needs the v3 variant"):
        env.rollout_sample(4, key="goal", **junk)
    env._u8 = True
    with pytest.raises(ValueError, match="key='env' needs the int32 planes"):
        env.rollout_sample(4, key="env", **junk)
    env._u8 = False
    env.num_envs = (2 ** 31 - 1) // S + 1
    with pytest.raises(ValueError, match=r"N \* G\*G <= 2\*\*31 - 1"):
        env.rollout_sample(4, key="env", **junk)
    env.num_envs = (2 ** 31 - 1) // S                                        # the largest N the key still fits
    with pytest.raises(ValueError, match="exactly one of"):
        env.rollout_sample(4, key="env", **junk)
    env.num_envs = N
    # 4. exactly one source, before any is looked at
    for kw in (dict(), dict(probs=object(), logits=object()), dict(probs=object(), thresholds=object()),
               dict(logits=object(), thresholds=object()), dict(probs=object(), logits=object(), thresholds=object())):
        for key in ("ball", "env"):
            with pytest.raises(ValueError, match="exactly one of probs=, logits= and thresholds="):
                env.rollout_sample(4, key=key, temperature=0.0, **kw)
    # 5. the source's shape, dtype and device, before the temperature
    meta = torch.ones(S, 4, device="meta")
    for name in ("probs", "logits"):
        for bad in (object(), [[0.25] * 4] * S, torch.ones(S, 5), torch.ones(S - 1, 4), torch.ones(S * 4), torch.ones(1, S, 4),
                    torch.ones(N * S, 4), torch.ones(S, 4, dtype=torch.int32), torch.ones(S, 4, dtype=torch.int64), meta):
            with pytest.raises(ValueError, match=r"%s must be a float tensor \[25, 4\] on cpu \(key='ball', G=5\)" % name):
                env.rollout_sample(4, temperature=0.0, **{name: bad})
        for bad in (torch.ones(S, 4), torch.ones(N, S, 5), torch.ones(N * S, 4, dtype=torch.int32),
                    torch.ones(N, 4, S).transpose(1, 2)):                    # [N, G*G, 4], but not the flat table's memory
            with pytest.raises(ValueError, match=r"%s must be a float tensor \[200, 4\] on cpu \(key='env', G=5\)" % name):
                env.rollout_sample(4, key="env", temperature=0.0, **{name: bad})
    env._is_v3 = True
    with pytest.raises(ValueError, match=r"probs must be a float tensor \[625, 4\] on cpu \(key='goal', G=5\)"):
        env.rollout_sample(4, key="goal", probs=probs)
    env._is_v3 = False
    # 6. the temperature: logits only, and after the logits' own check
    for bad in (0, 0.0, -1, float("nan")):
        with pytest.raises(ValueError, match="temperature must be > 0"):
            env.rollout_sample(4, logits=probs, temperature=bad, obs_every=-1)
        with pytest.raises(ValueError, match="obs_every must be >= 0"):      # not read with probs= or thresholds=
            env.rollout_sample(4, probs=probs, temperature=bad, obs_every=-1)
        with pytest.raises(ValueError, match="obs_every must be >= 0"):
            env.rollout_sample(4, thresholds=thr, temperature=bad, obs_every=-1)
    # 7. the converter's own refusals, before the recording request
    with pytest.raises(ValueError, match="finite and non-negative"):
        env.rollout_sample(4, probs=-probs, obs_every=-1)
    with pytest.raises(ValueError, match="positive, finite sum"):
        env.rollout_sample(4, probs=0 * probs, obs_every=-1)
    # 8. thresholds: dtype, shape, device, contiguity, 16-byte alignment -- one refusal, before the recording request
    flat = torch.zeros(S * 4 + 1, dtype=torch.int32)
    assert flat.data_ptr() % 16 == 0
    for bad in (object(), thr.view(torch.int32).to(torch.int64), thr.view(torch.int32).float(), thr.view(torch.int32).to(torch.uint8),
                thr.view(torch.int32)[:, :3].contiguous(), thr.view(torch.int32)[:-1], thr.view(torch.int32).reshape(-1),
                torch.zeros(S, 4, dtype=torch.int32, device="meta"), torch.zeros(S, 8, dtype=torch.int32)[:, ::2],
                flat[1:].view(S, 4)):
        with pytest.raises(ValueError, match=r"thresholds must be a contiguous, 16-byte aligned uint32 tensor \[25, 4\] on cpu "
                                             r"\(key='ball', G=5\)"):
            env.rollout_sample(4, thresholds=bad, obs_every=-1)
    # ... and what it takes: uint32 or int32, the caller's memory; for key="env" flat rows or the [N, G*G, 4] view of them
    envthr = abi.sampling_thresholds(torch.ones(N * S, 4))
    for key, good in (("ball", thr), ("ball", thr.view(torch.int32)), ("env", envthr), ("env", envthr.view(N, S, 4)),
                      ("env", envthr.view(torch.int32).view(N, S, 4))):
        with pytest.raises(ValueError, match="obs_every must be >= 0"):
            env.rollout_sample(4, key=key, thresholds=good, obs_every=-1)
    for name in ("probs", "logits"):
        for good in (torch.ones(N * S, 4), torch.ones(N, S, 4), torch.ones(N, S, 4, dtype=torch.float64)):
            with pytest.raises(ValueError, match="obs_every must be >= 0"):
                env.rollout_sample(4, key="env", obs_every=-1, **{name: good})
    for bad in (torch.zeros(N, S, 8, dtype=torch.int32)[:, :, ::2], torch.zeros(N, 4, S, dtype=torch.int32).transpose(1, 2),
                envthr.view(torch.int32).view(N, S, 4)[:-1], thr):
        with pytest.raises(ValueError, match=r"thresholds must be a contiguous, 16-byte aligned uint32 tensor \[200, 4\] on cpu "
                                             r"\(key='env', G=5\)"):
            env.rollout_sample(4, key="env", thresholds=bad, obs_every=-1)
    # 9. the recording request, last
    with pytest.raises(ValueError, match="obs_every=0 records the final planes only"):
        env.rollout_sample(4, thresholds=thr, obs_t=torch.zeros(1))
    with pytest.raises(ValueError, match="obs_every must be an int"):
        env.rollout_sample(4, thresholds=thr, obs_every=None)


# ------------------------------------------------------------- the host conversion
def _thr(abi, rows, dtype=torch.float64):
    t = abi.sampling_thresholds(torch.tensor(rows, dtype=dtype))
    assert t.dtype == torch.uint32 and tuple(t.shape) == (len(rows), 4) and t.is_contiguous()
    return t.numpy().astype(np.int64).tolist()


def test_sampling_thresholds_exact_values(abi):
    """c_k = min(floor(a_k / s * 2^32 + 0.5), 2^32 - 1) in float64, a_k the running sums, s the row's sum; word 3 is 0."""
    h = 2.0 ** -33
    got = _thr(abi, [[0.25, 0.25, 0.25, 0.25], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0.5, 0, 0.5],
                     [2, 2, 2, 2], [0, 0, 3, 0],                      # unnormalised rows: divided by their sum
                     [h, 1 - h, 0, 0],                                # 2^-33 * 2^32 + 0.5 = 1.0: rounds up to one count
                     [h / 2, 1 - h / 2, 0, 0],                        # 0.25 + 0.5: none
                     [3 * h, 1 - 3 * h, 0, 0],                        # 1.5 + 0.5: two
                     [1 - h, h, 0, 0],                                # 2^32 - 0.5 + 0.5 = 2^32: clamped
                     [1 - 2 * h, 0, 2 * h, 0],                        # 2^32 - 1 exactly, the largest word
                     [1 - 3 * h, 0, 0, 3 * h],                        # 2^32 - 1.5 + 0.5 = 2^32 - 1
                     [1 - 4 * h, 0, 4 * h, 0]])                       # 2^32 - 2
    assert got == [[1 << 30, 1 << 31, 3 << 30, 0], [TOP, TOP, TOP, 0], [0, 0, 0, 0], [0, 1 << 31, 1 << 31, 0],
                   [1 << 30, 1 << 31, 3 << 30, 0], [0, 0, TOP, 0],
                   [1, TOP, TOP, 0], [0, TOP, TOP, 0], [2, TOP, TOP, 0], [TOP, TOP, TOP, 0], [TOP, TOP, TOP, 0],
                   [TOP, TOP, TOP, 0], [TOP - 1, TOP - 1, TOP, 0]]
    # float32 and float16 input is widened first: 0.1f is not 0.1
    f = np.float32
    a0, a1, a2 = float(f(0.7)), float(f(0.7)) + float(f(0.1)), float(f(0.7)) + float(f(0.1)) + float(f(0.15))
    s = a2 + float(f(0.05))
    want = [int(np.floor(a / s * 4294967296.0 + 0.5)) for a in (a0, a1, a2)] + [0]
    assert _thr(abi, [[0.7, 0.1, 0.15, 0.05]], torch.float32) == [want]
    assert _thr(abi, [[0.5, 0.25, 0.25, 0]], torch.float16) == [[1 << 31, 3 << 30, TOP, 0]]
    # monotone whatever the row
    rs = np.random.RandomState(0)
    t = np.array(_thr(abi, (rs.rand(4096, 4) * (rs.rand(4096, 4) < 0.7) + 1e-300).tolist()))
    assert (t[:, 0] <= t[:, 1]).all() and (t[:, 1] <= t[:, 2]).all() and (t[:, 3] == 0).all()


def test_sampling_thresholds_refusals(abi):
    for bad in ([[0.5, -0.1, 0.3, 0.3]], [[0.5, float("nan"), 0.3, 0.2]], [[float("inf"), 0, 0, 0]], [[0, 0, 0, 0]],
                [[0.25] * 4, [0.0] * 4], [[-0.0, 0.0, -0.0, 0.0]], [[1e308, 1e308, 1e308, 1e308]]):
        with pytest.raises(ValueError):
            abi.sampling_thresholds(torch.tensor(bad, dtype=torch.float64))
    for bad in (torch.ones(4), torch.ones((3, 5)), torch.ones((3, 4), dtype=torch.int32), torch.ones((2, 3, 4)), [[0.25] * 4], None):
        with pytest.raises(ValueError):
            abi.sampling_thresholds(bad)


# ------------------------------------------------------------- the rule, restated
def test_the_sampling_rule_reproduces_its_probabilities(abi):
    """action = (r >= c0) + (r >= c1) + (r >= c2) with r the .x word of the closed loop's draw (the reset draw's counter
    with the top bit of its last word flipped), on 2^20 draws -- consecutive envs of one epoch, both words of the env index
    and of the epoch in use.  Each action's count is binomial(n, p): within 5 sigma; a probability of 0 never fires."""
    n, seed, base, ep = 1 << 20, 21, (1 << 33) + 1000, (1 << 35) + 77
    e = np.arange(n, dtype=np.uint64) + np.uint64(base)
    r = explore_draw(seed, ep, e)[0]
    rows = [[0.7, 0.1, 0.15, 0.05], [0.25, 0.25, 0.25, 0.25], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0.5, 0, 0.5], [0.3, 0, 0.7, 0]]
    thr = abi.sampling_thresholds(torch.tensor(rows, dtype=torch.float64)).numpy().astype(np.uint64)
    for p, c in zip(rows, thr):
        act = (r >= c[0]).astype(np.int64) + (r >= c[1]) + (r >= c[2])
        assert act.min() >= 0 and act.max() <= 3
        counts = np.bincount(act, minlength=4)
        for k in range(4):
            if p[k] == 0:
                assert counts[k] == 0, (p, counts)
            else:
                assert abs(counts[k] - n * p[k]) <= 5 * np.sqrt(n * p[k] * (1 - p[k])), (p, counts)
    # unvalidated rows still answer in 0..3: non-monotone, all zero, all ones
    for c, want in (((3 << 30, 1 << 30, 1 << 31), None), ((0, 0, 0), 3), ((TOP, TOP, TOP), 0)):
        c = np.array(c, np.uint64)
        act = (r >= c[0]).astype(np.int64) + (r >= c[1]) + (r >= c[2])
        assert act.min() >= 0 and act.max() <= 3
        if want is not None:
            assert (act == want).all()


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sampling_kernels_no_scratch_and_occupancy():
    """Six new rollout instantiations (three kernels x v0 / v3), none with scratch, none at fewer waves per SIMD than the
    epsilon-greedy closed-loop sibling of the same kernel and variant."""
    kernels = kernel_usage("lmaze_step.hip")
    new = {k: v for k, v in kernels.items() if "RolloutSampleArgs" in k or "RolloutSample8Args" in k}
    assert len(new) == 6, sorted(new)
    for name, v in new.items():
        sibling = name.replace("RolloutSample", "RolloutPolicy")
        assert sibling in kernels and sibling != name, name
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["Occupancy"] >= kernels[sibling]["Occupancy"], (name, v, kernels[sibling])
    for frag in ("21rollout_shared_kernel", "21rollout_perenv_kernel", "24rollout_shared_u8_kernel"):
        assert sum(frag in k for k in new) == 2, frag


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_returns_kernel_no_scratch():
    kernels = kernel_usage("lmaze_aux.hip")
    mine = {k: v for k, v in kernels.items() if "returns_kernel" in k}
    assert len(mine) == 1, sorted(kernels)
    (v,) = mine.values()
    assert v.get("ScratchSize", 0) == 0 and v["Occupancy"] >= 8, v
