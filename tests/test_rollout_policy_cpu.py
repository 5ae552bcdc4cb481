"""CPU: the closed-loop rollouts' C ABI without a GPU -- the symbols, every documented refusal in its order of precedence
(answered before any device call), the launch the describe call names (kernel form, envs per workgroup, LDS with the
ball-keyed table counted), the host's epsilon conversion, and what the new kernel forms need per wave."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest
import torch

from closed_loop_ref import (bare_grid_env, fields as _fields, grid_params as _params, perenv_lds as _perenv_lds, shared_lds as _shared_lds,
                             u8_lds as _u8_lds)
from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_rollout_policy", "lmaze_rollout_policy_u8", "lmaze_describe_rollout_policy")


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
    for needle in ("0x80000000", "2^63", "bit 8"):          # the stream separation, its epoch bound, the hint that is not read
        assert needle in header


def _call(abi, u8=False, variant="v0", G=11, mode=None, T=6, n=100, policy=64, key_mode=0, obs_t=None, every=0, params=True,
          layout=64, ball=64, goal=None, obs=None):
    """Fabricated device addresses: every refusal is returned before anything is dereferenced or queued."""
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else (abi.VARIANT_V0 if variant == "v0" else variant), G,
                        abi.LAYOUT_SHARED if mode is None else mode, 100, -1.0, -0.01, 100.0)
    fn = abi.lib.lmaze_rollout_policy_u8 if u8 else abi.lib.lmaze_rollout_policy
    return fn(C.byref(p) if params else None, layout, policy, key_mode, 0, T, ball, goal, 64, 64, 64, None, obs, None, None, None,
              None, n, 1, 1, 0, 0, obs_t, every, None)


@pytest.mark.parametrize("u8", [False, True])
def test_refusals_in_order_of_precedence(abi, u8):
    kw = dict(u8=u8)
    # 1. the recording request, before anything else -- even NULL params or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, n=-1, params=False, **kw) == E_NULL
    assert _call(abi, every=-1, policy=None, key_mode=7, **kw) == E_COUNT
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
        assert _call(abi, key_mode=km, policy=None, **kw) == E_COUNT
        assert _call(abi, key_mode=km, T=0, **kw) == E_COUNT
        assert _call(abi, variant="v3", key_mode=km, goal=64, **kw) == E_COUNT
    assert _call(abi, key_mode=1, policy=None, **kw) == E_VARIANT
    assert _call(abi, key_mode=1, n=0, **kw) == E_VARIANT
    # 4. pointers: the table among them; then alignment
    assert _call(abi, policy=None, **kw) == E_NULL
    assert _call(abi, variant="v3", key_mode=1, policy=None, goal=64, **kw) == E_NULL
    assert _call(abi, variant="v3", key_mode=1, goal=None, **kw) == E_NULL
    assert _call(abi, layout=None, **kw) == E_NULL
    assert _call(abi, policy=None, ball=68, **kw) == E_NULL          # NULL before alignment
    assert _call(abi, ball=68, **kw) == E_ALIGN
    assert _call(abi, obs=4096 + 8, **kw) == E_ALIGN
    if not u8:
        assert _call(abi, layout=72, **kw) == E_ALIGN


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("variant,key_mode", [("v0", 0), ("v3", 0), ("v3", 1)])
@pytest.mark.parametrize("T,n", [(0, 100), (6, 0), (0, 0)])
def test_nothing_to_do_reads_no_pointer(abi, u8, variant, key_mode, T, n):
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, 11, abi.LAYOUT_SHARED, 100, -1.0, -0.01, 100.0)
    fn = abi.lib.lmaze_rollout_policy_u8 if u8 else abi.lib.lmaze_rollout_policy
    none = (None,) * 11
    assert fn(C.byref(p), None, None, key_mode, 123, T, *none, n, 1, 1, 0, 0, None, 0, None) == 0
    assert fn(C.byref(p), None, None, key_mode, 123, T, *none, n, 1, 1, 0, 0, None, 3 if T < 3 else 7, None) == 0   # T / k == 0 slots
    assert fn(C.byref(p), None, None, key_mode, 123, -1, *none, n, 1, 1, 0, 0, None, 0, None) == E_COUNT


def _table(G):
    return (G * G + 15) & ~15


@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "ball"), ("v3", "goal")])
def test_describe_shared(abi, variant, key):
    """Shared layouts: the closed-loop form of rollout_shared_kernel at the recording form's envs per workgroup -- on-die 8x8
    included (no wave8 form), T == 1 and launch_hint bit 8 included (no T-launch fallback) -- with the table in the LDS."""
    S = abi.LAYOUT_SHARED
    for G, n, T, hint, epb in [(11, 65536, 64, 0, 64), (11, 1 << 20, 64, 0, 64), (12, 16384, 64, 0, 32), (11, 777, 9, 0, 16),
                               (8, 65536, 16, 0, 64), (11, 65536, 1, 0, 64), (11, 65536, 16, 0x100, 64), (32, 4099, 5, 0, 16)]:
        line = abi.describe_rollout_policy(_params(abi, variant, G, S, hint), n, T, obs_every=3 if T >= 3 else 0, key=key)
        head = "rollout_shared_kernel<v%s, policy=%s%s> T=%d every=%d " % (variant[1], key, ", obs_t" if T >= 3 else "", T,
                                                                         3 if T >= 3 else 0)
        assert line.startswith(head), line
        f = _fields(line)
        assert f["envs_per_workgroup"] == epb and f["grid"] == -(-n // epb) and f["block"] == 256, line
        assert f["lds"] == _shared_lds(G, epb) + _table(G), line
    # launch_hint bits 12-14: every value; bit 15: the slots' other store policy
    for k in range(1, 8):
        f = _fields(abi.describe_rollout_policy(_params(abi, variant, 11, S, k << 12), 4099, 8, key=key))
        assert f["envs_per_workgroup"] == 4 << (k - 1) and f["lds"] == _shared_lds(11, 4 << (k - 1)) + _table(11)
    line = abi.describe_rollout_policy(_params(abi, variant, 11, S, 1 << 15), 4099, 8, obs_every=2, key=key)
    assert ", obs_t, nt> " in line


@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "goal")])
def test_describe_u8(abi, variant, key):
    S = abi.LAYOUT_SHARED
    for G, n, hint, epb in [(11, 65536, 0, 64), (11, 777, 0, 16), (12, 16384, 0, 16), (11, 4099, 1 << 12, 16),
                            (11, 4099, 6 << 12, 128), (11, 4099, 7 << 12, 256), (64, 4099, 7 << 12, 256)]:
        line = abi.describe_rollout_policy(_params(abi, variant, G, S, hint), n, 16, with_obs="u8", obs_every=0, key=key)
        assert line.startswith("rollout_shared_u8_kernel<v%s, policy=%s> T=16 every=0 " % (variant[1], key)), line
        f = _fields(line)
        assert f["envs_per_workgroup"] == epb and f["grid"] == -(-n // epb), line
        assert f["lds"] == _u8_lds(G, epb) + _table(G) <= 64 << 10, line
    # recording beyond 262 144 envs: the widest workgroups, as lmaze_rollout_obs_u8
    f = _fields(abi.describe_rollout_policy(_params(abi, variant, 11, S), 1 << 20, 16, with_obs="u8", obs_every=1, key=key))
    assert f["envs_per_workgroup"] == 256


@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "ball"), ("v3", "goal")])
def test_describe_per_env_and_the_lds_clamp(abi, variant, key):
    PE = abi.LAYOUT_PER_ENV
    for G, n, hint, epb in [(11, 16384, 0, 16), (11, 777, 0, 16), (11, 65536, 0, 64), (32, 4099, 0, 16), (18, 4099, 7 << 12, 64),
                            (64, 4099, 0, 8),             # 32 KiB of layouts per workgroup
                            (64, 4099, 5 << 12, 32),      # hinted 64: 256 KiB of layouts, halved to what fits 160 KiB
                            (64, 4099, 7 << 12, 32), (51, 4099, 5 << 12, 32), (50, 4099, 5 << 12, 64)]:
        line = abi.describe_rollout_policy(_params(abi, variant, G, PE, hint), n, 16, obs_every=4, key=key)
        assert line.startswith("rollout_perenv_kernel<v%s, policy=%s, obs_t> T=16 every=4 " % (variant[1], key)), line
        f = _fields(line)
        assert f["envs_per_workgroup"] == epb and f["grid"] == -(-n // epb), line
        assert f["lds"] == _perenv_lds(G, epb) + _table(G) <= 160 << 10, line
    for k in range(1, 8):                                   # every value of bits 12-14; at most 64 (every lane in wave 0)
        f = _fields(abi.describe_rollout_policy(_params(abi, variant, 11, PE, k << 12), 4099, 8, key=key))
        assert f["envs_per_workgroup"] == min(4 << (k - 1), 64)


def test_describe_refusals_and_empty_lines(abi):
    p = _params(abi, "v0", 11, abi.LAYOUT_SHARED)
    buf = C.create_string_buffer(256)
    d = abi.lib.lmaze_describe_rollout_policy
    assert d(C.byref(p), 100, 6, 1, 1, -1, 0, buf, 256) == E_COUNT       # these rollouts always have an obs_every
    assert d(C.byref(p), 100, 6, 1, 1, 0, 0, None, 256) == E_NULL
    assert d(None, 100, 6, 1, 1, 0, 0, buf, 256) == E_NULL
    assert d(C.byref(p), 100, 6, 1, 1, 0, 2, buf, 256) == E_COUNT
    assert d(C.byref(p), 100, 6, 1, 1, 0, 1, buf, 256) == E_VARIANT
    assert d(C.byref(p), 100, -1, 1, 1, 0, 0, buf, 256) == E_COUNT
    assert d(C.byref(_params(abi, "v0", 11, abi.LAYOUT_PER_ENV)), 100, 6, 1, 2, 0, 0, buf, 256) == E_LAYOUT
    assert d(C.byref(_params(abi, "v0", 3, abi.LAYOUT_SHARED)), 100, 6, 1, 2, 0, 0, buf, 256) == E_GRID
    assert abi.describe_rollout_policy(p, 0, 6) == "" and abi.describe_rollout_policy(p, 100, 0) == ""


def test_epsilon_conversion(abi):
    """min(floor(eps * 2^32), 2^32 - 1): exact, a double times a power of two is not rounded."""
    f = abi.epsilon_u32
    assert f(0) == 0 and f(0.0) == 0
    assert f(1) == f(1.0) == 2 ** 32 - 1
    assert f(2.0 ** -32) == 1
    assert f(2.0 ** -33) == 0
    assert f(0.1) == 429496729                              # floor(429496729.6)
    assert f(0.25) == 1 << 30 and f(0.5) == 1 << 31
    assert f(1.0 - 2.0 ** -33) == 2 ** 32 - 1               # floor(2^32 - 0.5)
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            f(bad)


# ------------------------------------------------------------- the Python surface without a device
def test_python_argument_errors_that_need_no_device(abi, monkeypatch):
    """What LmazeVecEnv.rollout_policy() and rollout_qlearn() refuse before they touch the device, in their order of
    precedence, on an env object that never saw one (G = 5, N = 8; its tensors are the host's).  Every call carries what the
    LATER refusals would object to as well, so the one that answers is the earlier one."""
    G, N = 5, 8
    S = G * G
    env = bare_grid_env(monkeypatch)
    policy, q = torch.zeros(S, dtype=torch.uint8), torch.zeros(S, 4)
    junk = dict(policy=object(), q=object(), epsilon=2.0)                   # two tables, neither a tensor, a bad epsilon
    # 1. stream capture and the online tuner, before T
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match=r"rollout_policy\(\) is not available with a device-resident epoch or while the online"):
            env.rollout_policy(-1, key="nope", **junk)
        with pytest.raises(ValueError, match=r"rollout_qlearn\(\) is not available with a device-resident epoch or while the online"):
            env.rollout_qlearn(-1, object(), epsilon=2.0)
    env._tuner = object()
    with pytest.raises(ValueError, match="while the online tuner runs"):
        env.rollout_policy(-1, key="nope", **junk)
    with pytest.raises(ValueError, match="while the online tuner runs"):
        env.rollout_qlearn(-1, object(), epsilon=2.0)
    env._tuner = None
    # 2. T, before the key
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_policy(T, key="nope", **junk)
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_qlearn(T, object(), epsilon=2.0)
    # 3. the key, before the tables are counted
    for key in ("nope", None, 0):
        with pytest.raises(ValueError, match="key must be 'ball', 'goal' or 'env'"):
            env.rollout_policy(4, key=key, **junk)
    with pytest.raises(ValueError, match="key='goal' needs the v3 variant"):
        env.rollout_policy(4, key="goal", **junk)
    env._u8 = True
    with pytest.raises(ValueError, match="key='env' needs the int32 planes"):
        env.rollout_policy(4, key="env", **junk)
    with pytest.raises(ValueError, match="key='env' needs the int32 planes"):
        env.rollout_qlearn(4, object(), epsilon=2.0)
    env._u8 = False
    env.num_envs = (2 ** 31 - 1) // S + 1
    with pytest.raises(ValueError, match=r"N \* G\*G <= 2\*\*31 - 1"):
        env.rollout_policy(4, key="env", **junk)
    with pytest.raises(ValueError, match=r"N \* G\*G <= 2\*\*31 - 1"):
        env.rollout_qlearn(4, object(), epsilon=2.0)
    env.num_envs = N
    # 4. exactly one table, before either is looked at and before epsilon
    for key in ("ball", "env"):
        for kw in (dict(), dict(policy=object(), q=object())):
            with pytest.raises(ValueError, match="exactly one of policy= and q="):
                env.rollout_policy(4, key=key, epsilon=2.0, **kw)
    # 5. q: a float tensor [S, A] on the env's device, before the table's size is asked
    for bad in (object(), [[0.0] * 4] * S, torch.zeros(S, 4, device="meta")):
        with pytest.raises(ValueError, match=r"q must be a float tensor \[S, A\] on cpu"):
            env.rollout_policy(4, q=bad, epsilon=2.0)
    for bad in (torch.zeros(S), torch.zeros(S, 4, dtype=torch.int32), torch.zeros(S, 256), torch.zeros(S, 0), torch.zeros(2, S, 4)):
        with pytest.raises(ValueError, match=r"q must be a float tensor \[S, A\] with 1 <= A <= 255"):
            env.rollout_policy(4, q=bad, epsilon=2.0)
    with pytest.raises(ValueError, match=r"q must be a float tensor \[S, A\] with 1 <= A <= 255"):
        env.rollout_policy(4, q=torch.zeros(N, S + 1, 4), key="env", epsilon=2.0)    # not [N, G*G, A]: stays 3-d
    # 6. the table: uint8, on the device, contiguous, of the key's size -- before epsilon
    for bad in (object(), policy.to(torch.int32), policy[:-1], torch.zeros(2 * S, dtype=torch.uint8)[::2],
                torch.zeros(S, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match=r"policy must be a contiguous uint8 tensor of 25 entries on cpu \(key='ball', G=5\)"):
            env.rollout_policy(4, policy=bad, epsilon=2.0)
    with pytest.raises(ValueError, match=r"policy must be a contiguous uint8 tensor of 25 entries on cpu \(key='ball', G=5\)"):
        env.rollout_policy(4, q=torch.zeros(S + 1, 4), epsilon=2.0)          # greedy_table(q) has a row too many
    env._is_v3 = True
    with pytest.raises(ValueError, match=r"of 625 entries on cpu \(key='goal', G=5\)"):
        env.rollout_policy(4, policy=policy, key="goal", epsilon=2.0)
    env._is_v3 = False
    for bad in (policy, torch.zeros(S, N, dtype=torch.uint8), torch.zeros(N, S, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"policy must be uint8 \[8, 25\] or flat \[200\] \(key='env'\)"):
            env.rollout_policy(4, policy=bad, key="env", epsilon=2.0)
    for bad in (object(), torch.zeros(N, S, dtype=torch.int32), torch.zeros(N, 2 * S, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match=r"of 200 entries on cpu \(key='env', N=8, G=5\)"):
            env.rollout_policy(4, policy=bad, key="env", epsilon=2.0)
    with pytest.raises(ValueError, match=r"of 200 entries on cpu \(key='env', N=8, G=5\)"):
        env.rollout_policy(4, q=torch.zeros(N * S + 1, 4), key="env", epsilon=2.0)
    odd = torch.zeros(N * S + 4, dtype=torch.uint8)
    assert odd.data_ptr() % 4 == 0
    for off in (1, 2, 3):
        with pytest.raises(ValueError, match=r"policy must be 4-byte aligned \(key='env'\)"):
            env.rollout_policy(4, policy=odd[off:off + N * S], key="env", epsilon=2.0)
    # 7. epsilon, before the recording request; then that, which only an accepted table reaches
    for key, tables in (("ball", (dict(policy=policy), dict(q=q), dict(q=torch.zeros(S, 7, dtype=torch.float64)))),
                        ("env", (dict(policy=torch.zeros(N, S, dtype=torch.uint8)), dict(policy=torch.zeros(N * S, dtype=torch.uint8)),
                                 dict(q=torch.zeros(N, S, 4)), dict(q=torch.zeros(N * S, 4)), dict(policy=odd[4:])))):
        for kw in tables:
            for bad in (-0.1, 1.5, float("nan"), 2.0):
                with pytest.raises(ValueError, match=r"epsilon must be in \[0, 1\]"):
                    env.rollout_policy(4, key=key, epsilon=bad, obs_every=-1, **kw)
            with pytest.raises(ValueError, match="obs_every must be >= 0"):
                env.rollout_policy(4, key=key, obs_every=-1, **kw)
    with pytest.raises(ValueError, match="obs_every=0 records the final planes only"):
        env.rollout_policy(4, policy=policy, obs_t=torch.zeros(1))
    # rollout_qlearn(): q is the learner's own memory -- float32, contiguous, 16-byte aligned, one of two shapes, never copied
    ql = torch.zeros(N, S, 4)
    flat = torch.zeros(N * S * 4 + 1)
    assert flat.data_ptr() % 16 == 0
    for bad in (object(), None, ql.double(), ql.to(torch.int32), torch.zeros(N, S, 8)[:, :, ::2], torch.zeros(N, 4, S).transpose(1, 2),
                torch.zeros(S, 4), torch.zeros(N, S), torch.zeros(N * S * 4), torch.zeros(N, S, 4, device="meta"),
                flat[1:].view(N, S, 4), flat[1:].view(N * S, 4)):
        with pytest.raises(ValueError, match=r"q must be a contiguous, 16-byte aligned float32 tensor \[8, 25, 4\] or \[200, 4\] on cpu: "
                                             r"it is updated in place"):
            env.rollout_qlearn(4, bad, epsilon=2.0, td_t=object())
    for bad in (object(), torch.zeros(4, N, dtype=torch.float64), torch.zeros(3, N), torch.zeros(4, N + 1), torch.zeros(4 * N),
                torch.zeros(4, 2 * N)[:, ::2], torch.zeros(N, 4).t(), torch.zeros(4, N, device="meta")):
        with pytest.raises(ValueError, match=r"td_t must be a contiguous float32 tensor \[4, 8\] on cpu"):
            env.rollout_qlearn(4, ql, epsilon=2.0, td_t=bad)
    for good in (ql, ql.view(N * S, 4)):
        for td in (None, torch.zeros(4, N)):
            with pytest.raises(ValueError, match=r"epsilon must be in \[0, 1\]"):
                env.rollout_qlearn(4, good, epsilon=2.0, td_t=td, obs_every=-1)
            with pytest.raises(ValueError, match="obs_every must be >= 0"):
                env.rollout_qlearn(4, good, td_t=td, obs_every=-1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_closed_loop_kernels_no_scratch_and_occupancy():
    """Six new instantiations (three kernels x v0 / v3), none with scratch.  A closed-loop form is its recording twin with the
    action load replaced by a table lookup and a Philox draw, and these kernels are latency-bound, so the shared and per-env
    forms keep the twin's waves per SIMD (8 / 7).  The u8 forms keep 5, the v3 twin's: at the v0 twin's 6 the v0 form
    spills 12 bytes per lane (lmaze_step.hip)."""
    kernels = kernel_usage("lmaze_step.hip")
    new = {k: v for k, v in kernels.items() if "RolloutPolicyArgs" in k or "RolloutPolicy8Args" in k}
    assert len(new) == 6, sorted(new)
    for name, v in new.items():
        u8 = "RolloutPolicy8Args" in name
        twin = name.replace("ELb1EEEvNS_8StepArgsENS_18RolloutPolicy8Args", "EEEvNS_8StepArgsENS_15RolloutObs8Args")
        twin = twin.replace("17RolloutPolicyArgs", "14RolloutObsArgs")
        assert twin in kernels and twin != name, name
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["Occupancy"] >= (5 if u8 else kernels[twin]["Occupancy"]), (name, v, kernels[twin])
    for frag in ("21rollout_shared_kernel", "21rollout_perenv_kernel", "24rollout_shared_u8_kernel"):
        assert sum(frag in k for k in new) == 2, frag
