"""CPU: the sampling closed-loop foveal rollout's C ABI without a GPU -- the two symbols and the header's statement of the
rule, every documented refusal in its order (answered before any device call, on fabricated pointers), the launch the
describe call names on both sides of the 16 384-byte table rule, the Python argument errors that need no device,
sampling_thresholds(actions=25) against a numpy float64 restatement, the compare rule of lmaze_foveal_sample.h compiled for
the host under the address and undefined-behaviour sanitizers, what the new kernels need per wave next to their
epsilon-greedy twins, and -- from the oracle's side alone -- that every case of the GPU module takes every path."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import foveal_sample_ref as R
from closed_loop_ref import fields as _fields
from closed_loop_ref import test_numpy_philox_is_the_oracles  # noqa: F401  (collected here: the restatement draws with philox)
from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_foveal_rollout_sample", "lmaze_describe_foveal_rollout_sample")
MAX_ENVS = 1 << 30
VID = {"v1": 1, "v2": 2, "v4": 4, "v5": 5, "v6": 6}


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
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    pkg = importlib.import_module("gym-lmaze_amd")
    assert callable(pkg.LmazeFovealVecEnv.rollout_sample) and callable(abi.describe_foveal_rollout_sample)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("uint32[G G, 4]", "uint32[L G G, 24]", "sum over k of (r >= c_k)", "binary search is not equivalent",
                   "at most 16 384", "six 128-bit reads", "loaded with the rest and ignored", "always in 0..A-1",
                   "v5/v6 are refused with LMAZE_E_VARIANT", "whether or not auto_reset is set"):
        assert phrase in flat, phrase


def _params(abi, variant="v2", G=18, L=5, hint=0):
    return abi.LmazeFovealParams(VID.get(variant, variant), G, L, 50, 10, -1.0, -0.01, 100.0, hint)


def _bufs(abi, variant="v2", **kw):
    """fabricated device addresses for what the variant's step needs; nothing is dereferenced before the refusals"""
    names = ["ball_xy", "step_count", "reward", "done", "obs"]
    names += ["fgoal_xy", "foveal_step_count", "foveal_reward", "foveal_done"] if variant == "v1" else ["goal_xy", "layout_id"]
    if variant == "v4":
        names += ["visit", "visit_clock"]
    ptrs = {n: 4096 for n in names}
    ptrs.update(kw)
    return abi.LmazeFovealBuffers(**ptrs)


def _call(abi, variant="v2", G=18, L=5, hint=0, params=True, layouts=64, thresholds=64, T=6, bufs=True, n=100, obs_t=None, every=0,
          **bkw):
    p = _params(abi, variant, G, L, hint)
    b = _bufs(abi, variant if variant in ("v1", "v2", "v4") else "v4", **bkw)
    return abi.lib.lmaze_foveal_rollout_sample(C.byref(p) if params else None, layouts, thresholds, T, C.byref(b) if bufs else None,
                                               n, 1, 1, 0, 0, None, None, None, None, None, None, obs_t, every, None)


@pytest.mark.parametrize("variant", ["v1", "v2", "v4"])
def test_refusals_in_their_documented_order(abi, variant):
    """lmaze_foveal_rollout_policy's, in its order, with `thresholds` in the place of `policy`"""
    kw = dict(variant=variant, G=14 if variant == "v1" else 18, L=1 if variant == "v1" else 5)
    # 1. the recording request, before anything else -- even NULL params, a two-level variant or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, params=False, n=-1, **kw) == E_NULL
    assert _call(abi, every=-1, params=False, thresholds=None, T=-1, **kw) == E_COUNT
    assert _call(abi, variant="v5", obs_t=4096 + 8, every=1) == E_ALIGN
    # 2. the params' own, before the variant's refusal and the counts
    assert _call(abi, params=False, T=-1, **kw) == E_NULL
    assert _call(abi, variant=3, T=-1) == E_VARIANT
    assert _call(abi, variant=0, n=-1) == E_VARIANT
    assert _call(abi, **dict(kw, G=4), T=-1) == E_GRID
    assert _call(abi, **dict(kw, G=65), n=-1) == E_GRID
    assert _call(abi, variant="v5", G=4) == E_GRID                        # before 3.
    assert _call(abi, **dict(kw, L=0), T=-1) == E_LAYOUT
    assert _call(abi, **dict(kw, L=17), thresholds=None) == E_LAYOUT
    assert _call(abi, hint=0x400, T=-1, **kw) == E_LAYOUT
    # 3. v5/v6, before the counts and before "nothing to do"
    for two in ("v5", "v6"):
        assert _call(abi, variant=two) == E_VARIANT
        assert _call(abi, variant=two, T=-1, n=-1) == E_VARIANT
        assert _call(abi, variant=two, T=0) == E_VARIANT
        assert _call(abi, variant=two, n=0, thresholds=None, layouts=None, bufs=False) == E_VARIANT
    # 4. the counts, before "nothing to do" and before the pointers
    assert _call(abi, T=-1, **kw) == E_COUNT
    assert _call(abi, n=-1, **kw) == E_COUNT
    assert _call(abi, n=MAX_ENVS + 1, **kw) == E_COUNT
    assert _call(abi, T=-1, n=0, **kw) == E_COUNT
    assert _call(abi, T=0, n=-1, **kw) == E_COUNT
    assert _call(abi, T=-1, thresholds=None, layouts=None, bufs=False, **kw) == E_COUNT
    # 5. nothing to do: 0 whatever the pointers, odd ones included
    for T, n in ((0, 100), (6, 0), (0, 0), (0, MAX_ENVS)):
        assert _call(abi, T=T, n=n, thresholds=None, layouts=None, bufs=False, **kw) == 0
        assert _call(abi, T=T, n=n, thresholds=65, layouts=67, obs=4096 + 4, **kw) == 0
        assert _call(abi, T=T, n=n, thresholds=None, obs_t=4096, every=4, **kw) == 0
    assert _call(abi, T=2, n=0, obs_t=None, every=3, **kw) == 0           # T / every == 0: no slot wanted, obs_t may be NULL
    # 6. the pointers, thresholds among them; then alignment, the table's among it
    assert _call(abi, thresholds=None, **kw) == E_NULL
    assert _call(abi, layouts=None, **kw) == E_NULL
    assert _call(abi, bufs=False, **kw) == E_NULL
    for name in ("ball_xy", "step_count", "reward", "done", "obs") + (("fgoal_xy", "foveal_done") if variant == "v1" else
                                                                      ("goal_xy", "layout_id")):
        assert _call(abi, **dict(kw, **{name: None})) == E_NULL, name
        assert _call(abi, thresholds=64 + 4, **dict(kw, **{name: None})) == E_NULL, name      # NULL before alignment
    if variant == "v4":
        assert _call(abi, visit=None, **kw) == E_NULL and _call(abi, visit_clock=None, **kw) == E_NULL
        assert _call(abi, visit=4096 + 32, **kw) == E_ALIGN
    assert _call(abi, thresholds=None, obs=4096 + 4, **kw) == E_NULL      # NULL before alignment
    assert _call(abi, obs=4096 + 4, **kw) == E_ALIGN
    for off in (4, 8, 12, 1):
        assert _call(abi, thresholds=64 + off, **kw) == E_ALIGN


def _foveal_lds(variant, G, L, epb):
    """lmaze_foveal_defs.h foveal_lds: per-env strings and flags, row masks, layout characters, v4's visit samples"""
    L = 1 if variant == "v1" else L
    lds = epb * 64 + (3 * L * G + 2 * G) * 8 + ((L * G * G + 15) & ~15)
    return lds + (epb * (2 * 25 * 4 + 8) if variant == "v4" else 0)


DESCRIBED = [(s.variant, s.G, s.L or (1 if s.variant == "v1" else 5), s.table) for s in R.SHAPES] + [
    ("v2", 13, 1, "lds"), ("v4", 13, 1, "lds"),          # 16 224 B; an odd G and an odd L: the rows start 8 bytes further on
    ("v2", 14, 1, "global"), ("v1", 32, 1, "lds"),       # 18 816 B; 16 384 B, the rule's last size
    ("v1", 64, 1, "global"), ("v4", 64, 16, "global"), ("v2", 5, 1, "lds")]


@pytest.mark.parametrize("variant,G,L,side", DESCRIBED)
def test_describe_names_the_kernel_and_where_the_table_lives(abi, variant, G, L, side):
    """at most 16 384 bytes of thresholds: staged in LDS on the next 16-byte boundary behind the layout characters and counted
    in the launch's LDS; above: global, no extra LDS.  A rule, whatever n, T, the reset, the recording and the hint."""
    table = R.table_bytes(variant, G, L)
    assert (table <= R.LDS_RULE) == (side == "lds")
    GN = 14 if variant == "v1" else 18
    for n, hint, epb in ((333, 0, 32), (333, 0x30, 64), (333, 0x40, 128), (333, 0x120, 32), (40000, 0, 64), (1 << 20, 0x20, 32)):
        for ar in (0, 1):
            for every in (0, 1, 5):
                line = abi.describe_foveal_rollout_sample(_params(abi, variant, G, L, hint), n, 24, ar, every)
                assert line.startswith("foveal_rollout_sample_kernel<v%s, " % variant[1]), line
                f = _fields(line)
                base = _foveal_lds(variant, G, L, f["envs_per_workgroup"])
                want = ((base + 15) & ~15) + table if side == "lds" else base
                if want <= 64 << 10:                                     # the launcher assumes 64 KiB without a device
                    assert f["envs_per_workgroup"] == epb, line
                assert "%s, %d, %s%s> table=%s T=24 " % (f["envs_per_workgroup"], G if G == GN else 0,
                                                          "fused-reset" if ar else "plain", ", obs_t" if every else "", side) in line, line
                assert f["lds"] == want and f["block"] == 256, (line, want)
                chunks = ((hint >> 8) & 3) + 1
                assert f["chunks"] == chunks and f["grid"] == -(-(-(-n // f["envs_per_workgroup"])) // chunks), line
    # bits 0-3: the cap pads the LDS and is reported
    f = _fields(abi.describe_foveal_rollout_sample(_params(abi, variant, G, L, 0x25), 333, 24, 1, 0))
    assert f["workgroups_per_cu"] in (0, 5) and f["lds"] >= _foveal_lds(variant, G, L, 32)


def test_the_staged_table_counts_in_the_halving_fallback(abi):
    """v4 at 128 envs per workgroup with 16 layouts of 64 x 64 needs more than 64 KiB: the launcher halves the envs"""
    line = abi.describe_foveal_rollout_sample(_params(abi, "v4", 64, 16, 0x40), 1 << 20, 24, 1, 0)
    f = _fields(line)
    if f["envs_per_workgroup"] < 128:                                    # 64 KiB assumed without a device
        assert _foveal_lds("v4", 64, 16, 128) > 64 << 10 and f["lds"] == _foveal_lds("v4", 64, 16, f["envs_per_workgroup"]), line
    # v4, one 12 x 12 layout: 13 824 B of staged rows are part of the sum that is compared with the limit
    f = _fields(abi.describe_foveal_rollout_sample(_params(abi, "v4", 12, 1, 0x40), 1 << 20, 24, 1, 0))
    assert f["lds"] == ((_foveal_lds("v4", 12, 1, f["envs_per_workgroup"]) + 15) & ~15) + 13824


def test_describe_the_issue_line(abi):
    line = abi.describe_foveal_rollout_sample(_params(abi, "v2", 18, 5), 333, 24, 1, 3)
    assert line.startswith("foveal_rollout_sample_kernel<v2, 32, 18, fused-reset, obs_t> table=global T=24 grid="), line


def test_describe_refusals_and_empty_lines(abi):
    d = abi.lib.lmaze_describe_foveal_rollout_sample
    buf = C.create_string_buffer(256)
    p = _params(abi)
    assert d(C.byref(p), 100, 6, 1, 0, None, 256) == E_NULL
    assert d(C.byref(p), 100, 6, 1, 0, buf, 0) == E_NULL
    assert d(None, -1, -1, 1, -1, None, 256) == E_NULL                  # the text first
    assert d(C.byref(p), 100, 6, 1, -1, buf, 256) == E_COUNT
    assert d(None, 100, 6, 1, -1, buf, 256) == E_COUNT                  # the recording request before the params
    assert d(None, 100, 6, 1, 0, buf, 256) == E_NULL
    assert d(C.byref(_params(abi, 3)), 100, -1, 1, 0, buf, 256) == E_VARIANT
    assert d(C.byref(_params(abi, "v2", 4)), 100, -1, 1, 0, buf, 256) == E_GRID
    assert d(C.byref(_params(abi, "v2", 18, 17)), 100, -1, 1, 0, buf, 256) == E_LAYOUT
    assert d(C.byref(_params(abi, "v2", 18, 5, 0x400)), 100, -1, 1, 0, buf, 256) == E_LAYOUT
    for two in ("v5", "v6"):
        assert d(C.byref(_params(abi, two)), 100, 6, 1, 0, buf, 256) == E_VARIANT
        assert d(C.byref(_params(abi, two)), 0, -1, 1, 3, buf, 256) == E_VARIANT
    assert d(C.byref(p), 100, -1, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), -1, 6, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), MAX_ENVS + 1, 6, 1, 3, buf, 256) == E_COUNT
    buf.value = b"stale"
    assert d(C.byref(p), 0, 6, 1, 0, buf, 256) == 0 and buf.value == b""
    buf.value = b"stale"
    assert d(C.byref(p), 100, 0, 1, 3, buf, 256) == 0 and buf.value == b""
    assert d(C.byref(p), 100, 6, 1, 0, buf, 8) == 0 and buf.value == b"foveal_"      # truncated to len, always terminated
    # no grid size is refused: v1 records at any grid
    assert ", 0, plain, obs_t> table=lds" in abi.describe_foveal_rollout_sample(_params(abi, "v1", 13, 1), 100, 6, 0, 2)


def test_python_argument_errors_that_need_no_device(abi):
    """What rollout_sample() refuses before it touches the device, on an env object that never saw one."""
    pkg = importlib.import_module("gym-lmaze_amd")
    env = object.__new__(pkg.LmazeFovealVecEnv)
    env.variant, env._two_level, env.num_envs, env.grid, env.n_layouts = "v2", False, 8, 18, 5
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_sample(T, probs=object())
    with pytest.raises(ValueError, match="exactly one of"):
        env.rollout_sample(4)
    for kw in (dict(probs=object(), logits=object()), dict(probs=object(), thresholds=object()),
               dict(logits=object(), thresholds=object()), dict(probs=object(), logits=object(), thresholds=object())):
        with pytest.raises(ValueError, match="exactly one of"):
            env.rollout_sample(4, **kw)
    env.variant, env._two_level = "v5", True
    with pytest.raises(ValueError, match="v5/v6"):
        env.rollout_sample(4, probs=object())


# ------------------------------------------------------------- the converter
def _special_rows(A, rs):
    p = rs.rand(64, A)
    p[0] = 0.0
    p[0, 0] = 1.0                                  # one-hot at action 0
    p[1] = 0.0
    p[1, A - 1] = 1.0                              # one-hot at the last action
    p[2] = 0.25                                    # all equal
    p[3] = 1e-30
    p[4] = 1e30
    p[5:20][rs.rand(15, A) < 0.5] = 0.0            # rows with zero entries
    p[5:20, A - 1] += 1e-3
    p[20] = 0.0
    p[20, A // 2] = 7.0                            # one-hot in the middle
    p[21, :A - 1] = 0.0                            # everything on the last action but scaled
    p[22, 1:] = 0.0
    return p


@pytest.mark.parametrize("A", [25, 4, 2, 7])
def test_sampling_thresholds_is_the_numpy_restatement(abi, A):
    rs = np.random.RandomState(A)
    for p in (_special_rows(A, rs), rs.rand(500, A) ** 4, rs.rand(300, A).astype(np.float32)):
        got = abi.sampling_thresholds(torch.from_numpy(p), actions=A)
        want = R.thresholds(p)
        assert got.dtype == torch.uint32 and tuple(got.shape) == (p.shape[0], R.row_words(A))
        assert (got.view(torch.int32).numpy().view(np.uint32) == want).all()
        c = want[:, :A - 1].astype(np.int64)
        assert (np.diff(c, axis=1) >= 0).all()                          # monotone
    sp = R.thresholds(_special_rows(A, np.random.RandomState(A)))
    assert (sp[0, :A - 1] == 0xFFFFFFFF).all()                          # one-hot at 0: a cumulative 1 is stored as 1 - 2^-32
    assert (sp[1, :A - 1] == 0).all()                                   # one-hot at the last: every draw reaches every word
    w = R.widths(sp, A)
    assert (np.abs(w[2] - (1 << 32) / A) <= 1).all()                    # all equal: 2^32 / A draws each, to rounding
    zero = _special_rows(A, np.random.RandomState(A))[:, :A - 1] == 0
    assert (w[:, :A - 1][zero] == 0).all()                              # a zero weight below the last action: no draw gives it


def test_sampling_thresholds_default_is_what_it_was(abi):
    rs = np.random.RandomState(11)
    p = torch.from_numpy(_special_rows(4, rs))
    a, b = abi.sampling_thresholds(p), abi.sampling_thresholds(p, actions=4)
    assert a.dtype == b.dtype == torch.uint32 and tuple(a.shape) == (64, 4)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool((a.view(torch.int32)[:, 3] == 0).all())
    with pytest.raises(ValueError):
        abi.sampling_thresholds(torch.rand(8, 5))                       # the default stays the grid envs' four actions
    with pytest.raises(ValueError):
        abi.sampling_thresholds(torch.rand(8, 4), actions=25)
    for bad in (torch.full((2, 25), -1.0), torch.full((2, 25), float("nan")), torch.zeros(2, 25), torch.full((2, 25), float("inf")),
                torch.ones(25), torch.ones(2, 25, dtype=torch.int32)):
        with pytest.raises(ValueError):
            abi.sampling_thresholds(bad, actions=25)
    with pytest.raises(ValueError):
        abi.sampling_thresholds(torch.rand(8, 1), actions=1)


# ------------------------------------------------------------- lmaze_foveal_sample.h on the host
@pytest.fixture(scope="module")
def sample_host(tmp_path_factory):
    """tests/csrc/foveal_sample_host.cpp: a stand-alone program around lmaze_foveal_sample.h, built with the address and
    undefined-behaviour sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("sample")
    exe = str(tmp / "foveal_sample_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "csrc", "foveal_sample_host.cpp")])

    def run(A, rows, r):
        m = len(r)
        src, dst = str(tmp / "in"), str(tmp / "out")
        with open(src, "wb") as fh:
            fh.write(np.array([m], np.int64).tobytes() + np.array([A], np.int32).tobytes())
            fh.write(np.ascontiguousarray(rows, dtype=np.uint32).tobytes())
            fh.write(np.ascontiguousarray(r, dtype=np.uint32).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        got = np.frombuffer(open(dst, "rb").read(), np.int32)
        assert got[0] == R.row_words(A) and got.size == m + 1
        return got[1:]
    return run


@pytest.mark.parametrize("A", [4, 25])
def test_host_compare_rule_is_the_numpy_one(sample_host, A):
    """Random monotone rows (the converter's) and unsorted rows, draws at 0, c_k - 1, c_k, c_k + 1 and 2^32 - 1 and random."""
    rs = np.random.RandomState(A + 40)
    W, m = R.row_words(A), 6000
    mono = R.thresholds(rs.rand(m // 2, A) ** 4 * (rs.rand(m // 2, A) > 0.3) + 1e-12)
    raw = rs.randint(0, 1 << 32, (m - m // 2, W), dtype=np.uint64).astype(np.uint32)
    rows = np.concatenate([mono, raw])
    rows[:, W - 1] = rs.randint(0, 1 << 32, m, dtype=np.uint64) if A == 4 else rows[:, W - 1]     # the reserved word: anything
    k = rs.randint(0, A - 1, m)
    ck = rows[np.arange(m), k].astype(np.int64)
    pick = rs.randint(0, 6, m)
    r = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4],
                  [np.zeros(m, np.int64), np.full(m, (1 << 32) - 1), np.clip(ck - 1, 0, None), ck, np.clip(ck + 1, None, (1 << 32) - 1)],
                  rs.randint(0, 1 << 32, m, dtype=np.uint64).astype(np.int64)).astype(np.uint64)
    got = sample_host(A, rows, r)
    want = R.sample_action(rows, r, A - 1)
    assert (got == want).all()
    assert got.min() == 0 and got.max() == A - 1
    # the unsorted rows pin the sum: a search for the first threshold above the draw gives another action for many of them
    first_above = np.array([int(np.argmax(np.append(rows[i, :A - 1].astype(np.uint64) > r[i], True))) for i in range(m // 2, m)])
    assert (first_above != want[m // 2:]).any()
    assert (np.array([int(np.argmax(np.append(rows[i, :A - 1].astype(np.uint64) > r[i], True))) for i in range(m // 2)])
            == want[:m // 2]).all()                                     # and for monotone rows the two agree
    if A == 4:
        from closed_loop_ref import sample_action as grid_rule
        assert (grid_rule(rows, r) == want).all()                       # v1's table is the grid envs' format and rule


# ------------------------------------------------------------- the numpy restatement's own parts
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_case_takes_every_path(shape):
    """The GPU module's coverage conditions, from the oracle's side alone."""
    assert (R.table_bytes(shape.variant, shape.G, R.lay_of(shape, R.SEEDS[shape])[1].shape[0]) <= R.LDS_RULE) == (shape.table == "lds")
    for ar in (0, 1):
        lays, lay, probs, table, p, start, start_visit, out = R.case(shape, ar, None, R.SEEDS[shape])
        A = R.n_actions(shape.variant)
        assert table.shape == (lay.shape[0] * shape.G * shape.G, R.row_words(A)) and table.dtype == np.uint32
        assert (probs == 0).mean() > 0.25 and ((probs > 0).sum(axis=1) == 1).mean() > 0.03      # zero entries, one-hot rows
        R.check_coverage(out.coverage, ar, R.MIN_GOALS[shape])
        assert out.rows["key"].min() >= 0 and out.rows["key"].max() < table.shape[0]
        assert out.rows["action"].min() == 0 and out.rows["action"].max() == A - 1


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_no_scratch_and_within_one_wave_of_their_twins():
    """72 new kernels (v1 / v2 / v4 x 32 / 64 / 128 envs x specialised / generic grid x plain / fused x recording or not), none
    with scratch, none below 4 waves per SIMD, each at most one wave below its epsilon-greedy twin <variant, EPB, G, AR> /
    REC of lmaze_foveal_policy.hip compiled here from the same tree."""
    new = kernel_usage("lmaze_foveal_sample.hip")
    old = kernel_usage("lmaze_foveal_policy.hip")
    pat = re.compile(r"_ZN5lmaze28foveal_rollout_sample_kernelI(Li\dELi\d+ELi\d+ELb[01]E)EEvNS_10FovealArgsENS_(13FovealRollSmp|16FovealRollObsSmp)E")
    assert len(new) == 72 and len(old) == 72, sorted(new)
    for name, v in new.items():
        m = pat.fullmatch(name)
        assert m, name
        rec = m.group(2).startswith("16")
        twin = "_ZN5lmaze28foveal_rollout_policy_kernelI%sEEvNS_10FovealArgsENS_%sE" % (m.group(1), "16FovealRollObsPol" if rec else "13FovealRollPol")
        assert v.get("ScratchSize", 0) == 0 and v["Occupancy"] >= 4, (name, v)
        assert old[twin].get("ScratchSize", 0) == 0
        assert v["Occupancy"] >= old[twin]["Occupancy"] - 1, (name, v, old[twin])
