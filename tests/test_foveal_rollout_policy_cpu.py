"""CPU: the closed-loop foveal rollout's C ABI without a GPU -- the two symbols and the header's statement of the rule, every
documented refusal in its order (answered before any device call, on fabricated pointers), the launch the describe call
names on both sides of the table rule, the Python argument errors that need no device, the selection rule of
lmaze_foveal_select.h compiled for the host under the address and undefined-behaviour sanitizers against its numpy
restatement, the numpy Philox against the oracle's, and what the new kernels need per wave next to their open-loop twins."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import foveal_policy_ref as R
from closed_loop_ref import fields as _fields
from closed_loop_ref import test_numpy_philox_is_the_oracles  # noqa: F401  (collected here: the restatement draws with philox)
from helpers import HIPCC, kernel_usage
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_foveal_rollout_policy", "lmaze_describe_foveal_rollout_policy")
MAX_ENVS = 1 << 30


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
    assert callable(pkg.LmazeFovealVecEnv.rollout_policy) and callable(pkg.LmazeFovealVecEnv.state_keys)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("(r.y A) >> 32", "ep_hi ^ 0x80000000", "skipped ones included", "table=lds / table=global", "L G G <= 8192",
                   "reset, then no step", "v5/v6 are refused", "No grid size is refused", "whether or not auto_reset is set"):
        assert phrase in flat, phrase


VID = {"v1": 1, "v2": 2, "v4": 4, "v5": 5, "v6": 6}


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


def _call(abi, variant="v2", G=18, L=5, hint=0, params=True, layouts=64, policy=64, T=6, bufs=True, n=100, obs_t=None, every=0, **bkw):
    p = _params(abi, variant, G, L, hint)
    b = _bufs(abi, variant if variant in ("v1", "v2", "v4") else "v4", **bkw)
    return abi.lib.lmaze_foveal_rollout_policy(C.byref(p) if params else None, layouts, policy, 123, T, C.byref(b) if bufs else None,
                                               n, 1, 1, 0, 0, None, None, None, None, None, None, obs_t, every, None)


@pytest.mark.parametrize("variant", ["v1", "v2", "v4"])
def test_refusals_in_their_documented_order(abi, variant):
    kw = dict(variant=variant, G=14 if variant == "v1" else 18, L=1 if variant == "v1" else 5)
    # 1. the recording request, before anything else -- even NULL params, a two-level variant or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, params=False, n=-1, **kw) == E_NULL
    assert _call(abi, every=-1, params=False, policy=None, T=-1, **kw) == E_COUNT
    assert _call(abi, variant="v5", obs_t=4096 + 8, every=1) == E_ALIGN
    # 2. the params' own, before the variant's refusal and the counts
    assert _call(abi, params=False, T=-1, **kw) == E_NULL
    assert _call(abi, variant=3, T=-1) == E_VARIANT
    assert _call(abi, variant=0, n=-1) == E_VARIANT
    assert _call(abi, **dict(kw, G=4), T=-1) == E_GRID
    assert _call(abi, **dict(kw, G=65), n=-1) == E_GRID
    assert _call(abi, variant="v5", G=4) == E_GRID                        # before 3.
    assert _call(abi, **dict(kw, L=0), T=-1) == E_LAYOUT
    assert _call(abi, **dict(kw, L=17), policy=None) == E_LAYOUT
    assert _call(abi, hint=0x400, T=-1, **kw) == E_LAYOUT
    # 3. v5/v6, before the counts and before "nothing to do"
    for two in ("v5", "v6"):
        assert _call(abi, variant=two) == E_VARIANT
        assert _call(abi, variant=two, T=-1, n=-1) == E_VARIANT
        assert _call(abi, variant=two, T=0) == E_VARIANT
        assert _call(abi, variant=two, n=0, policy=None, layouts=None, bufs=False) == E_VARIANT
    # 4. the counts, before "nothing to do" and before the pointers
    assert _call(abi, T=-1, **kw) == E_COUNT
    assert _call(abi, n=-1, **kw) == E_COUNT
    assert _call(abi, n=MAX_ENVS + 1, **kw) == E_COUNT
    assert _call(abi, T=-1, n=0, **kw) == E_COUNT
    assert _call(abi, T=0, n=-1, **kw) == E_COUNT
    assert _call(abi, T=-1, policy=None, layouts=None, bufs=False, **kw) == E_COUNT
    # 5. nothing to do: 0 whatever the pointers, odd ones included
    for T, n in ((0, 100), (6, 0), (0, 0), (0, MAX_ENVS)):
        assert _call(abi, T=T, n=n, policy=None, layouts=None, bufs=False, **kw) == 0
        assert _call(abi, T=T, n=n, policy=65, layouts=67, obs=4096 + 4, **kw) == 0
        assert _call(abi, T=T, n=n, policy=None, obs_t=4096, every=4, **kw) == 0
    assert _call(abi, T=2, n=0, obs_t=None, every=3, **kw) == 0           # T / every == 0: no slot wanted, obs_t may be NULL
    # 6. the pointers, policy among them; then alignment
    assert _call(abi, policy=None, **kw) == E_NULL
    assert _call(abi, layouts=None, **kw) == E_NULL
    assert _call(abi, bufs=False, **kw) == E_NULL
    for name in ("ball_xy", "step_count", "reward", "done", "obs") + (("fgoal_xy", "foveal_done") if variant == "v1" else
                                                                      ("goal_xy", "layout_id")):
        assert _call(abi, **dict(kw, **{name: None})) == E_NULL, name
    if variant == "v4":
        assert _call(abi, visit=None, **kw) == E_NULL and _call(abi, visit_clock=None, **kw) == E_NULL
        assert _call(abi, visit=4096 + 32, **kw) == E_ALIGN
    assert _call(abi, policy=None, obs=4096 + 4, **kw) == E_NULL          # NULL before alignment
    assert _call(abi, obs=4096 + 4, **kw) == E_ALIGN


def _foveal_lds(variant, G, L, epb):
    """lmaze_foveal_defs.h foveal_lds: per-env strings and flags, row masks, layout characters, v4's visit samples"""
    L = 1 if variant == "v1" else L
    lds = epb * 64 + (3 * L * G + 2 * G) * 8 + ((L * G * G + 15) & ~15)
    return lds + (epb * (2 * 25 * 4 + 8) if variant == "v4" else 0)


@pytest.mark.parametrize("variant,G,L,side", [("v1", 14, 1, "lds"), ("v2", 18, 5, "lds"), ("v4", 18, 5, "lds"), ("v2", 12, 2, "lds"),
                                               ("v4", 24, 16, "global"), ("v2", 24, 16, "global"), ("v1", 64, 1, "lds"),
                                               ("v2", 64, 2, "lds"), ("v2", 64, 3, "global"), ("v4", 32, 8, "lds"),
                                               ("v4", 32, 9, "global")])
def test_describe_names_the_kernel_and_where_the_table_lives(abi, variant, G, L, side):
    """L G G <= 8192 bytes: staged in LDS behind the layout characters and counted in the launch's LDS; above: global, no
    extra LDS.  A rule, whatever n, T, the reset, the recording and the hint."""
    table = (1 if variant == "v1" else L) * G * G
    assert (table <= 8192) == (side == "lds")
    GN = 14 if variant == "v1" else 18
    for n, hint, epb in ((333, 0, 32), (333, 0x30, 64), (333, 0x40, 128), (333, 0x120, 32), (40000, 0, 64), (1 << 20, 0x20, 32)):
        for ar in (0, 1):
            for every in (0, 1, 5):
                line = abi.describe_foveal_rollout_policy(_params(abi, variant, G, L, hint), n, 24, ar, every)
                head = "foveal_rollout_policy_kernel<v%s, " % variant[1]
                assert line.startswith(head), line
                f = _fields(line)
                want = _foveal_lds(variant, G, L, f["envs_per_workgroup"]) + (((table + 15) & ~15) if side == "lds" else 0)
                if want <= 64 << 10:                                     # the launcher assumes 64 KiB without a device
                    assert f["envs_per_workgroup"] == epb, line
                assert "%s, %d, %s%s> table=%s T=24 " % (f["envs_per_workgroup"], G if G == GN else 0,
                                                          "fused-reset" if ar else "plain", ", obs_t" if every else "", side) in line, line
                assert f["lds"] == want and f["block"] == 256, (line, want)
                chunks = ((hint >> 8) & 3) + 1
                assert f["chunks"] == chunks and f["grid"] == -(-(-(-n // f["envs_per_workgroup"])) // chunks), line
    # bits 0-3: the cap pads the LDS and is reported
    f = _fields(abi.describe_foveal_rollout_policy(_params(abi, variant, G, L, 0x25), 333, 24, 1, 0))
    assert f["workgroups_per_cu"] in (0, 5) and f["lds"] >= _foveal_lds(variant, G, L, 32)


def test_describe_refusals_and_empty_lines(abi):
    d = abi.lib.lmaze_describe_foveal_rollout_policy
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
    # v1 records at any grid: no LMAZE_E_GRID as in lmaze_foveal_rollout_obs
    assert ", 0, plain, obs_t> table=lds" in abi.describe_foveal_rollout_policy(_params(abi, "v1", 13, 1), 100, 6, 0, 2)


def test_python_argument_errors_that_need_no_device(abi):
    """What rollout_policy() refuses before it touches the device, on an env object that never saw one."""
    pkg = importlib.import_module("gym-lmaze_amd")
    env = object.__new__(pkg.LmazeFovealVecEnv)
    env.variant, env._two_level, env.num_envs, env.grid, env.n_layouts = "v2", False, 8, 18, 5
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_policy(T, policy=object())
    with pytest.raises(ValueError, match="exactly one of"):
        env.rollout_policy(4)
    with pytest.raises(ValueError, match="exactly one of"):
        env.rollout_policy(4, policy=object(), q=object())
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            env.rollout_policy(4, policy=object(), epsilon=eps)
    env.variant, env._two_level = "v5", True
    with pytest.raises(ValueError, match="v5/v6"):
        env.rollout_policy(4, policy=object())


# ------------------------------------------------------------- the numpy restatement's own parts
def test_every_case_takes_the_paths_its_parameters_allow():
    """The GPU module's coverage conditions, here where the seeds were chosen: with the oracle alone."""
    for shape in R.SHAPES:
        for eps in (0.0, 0.25, 1.0):
            for ar in (0, 1):
                out = R.case(shape, eps, ar, None, R.SEEDS[shape])[-1]
                for path in R.expected_paths(shape.variant, eps, ar):
                    assert out.coverage[path] > 0, (shape, eps, ar, path, out.coverage)
                assert out.rows["key"].min() >= 0 and out.rows["key"].max() < R.case(shape, eps, ar, None, R.SEEDS[shape])[2].size


# ------------------------------------------------------------- lmaze_foveal_select.h on the host
@pytest.fixture(scope="module")
def select_host(tmp_path_factory):
    """tests/csrc/foveal_select_host.cpp: a stand-alone program around lmaze_foveal_select.h, built with the address and
    undefined-behaviour sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("select")
    exe = str(tmp / "foveal_select_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "csrc", "foveal_select_host.cpp")])

    def run(G, L, A, eps, table, lid, bx, by, rx, ry):
        m = len(lid)
        src, dst = str(tmp / "in"), str(tmp / "out")
        with open(src, "wb") as fh:
            fh.write(np.array([m], np.int64).tobytes() + np.array([G, L, A], np.int32).tobytes() + np.array([eps], np.uint32).tobytes())
            for a, dt in ((table, np.uint8), (lid, np.int32), (bx, np.int32), (by, np.int32), (rx, np.uint32), (ry, np.uint32)):
                fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        return np.frombuffer(open(dst, "rb").read(), np.int32).reshape(3, m)
    return run


@pytest.mark.parametrize("variant,G,L", [("v1", 14, 1), ("v2", 18, 5), ("v4", 24, 16), ("v2", 5, 1), ("v4", 64, 16)])
@pytest.mark.parametrize("eps", [0, 1, 1 << 30, (1 << 32) - 1])
def test_host_selection_rule_is_the_numpy_one(select_host, variant, G, L, eps):
    """Keys from states on and far off the grid (the table is allocated exactly: a key outside it is the sanitizer's to
    report), draws at 0, 2^32 - 1, around epsilon and on both sides of every boundary k 2^32 / A."""
    A = R.n_actions(variant)
    rs = np.random.RandomState(G * 100 + L)
    edge = np.array([0, 1, -1, G - 1, G, G + 1, -G, 1 << 30, -(1 << 30), np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int64)
    ry_edge = [0, 1, (1 << 32) - 1, (1 << 32) - 2]
    for k in range(1, A):
        b = -(-(k << 32) // A)                                          # the first r.y whose action is k
        ry_edge += [b - 1, b, b + 1]
    rx_edge = [0, (1 << 32) - 1, max(eps - 1, 0), eps, min(eps + 1, (1 << 32) - 1)]
    m = 4000
    lid = np.where(rs.rand(m) < 0.3, rs.choice(np.array([-1, -7, L, L + 3, 1 << 20], np.int64), m), rs.randint(0, L, m))
    bx = np.where(rs.rand(m) < 0.3, rs.choice(edge, m), rs.randint(0, G, m))
    by = np.where(rs.rand(m) < 0.3, rs.choice(edge, m), rs.randint(0, G, m))
    rx = np.where(rs.rand(m) < 0.5, rs.choice(np.array(rx_edge, np.uint64), m), rs.randint(0, 1 << 32, m, dtype=np.uint64))
    ry = np.where(rs.rand(m) < 0.7, rs.choice(np.array(ry_edge, np.uint64), m), rs.randint(0, 1 << 32, m, dtype=np.uint64))
    table = rs.randint(0, 256, L * G * G).astype(np.uint8)
    key, action, uniform = select_host(G, L, A, eps, table, lid, bx, by, rx, ry)
    want_key = R.keys_of(variant, G, L, lid.astype(np.int32), np.stack([bx, by], axis=1).astype(np.int32))
    if variant == "v1":                                                 # L = 1 clamps every row id to 0, as v1 has none
        assert L == 1
    assert (key == want_key).all() and key.min() >= 0 and key.max() < table.size
    want, explored = R.select(table[want_key], rx, ry, eps, A)
    assert (action == want).all()
    assert (uniform == (ry.astype(object) * A // (1 << 32)).astype(np.int64)).all() and uniform.min() == 0 and uniform.max() == A - 1
    if A == 4:
        assert (uniform == (ry >> np.uint64(30)).astype(np.int64)).all()          # the grid envs' rule
    assert explored.any() == (eps != 0) and (eps >= (1 << 32) - 1 or not explored.all())
    for k in range(1, A):                                               # the boundaries themselves
        b = -(-(k << 32) // A)
        assert R.select([0], [0], [b], 1, A)[0][0] == k and R.select([0], [0], [b - 1], 1, A)[0][0] == k - 1


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_no_scratch_and_within_one_wave_of_their_twins():
    """72 new kernels (v1 / v2 / v4 x 32 / 64 / 128 envs x specialised / generic grid x plain / fused x recording or not), none
    with scratch, none below 4 waves per SIMD, each at most one wave below its open-loop twin <variant, EPB, G, AR, REC> of
    lmaze_foveal.hip compiled here from the same tree.  v1's recording form at a generic grid has no twin (the open-loop
    one is refused there): it only has to hold the floor."""
    new = kernel_usage("lmaze_foveal_policy.hip")
    old = kernel_usage("lmaze_foveal.hip")
    pat = re.compile(r"_ZN5lmaze28foveal_rollout_policy_kernelI(Li\dELi\d+ELi\d+ELb[01]E)EEvNS_10FovealArgsENS_(13FovealRollPol|16FovealRollObsPol)E")
    mine = {k: v for k, v in new.items() if "foveal_rollout_policy_kernel" in k}
    assert len(mine) == 72 and len(new) == 72, sorted(new)
    twinless = 0
    for name, v in mine.items():
        m = pat.fullmatch(name)
        assert m, name
        rec = m.group(2).startswith("16")
        twin = "_ZN5lmaze21foveal_rollout_kernelI%sEEvNS_10FovealArgsENS_%sE" % (m.group(1), "13FovealRollObs" if rec else "10FovealRoll")
        assert v.get("ScratchSize", 0) == 0 and v["Occupancy"] >= 4, (name, v)
        if twin not in old:
            assert rec and m.group(1).startswith("Li1ELi") and "ELi0ELb" in m.group(1), name
            twinless += 1
            continue
        assert old[twin].get("ScratchSize", 0) == 0
        assert v["Occupancy"] >= old[twin]["Occupancy"] - 1, (name, v, old[twin])
    assert twinless == 6
