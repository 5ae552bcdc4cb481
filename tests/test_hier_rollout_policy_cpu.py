"""CPU: the closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_policy) without a GPU -- that the restatement's cases take
every path of the rule, the selection rule of lmaze_hier_select.h compiled for the host under the address and
undefined-behaviour sanitizers against its numpy restatement, the two symbols and the header's statement of the rule, the
launch the describe call names on both sides of the table rule for both tables, every documented refusal in its order
(answered before any device call, on fabricated pointers), what the 12 new kernels need per wave, and the Python argument
errors that need no device."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hier_policy_ref as R
from closed_loop_ref import fields as _fields
from closed_loop_ref import test_numpy_philox_is_the_oracles  # noqa: F401  (collected here: the restatement draws with philox)
from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_v5_rollout_policy", "lmaze_describe_v5_rollout_policy")
MAX_ENVS = 1 << 30
VID = {"v1": 1, "v2": 2, "v4": 4, "v5": 5, "v6": 6}
# waves per SIMD DESIGN.md 4.5 states for the recording forms (the row forms: 3, the issue's floor)
REC_WAVES = 3


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


# ------------------------------------------------------------- the restatement's own parts
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%s-G%d" % (s.variant, s.G))
def test_every_case_takes_the_paths_its_parameters_allow(shape):
    """The GPU module's coverage conditions, here where the seeds were chosen: with the oracle alone."""
    for ckey in R.CKEYS:
        for eps, peps in R.EPS:
            lays, lay, controller, planner, p, start, start_visit, out = R.case(shape, ckey, eps, peps, R.SEEDS[shape])
            for path in R.expected_paths(eps, peps):
                assert out.coverage[path] > 0, (shape, ckey, eps, peps, path, out.coverage)
            for path in set(R.PATHS) - set(R.expected_paths(eps, peps)):
                assert out.coverage[path] == 0, (shape, ckey, eps, peps, path)     # what the rates rule out never happens
            assert out.rows["key"].min() >= 0 and out.rows["key"].max() < controller.size
            planned = out.rows["goal_key"] >= 0
            assert (planned == (out.rows["goal"] >= 0)).all() and planned.any() and not planned.all()
            assert out.rows["goal_key"].max() < planner.size
            assert start["done"].any() and start["foveal_done"].any() and not (start["done"] | start["foveal_done"]).all()
            assert R.controller_side(shape, lay.shape[0], ckey) == ("lds" if ckey == "offset" else "global")
            assert (planner.size <= 8192) == (shape.planner == "lds")
            assert (controller > 3).any() and (planner > 24).any()


# ------------------------------------------------------------- lmaze_hier_select.h on the host
@pytest.fixture(scope="module")
def select_host(tmp_path_factory):
    """tests/csrc/hier_select_host.cpp: a stand-alone program around lmaze_hier_select.h, built with the address and
    undefined-behaviour sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("hier_select")
    exe = str(tmp / "hier_select_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "csrc", "hier_select_host.cpp")])

    def run(G, L, ck, eps, peps, controller, planner, ints, words):
        m = len(ints[0])
        src, dst = str(tmp / "in"), str(tmp / "out")
        with open(src, "wb") as fh:
            fh.write(np.array([m], np.int64).tobytes() + np.array([G, L, ck], np.int32).tobytes() + np.array([eps, peps], np.uint32).tobytes())
            fh.write(np.ascontiguousarray(controller, np.uint8).tobytes() + np.ascontiguousarray(planner, np.uint8).tobytes())
            for a in ints:
                fh.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
            for a in words:
                fh.write(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        return np.frombuffer(open(dst, "rb").read(), np.int32).reshape(5, m)
    return run


@pytest.mark.parametrize("G,L,ckey", [(18, 5, "offset"), (18, 5, "cell"), (24, 16, "offset"), (5, 1, "cell"), (64, 16, "offset"),
                                      (12, 2, "cell")])
@pytest.mark.parametrize("eps,peps", [(0, 0), (0, (1 << 32) - 1), ((1 << 32) - 1, 0), (1 << 30, 1 << 31), ((1 << 32) - 1, (1 << 32) - 1),
                                      (1, 1)])
def test_host_selection_rule_is_the_numpy_one(select_host, G, L, ckey, eps, peps):
    """Keys from states on and far off the grid and foveal goals at every offset -6..7 and at the ends of int32 (the tables are
    allocated exactly: a key outside them is the sanitizer's to report, an overflow the undefined-behaviour sanitizer's), draws
    at 0, 2^32 - 1, around each epsilon and on both sides of every boundary k 2^32 / 25 and k 2^30, in every word."""
    rs = np.random.RandomState(G * 100 + L)
    imax, imin = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    edge = np.array([0, 1, -1, G - 1, G, G + 1, -G, 1 << 30, -(1 << 30), imax, imin], np.int64)
    m = 6000
    lid = np.where(rs.rand(m) < 0.3, rs.choice(np.array([-1, -7, L, L + 3, 1 << 20], np.int64), m), rs.randint(0, L, m))
    bx = np.where(rs.rand(m) < 0.3, rs.choice(edge, m), rs.randint(0, G, m))
    by = np.where(rs.rand(m) < 0.3, rs.choice(edge, m), rs.randint(0, G, m))
    fgx = np.where(rs.rand(m) < 0.2, rs.choice(edge, m), np.clip(bx + rs.randint(-6, 8, m), imin, imax))
    fgy = np.where(rs.rand(m) < 0.2, rs.choice(edge, m), np.clip(by + rs.randint(-6, 8, m), imin, imax))

    def word(e, bounds):
        edges = [0, 1, (1 << 32) - 1, (1 << 32) - 2, max(e - 1, 0), e, min(e + 1, (1 << 32) - 1)]
        for b in bounds:
            edges += [b - 1, b, min(b + 1, (1 << 32) - 1)]
        return np.where(rs.rand(m) < 0.6, rs.choice(np.array(edges, np.uint64), m), rs.randint(0, 1 << 32, m, dtype=np.uint64))
    b25 = [-(-(k << 32) // 25) for k in range(1, 25)]                  # the first r.w whose goal is k
    b4 = [k << 30 for k in range(1, 4)]
    rx, ry, rz, rw = word(eps, ()), word(eps, b4), word(peps, ()), word(peps, b25)
    cells = L * G * G
    controller = rs.randint(0, 256, 100 * cells if ckey == "cell" else 100).astype(np.uint8)
    planner = rs.randint(0, 256, cells).astype(np.uint8)
    kp, d, kc, goal, action = select_host(G, L, R.CKEYS.index(ckey), eps, peps, controller, planner, (lid, bx, by, fgx, fgy),
                                          (rx, ry, rz, rw))
    ball, fg = np.stack([bx, by], axis=1), np.stack([fgx, fgy], axis=1)
    want_kp = R.planner_keys(G, L, np.clip(lid, imin, imax), np.clip(ball, 0, G - 1))     # int64 in, as the rule clamps
    want_d, raw = R.offsets(fg, ball)
    want_kc = want_d + (want_kp.astype(np.int64) * 100 if ckey == "cell" else 0)
    assert (kp == want_kp).all() and kp.min() >= 0 and kp.max() < planner.size
    assert (d == want_d).all() and d.min() == 0 and d.max() == 99
    assert set(np.unique(d // 10)) == set(range(10)) == set(np.unique(d % 10))           # every offset of both axes
    assert ((raw < 0) | (raw > 9)).any() and not ((raw < 0) | (raw > 9)).all()
    assert (kc == want_kc).all() and kc.min() >= 0 and kc.max() < controller.size
    want_goal, p_explored = R.select(planner[want_kp], rz, rw, peps, 25)
    want_action, c_explored = R.select(controller[want_kc], rx, ry, eps, 4)
    assert (goal == want_goal).all() and (action == want_action).all()
    assert p_explored.any() == (peps != 0) and c_explored.any() == (eps != 0)
    assert peps >= (1 << 32) - 1 or not p_explored.all()
    assert eps >= (1 << 32) - 1 or not c_explored.all()
    if peps == (1 << 32) - 1:                                           # 1 - 2^-32: only rz = 2^32 - 1 stays greedy
        assert (p_explored == (rz < (1 << 32) - 1)).all() and set(np.unique(goal[p_explored])) == set(range(25))
        assert (goal[p_explored] == (rw[p_explored].astype(object) * 25 // (1 << 32)).astype(np.int64)).all()
    if eps == (1 << 32) - 1:
        assert (c_explored == (rx < (1 << 32) - 1)).all() and set(np.unique(action[c_explored])) == set(range(4))
        assert (action[c_explored] == (ry[c_explored] >> np.uint64(30)).astype(np.int64)).all()
    if eps == 0 and peps == 0:                                          # the ids pass through, out-of-range ones included
        assert (goal == planner[want_kp]).all() and (action == controller[want_kc]).all() and goal.max() > 24 and action.max() > 3


# ------------------------------------------------------------- the C ABI
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in NAMES:
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    env = importlib.import_module("gym-lmaze_amd").LmazeFovealVecEnv
    assert callable(env.rollout_hier_policy) and callable(env.controller_keys) and callable(env.state_keys)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("v5:104-292", "r.z < planner_epsilon_u32", "(r.w 25) >> 32", "r.y >> 30", "ep_hi ^ 0x80000000", "drawn once",
                   "nothing is drawn when both are 0", "clamp(fgoal_x - ball_x + 4, 0, 9)", "kp' 100 + d", "both are -1",
                   "at most 8192 bytes", "controller=lds|global planner=lds|global", "LMAZE_E_VARIANT anything but v5/v6",
                   "controller_key outside {0, 1}", "keep refusing v5/v6", "The caller advances its epoch by T."):
        assert phrase in flat, phrase


def test_header_compiles_as_c99_with_a_caller_of_the_new_entries(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include "lmaze.h"\n'
                   'int main(void){ LmazeFovealParams f = {0}; char text[8];\n'
                   '  int (*run)(const LmazeFovealParams*, const uint8_t*, const uint8_t*, int32_t, uint32_t, const uint8_t*, uint32_t,\n'
                   '             int32_t, const LmazeFovealBuffers*, int64_t, uint64_t, uint64_t, int64_t, float*, uint8_t*, float*,\n'
                   '             uint8_t*, int32_t*, int32_t*, int32_t*, int32_t*, float*, float*, int32_t, void*) = lmaze_v5_rollout_policy;\n'
                   '  int (*say)(const LmazeFovealParams*, int64_t, int32_t, int32_t, int32_t, char*, int32_t) = lmaze_describe_v5_rollout_policy;\n'
                   '  (void)f; (void)text; return run != 0 && say != 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "probe.o")])


def _params(abi, variant="v5", G=18, L=5, hint=0):
    return abi.LmazeFovealParams(VID.get(variant, variant), G, L, 10, 50, -1.0, -0.01, 100.0, hint)


BUFS = ("ball_xy", "goal_xy", "fgoal_xy", "layout_id", "step_count", "foveal_step_count", "reward", "foveal_reward", "done",
        "foveal_done", "visit", "obs", "ball1_xy", "fovea_xy", "last_xy", "foveal_goal", "obs_local", "visit_clock")


def _call(abi, variant="v5", G=18, L=5, hint=0, params=True, layouts=64, controller=64, ck=0, planner=64, T=6, bufs=True, n=100,
          obs_t=None, obs_local_t=None, every=0, **bkw):
    """fabricated device addresses: nothing is dereferenced before the refusals"""
    p = _params(abi, variant, G, L, hint)
    ptrs = {name: 4096 for name in BUFS}
    ptrs.update(bkw)
    b = abi.LmazeFovealBuffers(**ptrs)
    return abi.lib.lmaze_v5_rollout_policy(C.byref(p) if params else None, layouts, controller, ck, 123, planner, 456, T,
                                           C.byref(b) if bufs else None, n, 1, 0, 0, None, None, None, None, None, None, None, None,
                                           obs_t, obs_local_t, every, None)


@pytest.mark.parametrize("variant", ["v5", "v6"])
def test_refusals_in_their_documented_order(abi, variant):
    kw = dict(variant=variant)
    # 1. the recording request, before anything else -- even NULL params, another variant or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_local_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=4096, obs_local_t=4096 + 8, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, params=False, n=-1, **kw) == E_NULL
    assert _call(abi, every=-1, params=False, controller=None, T=-1, **kw) == E_COUNT
    assert _call(abi, variant="v2", obs_t=4096 + 8, every=1) == E_ALIGN
    # 2. the params' own, before the variant's refusal and the counts
    assert _call(abi, params=False, T=-1, **kw) == E_NULL
    assert _call(abi, variant=3, T=-1) == E_VARIANT
    assert _call(abi, variant=0, n=-1) == E_VARIANT
    assert _call(abi, G=4, T=-1, **kw) == E_GRID
    assert _call(abi, G=65, n=-1, **kw) == E_GRID
    assert _call(abi, variant="v2", G=4) == E_GRID                        # before 3.
    assert _call(abi, L=0, T=-1, **kw) == E_LAYOUT
    assert _call(abi, L=17, planner=None, **kw) == E_LAYOUT
    assert _call(abi, hint=0x400, T=-1, **kw) == E_LAYOUT
    # 3. anything but v5/v6, before the counts and before "nothing to do"
    for other in ("v1", "v2", "v4"):
        L = 1 if other == "v1" else 5
        assert _call(abi, variant=other, L=L) == E_VARIANT
        assert _call(abi, variant=other, L=L, T=-1, n=-1, ck=7) == E_VARIANT
        assert _call(abi, variant=other, L=L, T=0) == E_VARIANT
        assert _call(abi, variant=other, L=L, n=0, controller=None, planner=None, layouts=None, bufs=False) == E_VARIANT
    # 4. the counts, controller_key among them, before "nothing to do" and before the pointers
    assert _call(abi, T=-1, **kw) == E_COUNT
    assert _call(abi, n=-1, **kw) == E_COUNT
    assert _call(abi, n=MAX_ENVS + 1, **kw) == E_COUNT
    assert _call(abi, T=-1, n=0, **kw) == E_COUNT
    for ck in (-1, 2, 100):
        assert _call(abi, ck=ck, **kw) == E_COUNT
        assert _call(abi, ck=ck, T=0, **kw) == E_COUNT
        assert _call(abi, ck=ck, n=0, controller=None, planner=None, layouts=None, bufs=False, **kw) == E_COUNT
    # 5. nothing to do: 0 whatever the pointers, odd ones included
    for T, n in ((0, 100), (6, 0), (0, 0), (0, MAX_ENVS)):
        for ck in (0, 1):
            assert _call(abi, T=T, n=n, ck=ck, controller=None, planner=None, layouts=None, bufs=False, **kw) == 0
            assert _call(abi, T=T, n=n, ck=ck, controller=65, planner=67, obs=4096 + 4, **kw) == 0
            assert _call(abi, T=T, n=n, ck=ck, planner=None, obs_t=4096, every=4, **kw) == 0
    assert _call(abi, T=2, n=0, obs_t=None, every=3, **kw) == 0           # T / every == 0: no slot wanted, obs_t may be NULL
    # 6. the pointers, both tables among them; then alignment
    assert _call(abi, controller=None, **kw) == E_NULL
    assert _call(abi, planner=None, **kw) == E_NULL
    assert _call(abi, layouts=None, **kw) == E_NULL
    assert _call(abi, bufs=False, **kw) == E_NULL
    for name in BUFS:
        assert _call(abi, **dict(kw, **{name: None})) == E_NULL, name
    assert _call(abi, planner=None, obs=4096 + 4, **kw) == E_NULL         # NULL before alignment
    assert _call(abi, obs=4096 + 4, **kw) == E_ALIGN
    assert _call(abi, obs_local=4096 + 4, **kw) == E_ALIGN
    assert _call(abi, visit=4096 + 32, **kw) == E_ALIGN
    assert _call(abi, controller=65, planner=67, **kw) not in (E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN)   # tables: any address


def _foveal_lds(G, L, epb):
    """lmaze_foveal_defs.h foveal_lds for v5/v6: per-env strings and flags, row masks, layout characters, visit samples"""
    return epb * 64 + (3 * L * G + 2 * G) * 8 + ((L * G * G + 15) & ~15) + epb * (2 * 25 * 4 + 8)


@pytest.mark.parametrize("variant,G,L", [("v5", 18, 5), ("v6", 18, 5), ("v5", 12, 2), ("v5", 24, 16), ("v6", 24, 14), ("v5", 24, 15),
                                         ("v5", 5, 3), ("v5", 5, 4), ("v5", 9, 1), ("v5", 10, 1), ("v5", 64, 2), ("v5", 64, 3)])
def test_describe_names_the_kernel_and_where_the_tables_live(abi, variant, G, L):
    """Each table of at most 8192 bytes: staged in LDS behind the layout characters and counted in the launch's LDS; above:
    global, no extra LDS.  A rule, whatever n, T, the recording and the hint; any grid runs at any envs per workgroup."""
    cells = L * G * G
    for ckey in R.CKEYS:
        cbytes = 100 * cells if ckey == "cell" else 100
        sides = ("lds" if cbytes <= 8192 else "global", "lds" if cells <= 8192 else "global")
        staged = sum((b + 15) & ~15 for b, s in zip((cbytes, cells), sides) if s == "lds")
        for n, hint, epb in ((333, 0, 32), (333, 0x30, 64), (333, 0x40, 128), (333, 0x120, 32), (40000, 0, 64), (1 << 20, 0x20, 32)):
            for every in (0, 1, 5):
                line = abi.describe_v5_rollout_policy(_params(abi, variant, G, L, hint), n, 24, ckey, every)
                f = _fields(line)
                want = _foveal_lds(G, L, f["envs_per_workgroup"]) + staged
                if _foveal_lds(G, L, epb) + staged <= 64 << 10:          # the launcher assumes 64 KiB without a device
                    assert f["envs_per_workgroup"] == epb, line
                assert line.startswith("foveal_hier_policy_kernel<v5, %d, %d%s> controller=%s planner=%s T=24 grid="
                                       % (f["envs_per_workgroup"], G if G == 18 else 0, ", obs_t" if every else "", *sides)), line
                assert f["lds"] == want and f["block"] == 256, (line, want)
                chunks = ((hint >> 8) & 3) + 1
                assert f["chunks"] == chunks and f["grid"] == -(-(-(-n // f["envs_per_workgroup"])) // chunks), line
    # bits 0-3: the cap pads the LDS and is reported
    f = _fields(abi.describe_v5_rollout_policy(_params(abi, variant, G, L, 0x25), 333, 24, "offset", 0))
    assert f["workgroups_per_cu"] in (0, 5) and f["lds"] >= _foveal_lds(G, L, 32)


def test_the_shapes_of_the_gpu_test_sit_where_it_says(abi):
    for shape in R.SHAPES:
        L = shape.L or 5
        for ckey in R.CKEYS:
            line = abi.describe_v5_rollout_policy(_params(abi, shape.variant, shape.G, L), R.N, R.T, ckey, 0)
            assert " controller=%s planner=%s " % (R.controller_side(shape, L, ckey), shape.planner) in line, line


def test_describe_refusals_and_empty_lines(abi):
    d = abi.lib.lmaze_describe_v5_rollout_policy
    buf = C.create_string_buffer(256)
    p = _params(abi)
    assert d(C.byref(p), 100, 6, 0, 0, None, 256) == E_NULL
    assert d(C.byref(p), 100, 6, 0, 0, buf, 0) == E_NULL
    assert d(None, -1, -1, 5, -1, None, 256) == E_NULL                  # the text first
    assert d(C.byref(p), 100, 6, 0, -1, buf, 256) == E_COUNT
    assert d(None, 100, 6, 0, -1, buf, 256) == E_COUNT                  # the recording request before the params
    assert d(None, 100, 6, 0, 0, buf, 256) == E_NULL
    assert d(C.byref(_params(abi, 3)), 100, -1, 0, 0, buf, 256) == E_VARIANT
    assert d(C.byref(_params(abi, "v5", 4)), 100, -1, 0, 0, buf, 256) == E_GRID
    assert d(C.byref(_params(abi, "v5", 18, 17)), 100, -1, 0, 0, buf, 256) == E_LAYOUT
    for other, L in (("v1", 1), ("v2", 5), ("v4", 5)):
        assert d(C.byref(_params(abi, other, 18, L)), 100, 6, 0, 0, buf, 256) == E_VARIANT
        assert d(C.byref(_params(abi, other, 18, L)), 0, -1, 2, 3, buf, 256) == E_VARIANT
    assert d(C.byref(p), 100, -1, 0, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), -1, 6, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), MAX_ENVS + 1, 6, 0, 3, buf, 256) == E_COUNT
    for ck in (-1, 2):
        assert d(C.byref(p), 100, 6, ck, 0, buf, 256) == E_COUNT
        assert d(C.byref(p), 0, 6, ck, 0, buf, 256) == E_COUNT          # before "nothing to do"
    buf.value = b"stale"
    assert d(C.byref(p), 0, 6, 0, 0, buf, 256) == 0 and buf.value == b""
    buf.value = b"stale"
    assert d(C.byref(p), 100, 0, 1, 3, buf, 256) == 0 and buf.value == b""
    assert d(C.byref(p), 100, 6, 0, 0, buf, 8) == 0 and buf.value == b"foveal_"      # truncated to len, always terminated
    # the siblings keep refusing v5/v6
    for name in ("lmaze_describe_foveal_rollout_policy", "lmaze_describe_foveal_rollout_sample"):
        assert getattr(abi.lib, name)(C.byref(p), 100, 6, 1, 0, buf, 256) == E_VARIANT


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_no_scratch_and_within_one_wave_of_their_twin():
    """12 kernels (v5 x 32 / 64 / 128 envs x G = 18 / any x row or recording form), none with scratch; the open-loop twin sits
    at 4 waves per SIMD, the row forms hold 3 and the recording forms what DESIGN.md 4.5 states."""
    new = kernel_usage("lmaze_hier_policy.hip")
    pat = re.compile(r"_ZN5lmaze25foveal_hier_policy_kernelILi5ELi(32|64|128)ELi(18|0)ELb1EEEvNS_10FovealArgsENS_(14FovealRollHier|17FovealRollObsHier)E")
    assert len(new) == 12, sorted(new)
    seen = set()
    for name, v in new.items():
        m = pat.fullmatch(name)
        assert m, name
        rec = m.group(3).startswith("17")
        seen.add((m.group(1), m.group(2), rec))
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["Occupancy"] >= (REC_WAVES if rec else 3), (name, v)
    assert len(seen) == 12
    old = kernel_usage("lmaze_foveal.hip")
    twin = old["_ZN5lmaze21foveal_rollout_kernelILi5ELi32ELi18ELb1EEEvNS_10FovealArgsENS_10FovealRollE"]
    assert twin.get("ScratchSize", 0) == 0 and twin["Occupancy"] == 4
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "recording forms hold %d waves" % REC_WAVES in " ".join(design.split())


# ------------------------------------------------------------- the Python surface without a device
def test_python_argument_errors_that_need_no_device(abi, monkeypatch):
    """What rollout_hier_policy() and controller_keys() refuse before they touch the device, on an env object that never saw one."""
    pkg = importlib.import_module("gym-lmaze_amd")
    env = object.__new__(pkg.LmazeFovealVecEnv)
    env.variant, env._two_level, env.num_envs, env.grid, env.n_layouts = "v5", True, 8, 18, 5
    with monkeypatch.context() as m:                                    # under stream capture, before the tables are looked at
        m.setattr(importlib.import_module("torch").cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="stream capture"):
            env.rollout_hier_policy(4, controller=object(), planner=object())
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_hier_policy(T, controller=object(), planner=object())
    for kw in (dict(), dict(controller=object()), dict(planner=object()), dict(controller=object(), controller_q=object(), planner=object()),
               dict(controller=object(), planner=object(), planner_q=object())):
        with pytest.raises(ValueError, match="exactly one of"):
            env.rollout_hier_policy(4, **kw)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            env.rollout_hier_policy(4, controller=object(), planner=object(), epsilon=bad)
        with pytest.raises(ValueError):
            env.rollout_hier_policy(4, controller=object(), planner=object(), planner_epsilon=bad)
    for bad in ("goal", 2, -1):
        with pytest.raises(ValueError, match="controller_key"):
            env.rollout_hier_policy(4, controller=object(), planner=object(), controller_key=bad)
        with pytest.raises(ValueError, match="controller_key"):
            env.controller_keys(bad)
    for variant in ("v1", "v2", "v4"):
        env.variant, env._two_level = variant, False
        with pytest.raises(ValueError, match="v5/v6"):
            env.rollout_hier_policy(4, controller=object(), planner=object())
        with pytest.raises(ValueError, match="v5/v6"):
            env.controller_keys()
    env.variant, env._two_level = "v5", True
    with pytest.raises(ValueError, match="v5/v6"):                       # rollout_policy() stays as it is
        env.rollout_policy(4, policy=object())
