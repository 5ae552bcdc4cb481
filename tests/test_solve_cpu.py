"""CPU: lmaze_solve / lmaze_describe_solve without a GPU -- the reference itself (solve_ref.py: the model extracted from the
C oracle, the float32 Jacobi sweep, a BFS) on the shipped layouts, every documented refusal in its order of precedence
(answered before any device call), the launch the describe call names for every grid size, and what the kernels need."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import solve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
MAX_ENVS = 1 << 30
LDS_PER_CU = 160 << 10


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def _shipped(name):
    L = importlib.import_module("gym-lmaze_amd.layouts")
    lay = L.to_codes(getattr(L, name))
    gx, gy = np.argwhere(lay == ord("X"))[0]
    return lay, np.array([gx, gy], np.int32)


SHIPPED = [("v0", "V0_GRID_12", 72, 2, 18), ("v3", "V3_GRID_18", 73, 0, 14)]


# ------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("variant,name,cells,sticky,sweeps", SHIPPED)
def test_reference_on_the_shipped_layouts(abi, variant, name, cells, sticky, sweeps):
    """No non-wall cell of the shipped layouts (v3: the goal at 'X') is cut off from a terminal pair -- the closed-loop GPU
    test puts an env on every one of them and relies on it -- and the greedy policy of the converged solve lowers
    steps_to_done by exactly one from every reachable cell.  The counts and the sweep at which the bits settle are the
    figures of a hand-written prototype of the same specification."""
    lay, goal = _shipped(name)
    m = R.extract_model(variant, lay, goal if variant == "v3" else None)
    assert int((~m.wall).sum()) == cells and int(m.sticky.sum()) == sticky
    dist = R.steps_to_done(m)
    assert int((np.isinf(dist) & ~m.wall).sum()) == 0
    assert np.isinf(dist[m.wall]).all()
    s = R.solve(m, 0.99, 4096)
    assert int(s.sweeps_run) == sweeps and float(s.delta) == 0.0
    assert R.greedy_lowers_distance(m, s.policy, dist).all()
    assert (R.bits(s.v) == R.bits(s.q.max(1))).all()
    # cut off at 5 sweeps: the 5th still moves values
    cut = R.solve(m, 0.99, 5)
    assert int(cut.sweeps_run) == 5 and float(cut.delta) > 0.0


def test_reference_model_carries_the_rules_quirks():
    """v0 refuses the 'S' cell and repeats the incoming reward (sticky); v3 pays the goal when the cell BEYOND the target is
    the goal; a bump keeps the ball and pays reward_wall; terminal is r == reward_goal."""
    G = 6
    codes = np.frombuffer("".join(("WWWWWW", "WBSBXW", "WBBBBW", "WBBBBW", "WBBBBW", "WWWWWW")).encode(), np.uint8).reshape(G, G)
    m = R.extract_model("v0", codes)
    s = 1 * G + 1
    assert m.sticky[s].tolist() == [False, False, False, True]           # right of (1,1) is 'S'
    assert m.nxt[s].tolist() == [s, s + G, s, s] and m.r[s, 0] == np.float32(-1.0) and m.r[s, 1] == np.float32(-0.01)
    s = 1 * G + 3
    assert m.terminal[s].tolist() == [False, False, False, True] and m.nxt[s, 3] == s + 1 and m.r[s, 3] == np.float32(100.0)
    assert m.sticky[s, 2]                                                  # left of (1,3) is 'S'
    m3 = R.extract_model("v3", codes, (1, 4))
    s = 1 * G + 2                                                          # v3 walks over 'S'; from (1,2) right lands on (1,3), beyond is the goal
    assert not m3.sticky.any() and m3.terminal[s].tolist() == [False, False, False, True] and m3.nxt[s, 3] == s + 1
    assert not m3.terminal[1 * G + 3].any() and m3.nxt[1 * G + 3, 3] == 1 * G + 4     # stepping ONTO the goal pays reward_move
    bump = R.extract_model("v0", codes, rewards=(100.0, -0.01, 100.0))   # reward_wall == reward_goal: a bump is terminal
    assert bump.terminal[1 * G + 1, 0] and bump.nxt[1 * G + 1, 0] == 1 * G + 1


def test_batched_reference_is_the_plain_one():
    lays = H.bordered_random_layouts(9, 8, 7)
    for variant, goals in (("v0", None), ("v3", H.random_free_cells(lays, 3))):
        vi = np.random.RandomState(2).randn(9, 64).astype(np.float32)
        for gamma, sweeps, v_init in ((0.99, 1400, None), (1.0, 40, vi), (0.0, 9, None)):
            many = R.solve_many(variant, lays, goals, gamma, sweeps, v_init=v_init)
            for p, m in enumerate(R.models_of(variant, lays, goals)):
                one = R.solve(m, gamma, sweeps, None if v_init is None else v_init[p])
                for f in R.Solved._fields:
                    a, b = np.asarray(getattr(many, f))[p], np.asarray(getattr(one, f))
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (variant, gamma, p, f)


def test_goals_off_the_grid_and_on_corners_are_never_hit():
    """The goals test_gpu_solve.py hands to lmaze_solve, through extract_model: a v3 goal off the grid or on a corner of the
    border gives no terminal pair, so every non-wall state has steps_to_done == inf; a goal on another wall cell is paid for
    by the look-ahead (v3:264) wherever the ball can stand two cells away in line with it."""
    lays = H.bordered_random_layouts(257, 8, 7)
    goals, off = R.unreachable_goals(lays, H.random_free_cells(lays, 3))
    goals, walled = R.walled_goals(lays, goals, 5)
    assert len(off) == 65 and len(walled) == 64 and not set(off) & set(walled)
    assert ((goals[off] < 0) | (goals[off] > 7)).any(1).sum() >= 39            # the rest: the four corners
    for p in off:
        m = R.extract_model("v3", lays[p], goals[p])
        assert not m.terminal.any() and not m.sticky.any(), (p, goals[p])
        assert np.isinf(R.steps_to_done(m)).all()
        assert (m.r[~m.wall] != np.float32(100.0)).all()
    paid = 0
    for p in walled:
        assert lays[p][tuple(goals[p])] == ord("W")
        m = R.extract_model("v3", lays[p], goals[p])
        paid += int(m.terminal.any())
        s, a = np.nonzero(m.terminal)
        assert (m.nxt[s, a] != s).all()                                        # a terminal pair moved: the goal lay beyond
    assert paid > 20


# ------------------------------------------------------------- refusals
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_solve", "lmaze_describe_solve"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    pkg = importlib.import_module("gym-lmaze_amd")
    assert callable(pkg.solve_tables) and "solve_tables" in pkg.__all__ and callable(pkg.LmazeVecEnv.solve)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("infinite-horizon discounted problem", "step limit is not part of the model", "STICKY pair", "-INFINITY",
                   "never a fused multiply-add", "strict '>'", "that sweep counts", "v0:172-195", "v0:246-249", "v3:224-265",
                   "v3:398", "does not depend on the order of the reduction"):
        assert phrase in flat, phrase


def test_solve_refusals_in_order(abi):
    f = abi.lib.lmaze_solve

    def P(variant=abi.VARIANT_V0, grid=12, mode=abi.LAYOUT_SHARED):
        return abi.make_params(variant, grid, mode, 100, -1.0, -0.01, 100.0)

    def call(p=None, lay=64, goal=64, problems=3, gamma=0.99, sweeps=10, v_init=None, q=64, v=64, pol=64, run=64, delta=64):
        p = P() if p is None else p
        return f(C.byref(p) if p != "null" else None, lay, goal, problems, gamma, sweeps, v_init, q, v, pol, run, delta, None)
    v3 = P(abi.VARIANT_V3, 18)
    # 1. params or layouts
    assert call(p="null") == E_NULL and call(lay=None) == E_NULL
    assert call(lay=None, p=P(grid=2)) == E_NULL
    # 2. the grid
    for g in (2, 65, -1):
        assert call(p=P(grid=g)) == E_GRID
        assert call(p=P(variant=1, grid=g, mode=7), goal=None, q=None, v=None, pol=None, problems=-1) == E_GRID
    assert call(p=P(grid=3), problems=0) == 0 and call(p=P(grid=64), problems=0) == 0
    # 3. the variant
    for var in (1, 2, 4, 5, 6, -1):
        assert call(p=P(variant=var, mode=7), q=None, v=None, pol=None, problems=-1) == E_VARIANT
    # 4. the layout mode
    assert call(p=P(mode=2)) == E_LAYOUT
    assert call(p=P(abi.VARIANT_V3, 18, 2), goal=None, q=None, v=None, pol=None, sweeps=0) == E_LAYOUT
    # 5. v3's goals
    assert call(p=v3, goal=None) == E_NULL
    assert call(p=v3, goal=None, q=None, v=None, pol=None, problems=-1, sweeps=0) == E_NULL
    assert call(goal=None, problems=0) == 0                         # v0 does not read them
    # 6. no table asked for
    assert call(q=None, v=None, pol=None) == E_NULL
    assert call(q=None, v=None, pol=None, problems=-1, sweeps=0) == E_NULL
    # 7. the counts
    assert call(problems=-1) == E_COUNT and call(problems=MAX_ENVS + 1) == E_COUNT
    assert call(sweeps=0) == E_COUNT and call(sweeps=-5) == E_COUNT
    assert call(sweeps=0, problems=0) == E_COUNT and call(problems=-1, q=8) == E_COUNT     # before the alignment
    # 8. alignment
    for kw in (dict(q=72), dict(q=8), dict(v=66), dict(v_init=65), dict(run=70), dict(delta=67)):
        assert call(**kw) == E_ALIGN, kw
        assert call(problems=0, **kw) == E_ALIGN, kw                # before "nothing to do"
    assert call(p=v3, goal=68) == E_ALIGN
    assert call(goal=68, problems=0) == 0                           # v0: not read, not judged
    assert call(pol=65, problems=0) == 0                            # bytes
    # 9. nothing to do: nothing is read, whatever the addresses; each output alone will do
    for kw in (dict(), dict(q=None, v=None), dict(q=None, pol=None), dict(v=None, pol=None), dict(run=None, delta=None),
               dict(p=v3), dict(p=P(mode=abi.LAYOUT_PER_ENV)), dict(gamma=float("nan")), dict(gamma=-3.0)):
        assert call(problems=0, **kw) == 0, kw
    # a grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration (9), from grid_ok, before any launch
    assert call(p=P(grid=17), problems=1 << 24) == 9
    assert call(p=P(grid=16), problems=1 << 26) == 9


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


def test_describe_solve_every_grid(abi):
    """Every G, both layout modes, both variants: the LDS fits a CU, the grid covers the problems exactly, a wave per problem
    while G*G <= 256 and a workgroup per problem above; the LDS holds two V buffers of the cells a problem's threads cover."""
    forms = set()
    for G in range(3, 65):
        for mode in (abi.LAYOUT_SHARED, abi.LAYOUT_PER_ENV):
            for variant, tag in ((abi.VARIANT_V0, "v0"), (abi.VARIANT_V3, "v3")):
                p = abi.make_params(variant, G, mode, 100, -1.0, -0.01, 100.0)
                for problems in (1, 2, 257, 65536):
                    line = abi.describe_solve(p, problems)
                    m = re.match(r"solve_kernel<(v0|v3), (wave|workgroup), (\d+)> grid=", line)
                    assert m and m.group(1) == tag, line
                    f = _fields(line)
                    ppw, cpl = f["problems_per_workgroup"], int(m.group(3))
                    assert f["block"] == 256 and 0 < f["lds"] <= LDS_PER_CU, line
                    assert f["grid"] * ppw >= problems > (f["grid"] - 1) * ppw, line
                    wave = G * G <= 256
                    assert m.group(2) == ("wave" if wave else "workgroup") and ppw == (4 if wave else 1), line
                    threads = 256 // ppw
                    assert cpl * threads >= G * G and (cpl == 1 or (cpl // 2) * threads < G * G), line     # the smallest form that covers it
                    assert 2 * 4 * cpl * threads * ppw <= f["lds"] <= 2 * 4 * cpl * threads * ppw + 512, line
                    assert f["lds"] <= 40 << 10, line                  # at least four workgroups per CU at any G
                    forms.add((m.group(2), cpl))
    assert forms == {("wave", 1), ("wave", 2), ("wave", 4), ("workgroup", 2), ("workgroup", 4), ("workgroup", 8), ("workgroup", 16)}


def test_describe_solve_refusals(abi):
    d = abi.lib.lmaze_describe_solve
    buf = C.create_string_buffer(256)

    def P(variant=abi.VARIANT_V0, grid=12, mode=abi.LAYOUT_SHARED):
        return abi.make_params(variant, grid, mode, 100, -1.0, -0.01, 100.0)
    assert d(None, 1, buf, 256) == E_NULL and d(C.byref(P()), 1, None, 256) == E_NULL and d(C.byref(P()), 1, buf, 0) == E_NULL
    assert d(C.byref(P(grid=2)), 1, buf, 256) == E_GRID
    assert d(C.byref(P(variant=2)), 1, buf, 256) == E_VARIANT
    assert d(C.byref(P(mode=3)), 1, buf, 256) == E_LAYOUT
    assert d(C.byref(P()), -1, buf, 256) == E_COUNT and d(C.byref(P()), MAX_ENVS + 1, buf, 256) == E_COUNT
    buf.value = b"stale"
    assert d(C.byref(P()), 0, buf, 256) == 0 and buf.value == b""
    assert d(C.byref(P()), 5, buf, 8) == 0 and buf.value == b"solve_k"       # truncated to len, always terminated


# ------------------------------------------------------------- what the kernels need
@pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not installed")
def test_solve_kernels_use_no_scratch():
    usage = H.kernel_usage("lmaze_solve.hip")
    mine = {k: v for k, v in usage.items() if "solve_kernel" in k}
    assert len(mine) == 14, sorted(usage)                           # 2 variants x (3 wave forms + 4 workgroup forms)
    for name, v in mine.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["VGPRs"] <= 256, (name, v)                         # two waves per SIMD at the least: 4 workgroups per CU
        wave = "Lb1E" in name                                       # and no form above what it had before the shared frame
        cpl = int(re.search(r"ILi\dELi(\d+)E", name).group(1))
        assert v["VGPRs"] <= ({1: 30, 2: 33, 4: 49} if wave else {2: 27, 4: 46, 8: 98, 16: 159})[cpl], (name, v)
