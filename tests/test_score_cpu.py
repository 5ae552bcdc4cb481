"""CPU: lmaze_score / lmaze_describe_score without a GPU -- the reference against itself (score_ref.py: the plain walk against
the emulation of the kernel's doubling rounds and sweeps, against solve_ref's BFS and against qlearn_ref.greedy_share's
counts), every documented refusal in its order of precedence (answered before any device call), the launch the describe call
names at every plan step, and what the kernels need."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import maze_ref as M
import qlearn_ref as Q
import score_ref as SC
import solve_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
MAX_ENVS = 1 << 30
PLAN_STEPS = (3, 5, 8, 9, 11, 12, 16, 17, 23, 32, 33, 46, 64)


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


# ------------------------------------------------------------- the reference itself
def plain_walk(model, act, s):
    """One start state, one step at a time: the definition"""
    seen = set()
    t = 0
    while True:
        if model.wall[s] or not 0 <= act[s] <= 3 or s in seen:
            return -1
        seen.add(s)
        a = act[s]
        if model.sticky[s, a]:
            return -1
        t += 1
        if model.terminal[s, a]:
            return t
        s = int(model.nxt[s, a])


@pytest.mark.parametrize("G", [5, 8, 11, 12, 16, 17, 33])
def test_walk_is_the_doubling_and_the_sweeps_are_the_bfs(G):
    """Generated mazes, solve_ref's policy, random bytes (some above 3) and random q rows: the vectorised walk is the plain
    one, the doubling emulation gives the same lengths within ceil(log2 S) rounds, the sweeps give the BFS's distances within S."""
    S = G * G
    lays, _ = M.generate(G, 3, 11, 0, 1 << 30)
    lays[2, 1, 1] = ord("S")                                               # v0's excluded pairs
    rs = np.random.RandomState(G)
    worst_rounds = worst_sweeps = 0
    for p in range(3):
        m = SR.extract_model("v0", lays[p])
        opt, k = SC.sweeps(m)
        assert (opt == SC.optimal(m)).all() and 1 <= k <= S
        worst_sweeps = max(worst_sweeps, k)
        solved = SR.solve(m, 0.99, 4096).policy
        rand = rs.randint(0, 4, S).astype(np.uint8)
        wild = rand.copy()
        wild[rs.rand(S) < 0.1] = 200
        q = rs.choice(np.array([-1.0, 0.0, 0.0, 2.0, np.nan, np.inf], np.float32), (S, 4))
        for act in (SC.actions_of(policy=solved), SC.actions_of(policy=rand), SC.actions_of(policy=wild), SC.actions_of(q=q)):
            steps = SC.walk(m, act)
            assert steps.tolist() == [plain_walk(m, act, s) for s in range(S)]
            dbl, rounds = SC.doubling(m, act)
            assert (dbl == steps).all() and rounds <= SC.log2_ceil(S)
            worst_rounds = max(worst_rounds, rounds)
            assert steps.max() < S and ((steps == -1) | (steps >= np.where(opt < 0, S, opt))).all()
        best = SC.score(m, policy=solved)
        free = int((~m.wall).sum())
        if p < 2:                                                          # no 'S': the planner's walk is a shortest one everywhere
            assert best.summary.tolist() == [free, free, free, 0], (G, p)
    print("G", G, "rounds", worst_rounds, "of", SC.log2_ceil(S), "sweeps", worst_sweeps)
    if G >= 11:
        assert worst_rounds == SC.log2_ceil(S)                             # a cycle keeps its pointers live: every round runs


@pytest.mark.parametrize("G", [17, 64])
def test_serpentine_is_deep(G):
    """One corridor through every free cell: the longest distance exceeds S / 4, the corridor's policy arrives from every
    cell in exactly the fewest steps, and one reversed cell cuts everything before it off."""
    S = G * G
    lay, path = SC.serpentine(G)
    m = SR.extract_model("v0", lay)
    opt = SC.optimal(m)
    assert opt.max() > S // 4 and opt.max() == len(path) - 1
    pol = SC.corridor_policy(G, path)
    got = SC.score(m, policy=pol)
    on_path = len(path) - 1                                                # the goal cell itself walks off it
    assert got.summary[0] == len(path) and got.summary[2] >= on_path and got.steps.max() == opt.max()
    assert (SC.doubling(m, SC.actions_of(policy=pol))[0] == got.steps).all()
    assert SC.sweeps(m)[1] == opt.max() + 1 or SC.sweeps(m)[1] == opt.max()
    cut = pol.copy()
    x, y = path[len(path) // 2]
    cut[x * G + y] ^= 1                                                    # up <-> down, left <-> right
    worse = SC.score(m, policy=cut)
    assert worse.summary[1] < got.summary[1] - len(path) // 2 + 2


def test_counts_are_greedy_shares():
    """The learner's table of qlearn_ref.learn_case(): the sums of shortest and reachable are the good and total that
    greedy_share counts by walking start by start"""
    case = Q.learn_case()
    got = SC.score_many("v0", case["lay"], q=case["q"])
    print("shortest", got.summary[:, 2].sum(), "reachable", got.summary[:, 0].sum(), "arrived", got.summary[:, 1].sum())
    assert (int(got.summary[:, 2].sum()), int(got.summary[:, 0].sum())) == (case["good"], case["total"])


# ------------------------------------------------------------- refusals
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_score", "lmaze_describe_score"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    lm = importlib.import_module("gym-lmaze_amd")
    assert callable(lm.score_tables) and callable(lm.LmazeVecEnv.score) and callable(abi.describe_score)
    assert lm.ScoredTables._fields == ("optimal", "steps", "summary")


def test_score_refusals_in_order(abi):
    f = abi.lib.lmaze_score

    def P(variant=abi.VARIANT_V0, grid=12, mode=abi.LAYOUT_SHARED):
        return abi.make_params(variant, grid, mode, 100, -1.0, -0.01, 100.0)

    def call(p=None, lay=64, goal=64, problems=3, pol=64, q=None, opt=64, steps=64, summ=64):
        p = P() if p is None else p
        return f(C.byref(p) if p != "null" else None, lay, goal, problems, pol, q, opt, steps, summ, None)
    v3 = P(abi.VARIANT_V3, 18)
    none = dict(opt=None, steps=None, summ=None)
    # 1. params or layouts
    assert call(p="null") == E_NULL and call(lay=None) == E_NULL
    assert call(lay=None, p=P(grid=2)) == E_NULL
    # 2. the grid
    for g in (2, 65, -1):
        assert call(p=P(grid=g)) == E_GRID
        assert call(p=P(variant=1, grid=g, mode=7), goal=None, problems=-1, **none) == E_GRID
    # 3. the variant
    for var in (1, 2, 4, 5, 6, -1):
        assert call(p=P(variant=var, mode=7), problems=-1, **none) == E_VARIANT
    # 4. the layout mode
    assert call(p=P(mode=2)) == E_LAYOUT
    assert call(p=P(abi.VARIANT_V3, 18, 2), goal=None, **none) == E_LAYOUT
    # 5. v3's goals
    assert call(p=v3, goal=None) == E_NULL
    assert call(p=v3, goal=None, problems=-1, q=8, **none) == E_NULL
    assert call(goal=None, problems=0) == 0                         # v0 does not read them
    # 6. no output asked for
    assert call(**none) == E_NULL and call(problems=-1, **none) == E_NULL
    # 7. both tables
    assert call(q=64) == E_NULL and call(q=64, problems=-1) == E_NULL and call(q=8, pol=65, problems=0) == E_NULL
    # 8. steps without a table
    assert call(pol=None) == E_NULL and call(pol=None, problems=-1, opt=66) == E_NULL
    assert call(pol=None, steps=None, problems=0) == 0              # distances only
    # 9. the count
    assert call(problems=-1) == E_COUNT and call(problems=MAX_ENVS + 1) == E_COUNT
    assert call(problems=-1, pol=None, q=8, opt=66) == E_COUNT      # before the alignment
    # 10. alignment
    for kw in (dict(pol=None, q=72), dict(pol=None, q=8), dict(pol=66), dict(pol=65), dict(opt=66), dict(steps=65), dict(summ=70)):
        assert call(**kw) == E_ALIGN, kw
        assert call(problems=0, **kw) == E_ALIGN, kw                # before "nothing to do"
    assert call(p=v3, goal=68) == E_ALIGN
    assert call(goal=68, problems=0) == 0                           # v0: not read, not judged
    # 11. nothing to do: nothing is read, whatever the addresses; each output alone will do
    for kw in (dict(), dict(opt=None, steps=None), dict(opt=None, summ=None), dict(steps=None, summ=None), dict(pol=None, q=64),
               dict(pol=None, steps=None), dict(p=v3), dict(p=P(mode=abi.LAYOUT_PER_ENV))):
        assert call(problems=0, **kw) == 0, kw
    # a grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration (9), from grid_ok, before any launch
    assert call(p=P(grid=17), problems=1 << 24) == 9
    assert call(p=P(grid=16), problems=1 << 26) == 9


def test_describe_score_refusals(abi):
    d = abi.lib.lmaze_describe_score
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
    assert abi.describe_score(P(), 0) == ""
    assert d(C.byref(P()), 5, buf, 8) == 0 and buf.value == b"score_k"     # truncated to len, always terminated
    with pytest.raises(abi.LmazeError):
        abi.describe_score(P(grid=2), 1)


# ------------------------------------------------------------- what a describe line must say
def test_describe_score_every_plan_step(abi):
    """The plan is lmaze_solve's: the same form, cells per lane, grid and LDS at every size, both variants, both layout modes"""
    want = {3: ("wave", 1), 5: ("wave", 1), 8: ("wave", 1), 9: ("wave", 2), 11: ("wave", 2), 12: ("wave", 4), 16: ("wave", 4),
            17: ("workgroup", 2), 23: ("workgroup", 4), 32: ("workgroup", 4), 33: ("workgroup", 8), 46: ("workgroup", 16),
            64: ("workgroup", 16)}
    assert tuple(sorted(want)) == PLAN_STEPS
    for G in range(3, 65):
        for mode in (abi.LAYOUT_SHARED, abi.LAYOUT_PER_ENV):
            for variant, tag in ((abi.VARIANT_V0, "v0"), (abi.VARIANT_V3, "v3")):
                p = abi.make_params(variant, G, mode, 100, -1.0, -0.01, 100.0)
                for problems in (1, 4, 5, 7, 259, 65536):
                    line = abi.describe_score(p, problems)
                    assert line == abi.describe_solve(p, problems).replace("solve_kernel", "score_kernel"), line
                    m = re.match(r"score_kernel<(v0|v3), (wave|workgroup), (\d+)> grid=(\d+) block=256 lds=(\d+) problems_per_workgroup=(\d+)$", line)
                    assert m and m.group(1) == tag, line
                    form, cpl, grid, lds, ppw = m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))
                    assert (form == "wave") == (G * G <= 256) and ppw == (4 if form == "wave" else 1), line
                    assert grid == -(-problems // ppw) and cpl * (256 // ppw) >= G * G, line
                    assert 2 * 4 * cpl * 256 <= lds <= 2 * 4 * cpl * 256 + 512 and lds <= 40 << 10, line
                    if G in want:
                        assert (form, cpl) == want[G], line


# ------------------------------------------------------------- what the kernels need
@pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not installed")
def test_score_kernels_use_no_scratch():
    """Fourteen kernels (two variants; three wave forms, four workgroup forms), none with scratch; the registers DESIGN 4.1c
    states: at most 40 in the wave forms (eight waves per SIMD), at most 112 in the largest workgroup form (four)."""
    usage = H.kernel_usage("lmaze_score.hip")
    mine = {k: v for k, v in usage.items() if "score_kernel" in k}
    assert len(mine) == 14, sorted(usage)
    for name, v in mine.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        wave = "Lb1E" in name
        cpl = int(re.search(r"ILi\dELi(\d+)E", name).group(1))
        assert v["VGPRs"] <= (40 if wave else {2: 32, 4: 40, 8: 80, 16: 112}[cpl]), (name, v)
        # and no form above what it had before the shared frame
        assert v["VGPRs"] <= ({1: 29, 2: 35, 4: 39} if wave else {2: 26, 4: 33, 8: 75, 16: 111})[cpl], (name, v)
        assert v["Occupancy"] >= (8 if wave or cpl == 2 else {4: 7, 8: 6, 16: 4}[cpl]), (name, v)
