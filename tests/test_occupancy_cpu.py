"""CPU: lmaze_occupancy / lmaze_describe_occupancy without a GPU -- every documented refusal in its order of precedence
(answered before any device call), the Python refusals that need no device, reset_distribution() against the oracle's reset,
the reference against itself (occupancy_ref.py: the stacked sweep against the per-problem one, the float32 fixed point against
a float64 linear solve in the L1 norm, the duality <start, V> = <d_sa, r> with evaluate_ref, the monotone claim of the header),
and what the kernels need."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import evaluate_ref as E
import helpers as H
import occupancy_ref as OR
import oracle_lib as O
import solve_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
MAX_ENVS = 1 << 30
EPSILONS = (0, 1 << 28, 1 << 31, (1 << 32) - 1)
U = 2.0 ** -24
# The roundings between an exact contribution gamma * p_a(s) * d(s) to d(c) and the float32 one, at most.  An incoming term:
# three behind p (two conversions, one division), the product with D, four sums of the accumulator (of five terms at most; the
# first sum, 0 + term, is exact), the product with gamma, the sum with start: 3 + 1 + 4 + 1 + 1 = 10.  The term that stays:
# three behind each p and three sums behind wself, the product with D, its one sum (it is added last), gamma, start:
# 3 + 3 + 1 + 1 + 1 + 1 = 10.  start itself takes one, the last sum.  u + rel(10) <= rel(11): eleven per cell and sweep.
ROUNDINGS = 11
# ... and between V and the float32 V: test_evaluate_cpu.py's test_float32_fixed_point_is_the_linear_solve
V_ROUNDINGS = 8


def rel(n):
    """gamma_n of the standard error analysis: n roundings compound to at most n u / (1 - n u)"""
    return n * U / (1 - n * U)


def d_bound(gamma, d_norm):
    """|| d32 - d ||_1 on a settled problem.  Everything is non-negative, so the float32 fixed point satisfies
    d32 = (1 + e0) start + gamma (P + dP)^T d32 exactly, |e0| <= u and |dP| <= rel(ROUNDINGS - 1) P entry by entry; then
    d32 - d = (I - gamma P^T)^-1 (e0 start + gamma dP^T d32), and in the L1 norm || P^T ||_1 <= 1 (a row of P sums to at most
    1: gamma P^T contracts in L1, not in the max norm), || (I - gamma P^T)^-1 ||_1 <= 1 / (1 - gamma), || start ||_1 <= || d ||_1:
    || d32 - d ||_1 <= (u + rel(ROUNDINGS - 1)) max(|| d ||_1, || d32 ||_1) / (1 - gamma) <= rel(ROUNDINGS) max(...) / (1 - gamma).
    d_norm is that maximum."""
    return rel(ROUNDINGS) * d_norm / (1 - gamma)


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


@pytest.fixture(scope="module")
def lm(abi):
    return importlib.import_module("gym-lmaze_amd")


@pytest.fixture(scope="module")
def mazes():
    """test_evaluate_cpu.py's: six random 11 x 11 mazes with an 'S' each, their v0 models, and what solve_ref plans"""
    lays = H.bordered_random_layouts(6, 11, 7)
    models = SR.models_of("v0", lays, None)
    solved = {g: [SR.solve(m, g, 8192) for m in models] for g in (0.9, 0.99)}
    return lays, models, solved


def random_thresholds(rs, shape, wild=0.2):
    c = rs.randint(0, 1 << 32, size=shape + (4,), dtype=np.uint64).astype(np.uint32)
    ordered = np.sort(c[..., :3], axis=-1)
    keep = rs.rand(*shape) < wild
    c[..., :3] = np.where(keep[..., None], c[..., :3], ordered)
    return c


def uniform_start(model):
    """float32[S]: uniform over the cells that are not 'W'"""
    free = ~model.wall
    return (free / free.sum()).astype(np.float32)


# ------------------------------------------------------------- refusals
def test_symbols_exported_and_declared(abi, lm):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_occupancy", "lmaze_describe_occupancy"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    assert callable(lm.occupancy_tables) and callable(lm.reset_distribution) and callable(lm.LmazeVecEnv.occupancy)
    assert callable(abi.describe_occupancy)
    assert lm.OccupancyTables._fields == ("d", "d_sa", "sweeps_run", "delta")
    for name in ("occupancy_tables", "OccupancyTables", "reset_distribution"):
        assert name in lm.__all__


def test_occupancy_refusals_in_order(abi):
    f = abi.lib.lmaze_occupancy

    def P(variant=abi.VARIANT_V0, grid=12, mode=abi.LAYOUT_SHARED):
        return abi.make_params(variant, grid, mode, 100, -1.0, -0.01, 100.0)

    def call(p=None, lay=64, goal=64, problems=3, pol=64, q=None, eps=0, thr=None, start=64, sweeps=10, tol=0.0, d_init=None, do=64,
             dsa=64, run=64, delta=64):
        p = P() if p is None else p
        return f(C.byref(p) if p != "null" else None, lay, goal, problems, pol, q, eps, thr, start, 0.99, sweeps, tol, d_init, do, dsa,
                 run, delta, None)
    v3 = P(abi.VARIANT_V3, 18)
    none = dict(do=None, dsa=None)
    # 1. params or layouts
    assert call(p="null") == E_NULL and call(lay=None) == E_NULL
    assert call(lay=None, p=P(grid=2)) == E_NULL
    # 2. the grid
    for g in (2, 65, -1):
        assert call(p=P(grid=g)) == E_GRID
        assert call(p=P(variant=1, grid=g, mode=7), goal=None, problems=-1, start=None, **none) == E_GRID
    # 3. the variant
    for var in (1, 2, 4, 5, 6, -1):
        assert call(p=P(variant=var, mode=7), problems=-1, start=None, **none) == E_VARIANT
    # 4. the layout mode
    assert call(p=P(mode=2)) == E_LAYOUT
    assert call(p=P(abi.VARIANT_V3, 18, 2), goal=None, start=None, **none) == E_LAYOUT
    # 5. v3's goals
    assert call(p=v3, goal=None) == E_NULL
    assert call(p=v3, goal=None, problems=-1, q=8, **none) == E_NULL
    assert call(goal=None, problems=0) == 0                         # v0 does not read them
    # 6. neither d_out nor dsa_out
    assert call(**none) == E_NULL and call(problems=-1, pol=None, start=None, **none) == E_NULL
    assert call(do=None, problems=0) == 0 and call(dsa=None, problems=0) == 0 and call(run=None, delta=None, problems=0) == 0
    # 7. exactly one policy input
    assert call(pol=None) == E_NULL and call(pol=None, problems=-1, sweeps=0, start=None) == E_NULL
    for kw in (dict(q=64), dict(thr=64), dict(q=64, thr=64), dict(pol=None, q=64, thr=64)):
        assert call(**kw) == E_NULL and call(problems=-1, **kw) == E_NULL and call(problems=0, dsa=8, **kw) == E_NULL, kw
    # 8. start: with the other NULL checks, before the counts and the alignment, also with nothing to do
    assert call(start=None) == E_NULL and call(start=None, problems=-1) == E_NULL and call(start=None, sweeps=0) == E_NULL
    assert call(start=None, dsa=8) == E_NULL and call(start=None, problems=0) == E_NULL
    # 9. the counts
    assert call(problems=-1) == E_COUNT and call(problems=MAX_ENVS + 1) == E_COUNT
    assert call(sweeps=0) == E_COUNT and call(sweeps=-5, problems=0) == E_COUNT
    assert call(problems=-1, pol=None, q=8, dsa=66, start=65) == E_COUNT      # before the alignment
    # 10. alignment
    for kw in (dict(pol=None, q=72), dict(pol=None, q=8), dict(pol=None, thr=72), dict(pol=None, thr=4), dict(dsa=72), dict(dsa=8),
               dict(do=66), dict(start=66), dict(start=65), dict(d_init=65), dict(run=70), dict(delta=67)):
        assert call(**kw) == E_ALIGN, kw
        assert call(problems=0, **kw) == E_ALIGN, kw                # before "nothing to do"
    assert call(p=v3, goal=68) == E_ALIGN
    assert call(goal=68, problems=0) == 0                           # v0: not read, not judged
    assert call(pol=65, problems=0) == 0                            # bytes: no alignment asked of them
    assert call(do=68, start=68, d_init=68, problems=0) == 0        # floats: 4 bytes
    # 11. nothing to do: nothing is read, whatever the addresses; tol is never judged
    for kw in (dict(), dict(do=None), dict(dsa=None), dict(pol=None, q=64), dict(pol=None, thr=64, eps=77), dict(p=v3),
               dict(p=P(mode=abi.LAYOUT_PER_ENV)), dict(tol=-1.0), dict(tol=float("nan")), dict(d_init=64, run=None, delta=None)):
        assert call(problems=0, **kw) == 0, kw
    # a grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration (9), from grid_ok, before any launch
    assert call(p=P(grid=17), problems=1 << 24) == 9
    assert call(p=P(grid=16), problems=1 << 26) == 9


def test_describe_occupancy_refusals_and_plan(abi):
    d = abi.lib.lmaze_describe_occupancy
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
    assert abi.describe_occupancy(P(), 0) == ""
    assert d(C.byref(P()), 5, buf, 8) == 0 and buf.value == b"occupan"     # truncated to len, always terminated
    with pytest.raises(abi.LmazeError):
        abi.describe_occupancy(P(grid=2), 1)
    # the plan is lmaze_solve's at every size, both variants, both layout modes
    for G in range(3, 65):
        for mode in (abi.LAYOUT_SHARED, abi.LAYOUT_PER_ENV):
            for variant, tag in ((abi.VARIANT_V0, "v0"), (abi.VARIANT_V3, "v3")):
                p = P(variant, G, mode)
                for problems in (1, 5, 259, 65536):
                    line = abi.describe_occupancy(p, problems)
                    assert line == abi.describe_solve(p, problems).replace("solve_kernel", "occupancy_kernel"), line
                    assert re.match(r"occupancy_kernel<%s, (wave|workgroup), (\d+)> grid=(\d+) block=256 lds=(\d+) "
                                    r"problems_per_workgroup=(\d+)$" % tag, line), line


def test_python_refusals_that_need_no_device(lm):
    import torch
    V = lm.vec_env
    cpu = torch.device("cpu")
    lay = torch.from_numpy(H.bordered_random_layouts(2, 11, 3))
    pol = torch.zeros((2, 121), dtype=torch.uint8)
    q = torch.zeros((2, 121, 4))
    # exactly one table: judged before the mazes, so without a device
    for kw in (dict(), dict(policy=pol, q=q), dict(policy=pol, thresholds=q.to(torch.int32)), dict(probs=q, logits=q)):
        with pytest.raises(ValueError, match="exactly one|one of"):
            lm.occupancy_tables(lay, **kw)
    # start: shape, dtype, device, sign
    ok = torch.full((2, 121), 0.5)
    V._check_start(ok, cpu, 2, 121, True)
    bad = [ok[:1], ok.reshape(-1), ok.double(), ok.t().contiguous().t(), ok.to("meta"), None]
    for s in bad:
        with pytest.raises(ValueError, match="start"):
            V._check_start(s, cpu, 2, 121, True)
    for value in (-1e-9, float("nan"), float("inf")):
        neg = ok.clone()
        neg[1, 7] = value
        with pytest.raises(ValueError, match="negative or non-finite"):
            V._check_start(neg, cpu, 2, 121, True)
        V._check_start(neg, cpu, 2, 121, False)                              # validate=False: not looked at
    # start="state" with key="goal", and a start that is neither: refused before the env is looked at
    with pytest.raises(ValueError, match="key='goal'"):
        lm.LmazeVecEnv._occupancy_start(None, "state", "goal", None, 121, False)
    for s in ("cells", 3, None):
        with pytest.raises(ValueError, match="start"):
            lm.LmazeVecEnv._occupancy_start(None, s, "ball", None, 1, True)
    # reset_distribution's own
    for kw in (dict(variant="v1"), dict(variant="v3"), dict(goals=torch.zeros((2, 2), dtype=torch.int32)),
               dict(variant="v3", goals=torch.zeros((3, 2), dtype=torch.int32))):
        with pytest.raises(ValueError):
            lm.reset_distribution(lay, **kw)
    with pytest.raises(ValueError):
        lm.reset_distribution(lay.float())


# ------------------------------------------------------------- reset_distribution against the oracle
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_reset_distribution_is_the_oracles_support(lm, variant):
    """The cells the oracle's reset lands on over 2^16 draws per layout (v3: per goal it drew, the goals drawn most often):
    the same support, and one weight, 1 / its size, on all of it.  A cell of a support of at most 81 is missed by 2^10 draws
    with probability below 81 * exp(-2^10 / 81) < 3e-4; the seeds are fixed."""
    import torch
    shipped = lm.layouts.to_codes(lm.VARIANTS[variant]["layout"])
    lays = [np.ascontiguousarray(shipped)] + [np.ascontiguousarray(x) for x in H.bordered_random_layouts(3, 11, 5)]
    n = 1 << 16
    for i, lay in enumerate(lays):
        G = lay.shape[0]
        ball, goal = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
        p = O.params(O.VARIANT_V3 if variant == "v3" else O.VARIANT_V0, G)
        O.reset(p, lay, None, 100 + i, 0, ball, goal if variant == "v3" else None, np.zeros(n, np.int32), np.zeros(n, np.float32),
                np.zeros(n, np.uint8))
        cells = ball[:, 0] * G + ball[:, 1]
        if variant == "v0":
            groups = [(None, cells)]
        else:
            gc = goal[:, 0] * G + goal[:, 1]
            top = np.argsort(np.bincount(gc, minlength=G * G))[::-1][:3]
            groups = [(g, cells[gc == g]) for g in top]
        for g, drawn in groups:
            goals = None if g is None else torch.tensor([[g // G, g % G]], dtype=torch.int32)
            got = lm.reset_distribution(torch.from_numpy(lay.copy()), variant, goals).numpy()
            assert got.shape == (1, G * G) and got.dtype == np.float32
            hit = np.bincount(drawn, minlength=G * G) > 0
            assert len(drawn) >= 1 << 9 and ((got[0] > 0) == hit).all(), (variant, i, g)
            assert (got[0][hit] == np.float32(1) / np.float32(hit.sum())).all()
    # batched: per-env layouts give their rows; one shared layout with P goals gives P rows
    batch = torch.from_numpy(np.stack(lays[1:]))
    if variant == "v0":
        rows = lm.reset_distribution(batch).numpy()
        for j in range(3):
            assert (rows[j] == lm.reset_distribution(batch[j]).numpy()[0]).all()
    else:
        goals = torch.tensor([[1, 1], [9, 9], [-1, 4], [0, 0]], dtype=torch.int32)
        rows = lm.reset_distribution(batch[0], "v3", goals).numpy()
        assert rows.shape == (4, 121) and rows[0, 12] == 0 and rows[1, 12] > 0 and (rows[2] == rows[3]).all()


# ------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_stacked_is_the_per_problem_reference(variant, mazes):
    lays, _, _ = mazes
    rs = np.random.RandomState(3)
    P, S = len(lays), lays.shape[-1] ** 2
    goals = H.random_free_cells(lays, 5) if variant == "v3" else None
    models = SR.models_of(variant, lays, goals)
    pol = rs.randint(0, 4, (P, S)).astype(np.uint8)
    pol[rs.rand(P, S) < 0.05] = 9
    q = rs.choice(np.array([-1.0, 0.0, 0.0, 2.0, np.nan], np.float32), (P, S, 4))
    start = rs.rand(P, S).astype(np.float32)
    d0 = rs.randn(P, S).astype(np.float32)                                  # walls too, and negative
    cases = [dict(policy=pol, epsilon_u32=0), dict(policy=pol, epsilon_u32=(1 << 28) + 3), dict(q=q, epsilon_u32=(1 << 32) - 1),
             dict(thresholds=random_thresholds(rs, (P, S)))]
    for table in cases:
        for kw in (dict(sweeps=3000), dict(sweeps=7), dict(sweeps=3000, tol=1e-3), dict(sweeps=3000, d_init=d0)):
            many = OR.occupancy_many(models, 0.99, start=start, **kw, **table)
            for p in range(P):
                one_kw = dict(kw)
                if "d_init" in one_kw:
                    one_kw["d_init"] = d0[p]
                one = OR.occupancy(models[p], 0.99, start=start[p], **one_kw,
                                   **{k: (t if k == "epsilon_u32" else t[p]) for k, t in table.items()})
                for name in ("d", "d_sa", "sweeps_run", "delta"):
                    a, b = np.asarray(getattr(many, name)[p]), np.asarray(getattr(one, name))
                    assert a.tobytes() == b.tobytes(), (variant, sorted(table), kw, p, name)


def settled_cases(mazes, gamma, seed):
    """The settled problems of test_evaluate_cpu.py: per maze the planner's policy at four epsilons and one sorted thresholds
    table, each with the occupancy reference run to its exact stop from the reset law"""
    lays, models, solved = mazes
    rs = np.random.RandomState(seed)
    S = lays.shape[-1] ** 2
    for p, m in enumerate(models):
        start = uniform_start(m)
        tables = [dict(policy=solved[gamma][p].policy, epsilon_u32=e) for e in EPSILONS] + [dict(thresholds=random_thresholds(rs, (S,), 0.0))]
        for table in tables:
            history = []
            got = OR.occupancy(m, gamma, 20000, start, history=history, **table)
            assert got.sweeps_run < 20000 and got.delta == 0, (p, sorted(table))      # the exact stop is reached
            yield p, m, table, start, got, history


@pytest.mark.parametrize("gamma", [0.9, 0.99])
def test_float32_fixed_point_is_the_linear_solve(gamma, mazes):
    """|| d32 - d ||_1 <= rel(11) max(|| d ||_1, || d32 ||_1) / (1 - gamma): d_bound() above derives it, ROUNDINGS counts the
    roundings per cell and sweep.  Worst ratio err / bound seen: 0.091 at gamma = 0.9, 0.097 at gamma = 0.99 (profiles/occupancy/README.md)."""
    worst, n = 0.0, 0
    for p, m, table, start, got, _ in settled_cases(mazes, gamma, 11):
        exact, _ = OR.exact_occupancy(m, gamma, E.weights(**table), start)
        assert (exact >= 0).all()
        err = np.abs(got.d.astype(np.float64) - exact).sum()
        bound = d_bound(float(np.float32(gamma)), max(exact.sum(), got.d.astype(np.float64).sum()))
        worst = max(worst, err / bound)
        print("gamma", gamma, "maze", p, sorted(table)[0], table.get("epsilon_u32"), "sweeps", int(got.sweeps_run), "err", err, "bound", bound)
        assert err <= bound
        n += 1
    print("gamma", gamma, "worst err / bound", worst)
    assert n == 30


@pytest.mark.parametrize("gamma", [0.9, 0.99])
def test_duality_of_the_two_float32_references(gamma, mazes):
    """J two ways, in float64 from the float32 tables: <start, V32> and <d_sa32, r>.  Exactly <start, V> = <d_sa, r>.
    |<start, V32 - V>| <= || start ||_1 * 8 u M / (1 - gamma) (test_evaluate_cpu.py's bound, M = max |Q|), and
    |<d_sa32 - d_sa, r>| <= R || d_sa32 - d_sa ||_1 with R = max |r| over the usable pairs and d_sa32 = fl(d32 p32),
    p32 = p (1 + 3 roundings), the p of a state summing to 1:  || d_sa32 - d_sa ||_1 <= (1 + rel(4)) || d32 - d ||_1 + rel(4) || d ||_1
    with d_bound() for the first norm."""
    g32 = float(np.float32(gamma))
    worst = 0.0
    for p, m, table, start, got, _ in settled_cases(mazes, gamma, 12):
        ev = E.evaluate(m, gamma, 20000, **table)
        assert ev.sweeps_run < 20000
        use = ~m.sticky & ~m.wall[:, None]
        r = np.where(use, m.r, 0).astype(np.float64)
        j_v = float((start.astype(np.float64) * ev.v.astype(np.float64)).sum())
        j_d = float((got.d_sa.astype(np.float64) * r).sum())
        M = float(np.abs(ev.q[np.isfinite(ev.q)]).max())
        R = float(np.abs(r).max())
        d_norm = float(got.d.astype(np.float64).sum()) * (1 + 2 * d_bound(g32, 1.0))       # covers || d ||_1 as well
        bound = float(start.astype(np.float64).sum()) * V_ROUNDINGS * U * M / (1 - g32) \
            + R * ((1 + rel(4)) * d_bound(g32, d_norm) + rel(4) * d_norm)
        worst = max(worst, abs(j_v - j_d) / bound)
        print("gamma", gamma, "maze", p, sorted(table)[0], table.get("epsilon_u32"), "J", j_v, j_d, "bound", bound)
        assert abs(j_v - j_d) <= bound
    print("gamma", gamma, "worst |dJ| / bound", worst)


@pytest.mark.parametrize("gamma", [0.9, 0.99])
def test_sweeps_are_monotone_from_zero(gamma, mazes):
    """From d_init = None and a start without a negative entry every D_k >= D_(k-1) in every cell, and the exact stop is reached
    on every case (settled_cases asserts that)"""
    n = 0
    for p, m, table, start, got, history in settled_cases(mazes, gamma, 13):
        h = np.stack([np.zeros_like(history[0])] + history)
        assert (h[1:] >= h[:-1]).all(), (p, sorted(table))
        assert len(history) == got.sweeps_run and (history[-1] == history[-2]).all()
        n += 1
    assert n == 30


def test_free_border_model_by_padding():
    """occupancy_ref.pad_walls / unpad_model: on a bordered layout the padded model is the model"""
    lays = H.bordered_random_layouts(3, 7, 2)
    for lay in lays:
        a = SR.extract_model("v0", lay)
        b = OR.unpad_model(SR.extract_model("v0", OR.pad_walls(lay)))
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


# ------------------------------------------------------------- what the kernels need
@pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not installed")
def test_occupancy_kernels_use_no_scratch():
    """Fourteen kernels (two variants; three wave forms, four workgroup forms), none with scratch: the descriptor, the four
    incoming weights, wself and start of every cell a lane owns stay in registers, 7 per cell, 112 at sixteen cells per lane.
    The counts are the ones measured per form (v0 / v3 where they differ: the larger)."""
    usage = H.kernel_usage("lmaze_occupancy.hip")
    mine = {k: v for k, v in usage.items() if "occupancy_kernel" in k}
    assert len(mine) == 14, sorted(usage)
    for name, v in mine.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        print(name, v)
        wave = "Lb1E" in name
        cpl = int(re.search(r"ILi\dELi(\d+)E", name).group(1))
        assert v["VGPRs"] <= ({1: 37, 2: 34, 4: 47} if wave else {2: 30, 4: 45, 8: 82, 16: 155})[cpl], (name, v)
        if cpl == 16:
            assert v["Occupancy"] >= 2, (name, v)                   # two workgroups share a CU, as evaluate_kernel's
