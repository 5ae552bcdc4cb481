"""CPU: lmaze_evaluate / lmaze_describe_evaluate without a GPU -- the reference against itself (evaluate_ref.py: the stacked
sweep against the per-problem one, the float32 fixed point against a float64 linear solve, V^pi of the planner's own policy
against V*), the weight rule's corner cases, every documented refusal in its order of precedence (answered before any device
call), the launch the describe call names at every plan step, and what the kernels need."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import evaluate_ref as E
import helpers as H
import solve_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
MAX_ENVS = 1 << 30
EPSILONS = (0, 1 << 28, 1 << 31, (1 << 32) - 1)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


@pytest.fixture(scope="module")
def mazes():
    """Six random 11 x 11 mazes with an 'S' each, their v0 models, and what solve_ref plans at both discounts"""
    lays = H.bordered_random_layouts(6, 11, 7)
    models = SR.models_of("v0", lays, None)
    solved = {g: [SR.solve(m, g, 8192) for m in models] for g in (0.9, 0.99)}
    return lays, models, solved


def random_thresholds(rs, shape, wild=0.2):
    """uint32[..., 4]: sorted rows, a share of them left unsorted, word 3 noise"""
    c = rs.randint(0, 1 << 32, size=shape + (4,), dtype=np.uint64).astype(np.uint32)
    ordered = np.sort(c[..., :3], axis=-1)
    keep = rs.rand(*shape) < wild
    c[..., :3] = np.where(keep[..., None], c[..., :3], ordered)
    return c


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
    v0 = rs.randn(P, S).astype(np.float32)                                  # walls too: the first sweep zeroes them
    cases = [dict(policy=pol, epsilon_u32=0), dict(policy=pol, epsilon_u32=(1 << 28) + 3), dict(q=q, epsilon_u32=(1 << 32) - 1),
             dict(thresholds=random_thresholds(rs, (P, S)))]
    for table in cases:
        for kw in (dict(sweeps=3000), dict(sweeps=7), dict(sweeps=3000, tol=1e-3), dict(sweeps=3000, v_init=v0)):
            many = E.evaluate_many(variant, lays, goals, 0.99, models=models, **kw, **table)
            for p in range(P):
                one_kw = dict(kw)
                if "v_init" in one_kw:
                    one_kw["v_init"] = v0[p]
                one = E.evaluate(models[p], 0.99, **one_kw, **{k: (t if k == "epsilon_u32" else t[p]) for k, t in table.items()})
                for name in ("q", "v", "sweeps_run", "delta"):
                    a, b = np.asarray(getattr(many, name)[p]), np.asarray(getattr(one, name))
                    assert a.tobytes() == b.tobytes(), (variant, sorted(table), kw, p, name)


@pytest.mark.parametrize("gamma", [0.9, 0.99])
def test_float32_fixed_point_is_the_linear_solve(gamma, mazes):
    """On settled problems |v - v64| <= 8 u M / (1 - gamma), u = 2^-24, M = max |Q|: a cell's value takes at most 8 roundings per
    sweep (the conversions and the division behind p, the product and the sum of the backup, the product with p, the sums over
    the actions), each at most u relative to a magnitude <= M, and the contraction amplifies a per-sweep error by 1 / (1 - gamma)."""
    lays, models, solved = mazes
    rs = np.random.RandomState(11)
    S = lays.shape[-1] ** 2
    settled = 0
    for p, m in enumerate(models):
        tables = [dict(policy=solved[gamma][p].policy, epsilon_u32=e) for e in EPSILONS] + [dict(thresholds=random_thresholds(rs, (S,), 0.0))]
        for table in tables:
            got = E.evaluate(m, gamma, 8192, **table)
            assert got.sweeps_run < 8192, (p, sorted(table))                # every case settles: the exact stop is reachable
            settled += 1
            exact = E.exact_values(m, gamma, E.weights(**table))
            M = np.abs(got.q[np.isfinite(got.q)]).max()
            err = np.abs(got.v.astype(np.float64) - exact).max()
            bound = 8 * U * M / (1 - gamma)
            print("gamma", gamma, "maze", p, sorted(table)[0], table.get("epsilon_u32"), "sweeps", int(got.sweeps_run), "err", err, "bound", bound)
            assert err <= bound
    assert settled == len(models) * 5


@pytest.mark.parametrize("gamma", [0.9, 0.99])
def test_planner_policy_evaluates_to_v_star(gamma, mazes):
    """epsilon = 0, the planner's own policy, started from its settled values: the first sweep changes no bit"""
    _, models, solved = mazes
    for m, s in zip(models, solved[gamma]):
        assert s.sweeps_run < 8192
        got = E.evaluate(m, gamma, 50, v_init=s.v, policy=s.policy, epsilon_u32=0)
        assert got.sweeps_run == 1 and got.delta == 0
        assert (SR.bits(got.v) == SR.bits(s.v)).all()
        # and from zero it gets there on its own
        cold = E.evaluate(m, gamma, 8192, policy=s.policy, epsilon_u32=0)
        assert cold.sweeps_run < 8192 and (SR.bits(cold.v) == SR.bits(s.v)).all()


# ------------------------------------------------------------- the weight rule
def test_thresholds_of_epsilon_greedy_probabilities_give_its_weights(abi):
    """Where the mixture is representable -- epsilon_u32 a multiple of 4 and not 0 -- the sampler's converter gives thresholds
    whose weights are the epsilon-greedy ones"""
    import torch
    rs = np.random.RandomState(2)
    pol = rs.randint(0, 4, 500).astype(np.uint8)
    for e in (4, 1 << 28, (1 << 28) + 4, 1 << 31, (1 << 32) - 4):
        w = E.weights(policy=pol, epsilon_u32=e)
        assert (w.sum(-1) == E.FULL).all()
        thr = abi.sampling_thresholds(torch.from_numpy(w.astype(np.float64) / E.FULL)).view(torch.int32).numpy()
        assert (E.weights(thresholds=thr) == w).all(), e
    odd = E.weights(policy=pol, epsilon_u32=(1 << 28) + 3)                     # not representable: the thresholds round
    thr = abi.sampling_thresholds(torch.from_numpy(odd.astype(np.float64) / E.FULL)).view(torch.int32).numpy()
    assert (E.weights(thresholds=thr) != odd).any() and np.abs(E.weights(thresholds=thr) - odd).max() <= 4


def test_one_hot_row_keeps_a_draw_for_action_three(abi):
    import torch
    thr = abi.sampling_thresholds(torch.eye(4, dtype=torch.float64)).view(torch.int32).numpy()
    w = E.weights(thresholds=thr)
    top = 4 * ((1 << 32) - 1)
    assert w.tolist() == [[top, 0, 0, 4], [0, top, 0, 4], [0, 0, top, 4], [0, 0, 0, 1 << 34]]
    # a non-monotone row has the weights of its sorted words, which is how often the sampler's compares give each action
    w = E.weights(thresholds=np.array([[10, 5, 20, 77]], np.uint32))
    assert w.tolist() == [[20, 20, 40, 4 * ((1 << 32) - 20)]]


def test_mass_on_sticky_pairs_and_bytes_above_three(mazes):
    _, models, solved = mazes
    seen = 0
    for m, s in zip(models, solved[0.99]):
        pol = s.policy.copy()
        cells, acts = np.nonzero(m.sticky)
        assert len(cells)                                                   # every maze has its 'S'
        s0, a0 = int(cells[0]), int(acts[0])
        pol[s0] = a0                                                        # the whole mass on a sticky pair
        free = np.flatnonzero(~m.wall & ~m.sticky.any(1))
        s1 = int(free[len(free) // 2])
        pol[s1] = 200                                                       # no action at all
        got = E.evaluate(m, 0.99, 8192, policy=pol, epsilon_u32=0)
        assert got.v[s0] == 0 and got.v[s1] == 0
        assert np.isneginf(got.q[s0, a0]) and np.isfinite(got.q[s1]).all()
        # with exploration the same states are worth something: the sticky state renormalises over its usable pairs
        w = E.weights(policy=pol, epsilon_u32=1 << 30)
        p = E.probabilities(w, m.sticky, m.wall)
        assert E.renormalised(w, m.sticky, m.wall)[s0] and not E.renormalised(w, m.sticky, m.wall)[s1]
        usable = ~m.sticky[s0]
        assert (p[s0][usable] == np.float32(1) / np.float32(usable.sum())).all() and (p[s0][~usable] == 0).all()
        assert (p[s1] == 0.25).all()
        seen += 1
    assert seen == len(models)


# ------------------------------------------------------------- refusals
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_evaluate", "lmaze_describe_evaluate"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    lm = importlib.import_module("gym-lmaze_amd")
    assert callable(lm.evaluate_tables) and callable(lm.LmazeVecEnv.evaluate) and callable(abi.describe_evaluate)
    assert lm.EvaluatedTables._fields == ("q", "v", "sweeps_run", "delta")
    assert "evaluate_tables" in lm.__all__ and "EvaluatedTables" in lm.__all__


def test_evaluate_refusals_in_order(abi):
    f = abi.lib.lmaze_evaluate

    def P(variant=abi.VARIANT_V0, grid=12, mode=abi.LAYOUT_SHARED):
        return abi.make_params(variant, grid, mode, 100, -1.0, -0.01, 100.0)

    def call(p=None, lay=64, goal=64, problems=3, pol=64, q=None, eps=0, thr=None, sweeps=10, tol=0.0, v_init=None, qo=64, vo=64,
             run=64, delta=64):
        p = P() if p is None else p
        return f(C.byref(p) if p != "null" else None, lay, goal, problems, pol, q, eps, thr, 0.99, sweeps, tol, v_init, qo, vo, run,
                 delta, None)
    v3 = P(abi.VARIANT_V3, 18)
    none = dict(qo=None, vo=None)
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
    # 6. neither q_out nor v_out
    assert call(**none) == E_NULL and call(problems=-1, pol=None, **none) == E_NULL
    assert call(qo=None, problems=0) == 0 and call(vo=None, problems=0) == 0 and call(run=None, delta=None, problems=0) == 0
    # 7. exactly one policy input
    assert call(pol=None) == E_NULL and call(pol=None, problems=-1, sweeps=0) == E_NULL
    for kw in (dict(q=64), dict(thr=64), dict(q=64, thr=64), dict(pol=None, q=64, thr=64)):
        assert call(**kw) == E_NULL and call(problems=-1, **kw) == E_NULL and call(problems=0, qo=8, **kw) == E_NULL, kw
    # 8. the counts
    assert call(problems=-1) == E_COUNT and call(problems=MAX_ENVS + 1) == E_COUNT
    assert call(sweeps=0) == E_COUNT and call(sweeps=-5, problems=0) == E_COUNT
    assert call(problems=-1, pol=None, q=8, qo=66) == E_COUNT       # before the alignment
    # 9. alignment
    for kw in (dict(pol=None, q=72), dict(pol=None, q=8), dict(pol=None, thr=72), dict(pol=None, thr=4), dict(qo=72), dict(qo=8),
               dict(vo=66), dict(v_init=65), dict(run=70), dict(delta=67)):
        assert call(**kw) == E_ALIGN, kw
        assert call(problems=0, **kw) == E_ALIGN, kw                # before "nothing to do"
    assert call(p=v3, goal=68) == E_ALIGN
    assert call(goal=68, problems=0) == 0                           # v0: not read, not judged
    assert call(pol=65, problems=0) == 0                            # bytes: no alignment asked of them
    # 10. nothing to do: nothing is read, whatever the addresses; tol is never judged
    for kw in (dict(), dict(qo=None), dict(vo=None), dict(pol=None, q=64), dict(pol=None, thr=64, eps=77), dict(p=v3),
               dict(p=P(mode=abi.LAYOUT_PER_ENV)), dict(tol=-1.0), dict(tol=float("nan")), dict(v_init=64, run=None, delta=None)):
        assert call(problems=0, **kw) == 0, kw
    # a grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration (9), from grid_ok, before any launch
    assert call(p=P(grid=17), problems=1 << 24) == 9
    assert call(p=P(grid=16), problems=1 << 26) == 9


def test_describe_evaluate_refusals(abi):
    d = abi.lib.lmaze_describe_evaluate
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
    assert abi.describe_evaluate(P(), 0) == ""
    assert d(C.byref(P()), 5, buf, 8) == 0 and buf.value == b"evaluat"     # truncated to len, always terminated
    with pytest.raises(abi.LmazeError):
        abi.describe_evaluate(P(grid=2), 1)


# ------------------------------------------------------------- what a describe line must say
def test_describe_evaluate_every_plan_step(abi):
    """The plan is lmaze_solve's: the same form, cells per lane, grid and LDS at every size, both variants, both layout modes"""
    want = {3: ("wave", 1), 8: ("wave", 1), 9: ("wave", 2), 11: ("wave", 2), 12: ("wave", 4), 16: ("wave", 4), 17: ("workgroup", 2),
            22: ("workgroup", 2), 23: ("workgroup", 4), 32: ("workgroup", 4), 33: ("workgroup", 8), 45: ("workgroup", 8),
            46: ("workgroup", 16), 64: ("workgroup", 16)}
    for G in range(3, 65):
        for mode in (abi.LAYOUT_SHARED, abi.LAYOUT_PER_ENV):
            for variant, tag in ((abi.VARIANT_V0, "v0"), (abi.VARIANT_V3, "v3")):
                p = abi.make_params(variant, G, mode, 100, -1.0, -0.01, 100.0)
                for problems in (1, 4, 5, 7, 259, 65536):
                    line = abi.describe_evaluate(p, problems)
                    assert line == abi.describe_solve(p, problems).replace("solve_kernel", "evaluate_kernel"), line
                    m = re.match(r"evaluate_kernel<(v0|v3), (wave|workgroup), (\d+)> grid=(\d+) block=256 lds=(\d+) problems_per_workgroup=(\d+)$", line)
                    assert m and m.group(1) == tag, line
                    if G in want:
                        assert (m.group(2), int(m.group(3))) == want[G], line


# ------------------------------------------------------------- what the kernels need
@pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not installed")
def test_evaluate_kernels_use_no_scratch():
    """Fourteen kernels (two variants; three wave forms, four workgroup forms), none with scratch: the descriptor and the four
    probabilities of every cell a lane owns stay in registers, 5 per cell, 80 at sixteen cells per lane"""
    usage = H.kernel_usage("lmaze_evaluate.hip")
    mine = {k: v for k, v in usage.items() if "evaluate_kernel" in k}
    assert len(mine) == 14, sorted(usage)
    for name, v in mine.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        print(name, v)
        wave = "Lb1E" in name                                       # and no form above what it had before the shared frame
        cpl = int(re.search(r"ILi\dELi(\d+)E", name).group(1))
        assert v["VGPRs"] <= ({1: 32, 2: 40, 4: 65} if wave else {2: 39, 4: 64, 8: 117, 16: 226})[cpl], (name, v)
