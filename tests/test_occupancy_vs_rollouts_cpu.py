"""CPU: the twin of test_gpu_occupancy_vs_rollouts.py -- the same cases, seeds and shapes with rows made by the C oracle under
closed_loop_ref's draws (occupancy_rollout_ref.HostEnv, epoch for epoch as LmazeVecEnv spends them) and occupancy_ref in the
place of the kernel.  It establishes, before a GPU is asked, that at the committed values the references alone see every pair
(a), keep every binomial tail (b) and reach every exact stop; and it holds occupancy_ref to the flow identity over the
transitions the oracle makes, which occupancy_ref.gather() otherwise takes from solve_ref's model."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import evaluate_ref as E
import maze_ref as MZ
import occupancy_ref as OR
import occupancy_rollout_ref as RR
import policy_law as L
import solve_ref as SR
import test_gpu_planning_vs_rollouts as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, GAMMA, SWEEPS, EPSILON, ALPHA = PR.T, PR.GAMMA, PR.SWEEPS, PR.EPSILON, PR.ALPHA
MAZE_SEED = 7                    # maze_ref.generate(11, 1, MAZE_SEED): the 'S'-free v0 maze of (b)
B_N = 8192
B_SEED = 5                       # the thresholds of (b)


@pytest.fixture(scope="module")
def lm():
    if not os.path.exists(os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd")


def reset_law(lm, variant, lay, goals=None):
    """lm.reset_distribution() on the host: float32[problems, S]"""
    import torch
    g = None if goals is None else torch.from_numpy(np.ascontiguousarray(goals, dtype=np.int32))
    return lm.reset_distribution(torch.from_numpy(np.ascontiguousarray(lay).copy()), variant, g).numpy()


def laws(w, thr, pol):
    """The float32 probabilities of the two rules that run, from policy_law's counts: what law_is_what_was_evaluated() uses"""
    p_s = E.probabilities(4 * L.sampling_law(thr), w["sticky"], w["wall"])
    p_g = E.probabilities(L.epsilon_greedy_law(pol, RR.eps_u32(EPSILON))[:, :4], w["sticky"], w["wall"])
    return p_s, p_g


def case_start(lm, variant, layouts, w):
    """start="reset" of a case: float32[problems, S]; key="goal": a row per goal cell"""
    if variant == "v3":
        cells = np.arange(w["S"])
        return reset_law(lm, "v3", w["lay"], np.stack([cells // w["G"], cells % w["G"]], 1))
    return reset_law(lm, "v0", w["lay"])


def models_for(variant, layouts, w, problems):
    G = w["G"]
    if layouts == "per_env":
        return SR.models_of("v0", w["lay"], None)
    if variant == "v3":
        return [SR.extract_model("v3", w["lay"], (p // G, p % G)) for p in problems]
    return [SR.extract_model("v0", w["lay"], None)]


# ------------------------------------------------------------- (a)
@pytest.mark.parametrize("variant,layouts,key,N", PR.CASES)
def test_reference_rows_cover_every_pair_and_keep_the_flow_identity(lm, variant, layouts, key, N):
    w = PR.world(lm, variant, layouts, key, N)
    what = "%s %s key=%s (host)" % (variant, layouts, key)
    thr, pol = PR.threshold_table(w["entries"], PR.THRESHOLD_SEED), PR.byte_table(w["entries"], PR.BYTE_SEED)
    env = RR.HostEnv(variant, w["lay"], N, 7, PR.STEP_LIMIT)
    env.reset()                                                       # make_env()'s
    rows, goals = RR.case_rows(RR.HostAdapter(env), variant, layouts, key, N, w["lay"], w["entries"], thr, pol, T, EPSILON)
    assert int(env.step_count.max()) < PR.STEP_LIMIT - 1
    start = case_start(lm, variant, layouts, w)
    problems = [0] if key == "ball" else ([int(g) for g in goals] if key == "goal" else list(range(N)))
    models = models_for(variant, layouts, w, problems)
    S = w["S"]
    tables = []
    for name, p, table in (("sample", laws(w, thr, pol)[0], dict(thresholds=thr)),
                           ("bytes", laws(w, thr, pol)[1], dict(policy=pol, epsilon_u32=RR.eps_u32(EPSILON)))):
        d, d_sa = np.zeros(w["entries"], np.float32), np.zeros((w["entries"], 4), np.float32)
        sub = {k: (v if k == "epsilon_u32" else np.stack([v[pr * S:(pr + 1) * S] for pr in problems])) for k, v in table.items()}
        got = OR.occupancy_many(models, GAMMA, SWEEPS, start[problems], **sub)
        assert (got.sweeps_run < SWEEPS).all(), what
        for j, pr in enumerate(problems):
            d[pr * S:(pr + 1) * S], d_sa[pr * S:(pr + 1) * S] = got.d[j], got.d_sa[j]
        tables.append((name, p, d, d_sa))
    assert RR.check_flows(w, key, N, rows, goals, start, GAMMA, tables, what) > 0


# ------------------------------------------------------------- (b)
def marginal_cases(lm):
    """(name, variant, layout, goal or None, start float32[S] or None for the env's own reset, the cell all balls stand on)"""
    lay0 = MZ.generate(11, 1, MAZE_SEED)[0][0]
    assert not (lay0 == ord("S")).any()
    lay3 = lm.layouts.to_codes(lm.VARIANTS["v3"]["layout"])              # v3 refuses no pair: marginal_setup() asserts it
    goal = int(RR.spawn_cells(lay3, "v3")[40])
    return (("v0 one cell", "v0", lay0, None, 3 * 11 + 9),
            ("v3 one cell", "v3", lay3, goal, int(RR.spawn_cells(lay3, "v3", goal)[30])),
            ("v0 reset", "v0", lay0, None, None))


def marginal_setup(lm, name, variant, lay, goal, cell):
    """The model, the thresholds, start float32[S], the exact law and mu float64[T,S] of a case of (b)"""
    G = lay.shape[0]
    S = G * G
    model = SR.extract_model(variant, lay, None if goal is None else (goal // G, goal % G))
    assert not model.sticky.any()
    thr = PR.threshold_table(S, B_SEED)
    if cell is None:
        start = reset_law(lm, "v0", lay)[0]
    else:
        start = np.zeros(S, np.float32)
        start[cell] = 1
    prob = E.exact_probabilities(4 * L.sampling_law(thr), model.sticky, model.wall)
    return model, thr, start, OR.step_marginals(model, prob, start, T)


@pytest.mark.parametrize("case", range(3))
def test_reference_counts_follow_the_marginals_and_the_partial_sums(lm, case):
    name, variant, lay, goal, cell = marginal_cases(lm)[case]
    G = lay.shape[0]
    model, thr, start, mu = marginal_setup(lm, name, variant, lay, goal, cell)
    env = RR.HostEnv(variant, lay, B_N, 11, PR.STEP_LIMIT)
    env.reset()
    if cell is not None:
        env.place(np.tile(np.array([cell // G, cell % G], np.int32), (B_N, 1)),
                  None if goal is None else np.tile(np.array([goal // G, goal % G], np.int32), (B_N, 1)))
    rows = env.rollout(T, "ball", False, thresholds=thr)
    assert rows[1].any()                                                   # some episodes end inside T: absorption is in play
    RR.counts_follow_marginals(RR.running_counts(rows, G * G), mu, B_N, ALPHA, name + " (host)")
    for g in (0.9, 1.0):
        got = OR.occupancy(model, g, T, start, thresholds=thr)
        want = RR.partial_sum(mu, g)
        err = np.abs(got.d.astype(np.float64) - want).sum()
        bound = RR.partial_bound(g, T, max(want.sum(), got.d.astype(np.float64).sum()))
        print(name, "gamma", g, "sweeps", int(got.sweeps_run), "|| D32 - D ||_1", err, "bound", bound, "ratio", err / bound)
        assert got.sweeps_run == T or g < 1
        assert err <= bound


def test_partial_bound_is_below_d_bound():
    import test_occupancy_cpu as OC
    assert RR.ROUNDINGS == OC.ROUNDINGS and RR.rel(5) == OC.rel(5)
    for g in (0.5, 0.9, 0.99):
        assert RR.partial_bound(g, T, 3.0) <= OC.d_bound(float(np.float32(g)), 3.0)
    assert RR.partial_bound(1.0, T, 3.0) == RR.rel(RR.ROUNDINGS) * 3.0 * T


def test_step_marginals_sum_to_the_occupancy():
    """occupancy_ref.step_marginals against exact_occupancy: sum_t gamma^t mu_t is the linear solve, and mass only leaves"""
    lays = PR.H.bordered_random_layouts(3, 11, 7)
    rs = np.random.RandomState(1)
    for m in SR.models_of("v0", lays, None):
        thr = PR.threshold_table(121, 2)
        start = np.where(m.wall, 0, rs.rand(121)).astype(np.float32)
        exact, prob = OR.exact_occupancy(m, 0.9, E.weights(thresholds=thr), start)
        mu = OR.step_marginals(m, prob, start, 400)
        assert (np.diff(mu.sum(1)) <= 1e-15).all()
        assert np.abs(RR.partial_sum(mu, 0.9) - exact).sum() <= 1e-12 * exact.sum()
