"""GPU: what occupancy() says, held against where closed-loop rollouts really put the ball.  test_gpu_occupancy.py pins the
kernel to occupancy_ref, and both read one model, solve_ref's; here the transitions are the step kernel's own.
(a) The successor table is built from the rows of rollout_sample() and rollout_policy(epsilon = 0.25) alone (key, action, done,
    next key; every pair of every checked problem seen, see occupancy_rollout_ref.case_rows), win / src / wself are gathered
    from it, and one sweep of occupancy_ref over those applied to the GPU's d returns d in every bit; d_sa = fl(d p) with p the
    exact law of the rule that ran (policy_law.py).  The start is reset_distribution(), gamma 0.9, every problem at its exact
    stop.  It fails if the kernel's gather disagrees with the transitions the step makes (a clamp, a row guard, which pairs
    flow), if a terminal pair leaks mass, or if the weights inside lmaze_occupancy are not the running sampler's law.
(b) The number of running envs on every cell before every step t < 32 of rollout_sample(auto_reset=False) follows
    Binomial(N, mu_t[s]), mu_t = (P_pi^T)^t start over the model in float64 (exact binomial tails, ALPHA / bins), from one cell
    and -- the first test of reset_distribution() against the cells reset() itself places balls on -- from a plain reset(); and
    occupancy(sweeps=32, d_init=None) is sum_{j<32} g^j mu_j within the rounding bound, at g = 0.9 and g = 1.  Mazes without a
    refused pair only: the model renormalises the mass a table puts on v0's sticky pairs, while a rollout spends a step in place
    there, so next to an 'S' the step marginals are not the model's.
test_occupancy_vs_rollouts_cpu.py runs the same cases on rows of the C oracle with occupancy_ref in the kernel's place.
Nothing outside the tree is read."""
import importlib

import numpy as np
import pytest
import torch

import occupancy_rollout_ref as RR
import test_gpu_planning_vs_rollouts as PR
import test_occupancy_vs_rollouts_cpu as TW

pytestmark = pytest.mark.gpu

T, GAMMA, SWEEPS, EPSILON, ALPHA = PR.T, PR.GAMMA, PR.SWEEPS, PR.EPSILON, PR.ALPHA


@pytest.fixture(scope="module")
def lm():
    assert torch.cuda.is_available()
    return importlib.import_module("gym-lmaze_amd")


def place(env, ball_xy, goal_xy=None):
    n = env.num_envs
    state = dict(ball_xy=ball_xy, reward=np.full(n, -0.01, np.float32), done=np.zeros(n, np.uint8), step_count=np.zeros(n, np.int32))
    if goal_xy is not None:
        state["goal_xy"] = goal_xy
    env.set_state(**state)


class Adapter:
    """occupancy_rollout_ref.case_rows()'s adapter over an LmazeVecEnv; a table goes up once"""

    def __init__(self, env):
        self.env, self.up = env, {}

    def table(self, x):
        if id(x) not in self.up:
            self.up[id(x)] = (x, PR.up(x))
        return self.up[id(x)][1]

    def place(self, ball_xy, goal_xy=None):
        place(self.env, ball_xy, goal_xy)

    def sample(self, steps, thr, key):
        out = self.env.rollout_sample(steps, thresholds=self.table(thr).reshape(-1, 4), key=key, auto_reset=True, trajectory=True)
        return PR.rows_of(self.env, out, key)

    def greedy(self, steps, pol, epsilon, key):
        out = self.env.rollout_policy(steps, policy=self.table(pol), epsilon=epsilon, key=key, auto_reset=True, trajectory=True)
        return PR.rows_of(self.env, out, key)


# ------------------------------------------------------------- (a)
@pytest.mark.parametrize("variant,layouts,key,N", PR.CASES)
def test_occupancy_is_stationary_under_the_rollouts_own_transitions(lm, variant, layouts, key, N):
    w = PR.world(lm, variant, layouts, key, N)
    what = "%s %s key=%s" % (variant, layouts, key)
    thr, pol = PR.threshold_table(w["entries"], PR.THRESHOLD_SEED), PR.byte_table(w["entries"], PR.BYTE_SEED)
    env = PR.make_env(lm, variant, layouts, w, N, seed=7)
    ad = Adapter(env)
    rows, goals = RR.case_rows(ad, variant, layouts, key, N, w["lay"], w["entries"], thr, pol, T, EPSILON)
    pkey = "ball" if layouts == "per_env" else key
    p_s, p_g = TW.laws(w, thr, pol)
    tables = []
    for name, p, kw in (("sample", p_s, dict(thresholds=ad.table(thr))), ("bytes", p_g, dict(policy=ad.table(pol), epsilon=EPSILON))):
        got = env.occupancy(key=pkey, gamma=GAMMA, sweeps=SWEEPS, **kw)                 # start="reset"
        assert bool((got.sweeps_run < SWEEPS).all()) and bool((got.delta == 0).all()), (what, name)
        tables.append((name, p, got.d.cpu().numpy().reshape(-1), got.d_sa.cpu().numpy().reshape(-1, 4)))
        assert tables[-1][2].shape == (w["entries"],)
    start = TW.case_start(lm, variant, layouts, w)
    assert RR.check_flows(w, key, N, rows, goals, start, GAMMA, tables, what) > 0


# ------------------------------------------------------------- (b)
@pytest.mark.parametrize("case", range(3))
def test_running_envs_follow_the_law_occupancy_sums(lm, case):
    name, variant, lay, goal, cell = TW.marginal_cases(lm)[case]
    G = lay.shape[0]
    N = TW.B_N
    model, thr, start, mu = TW.marginal_setup(lm, name, variant, lay, goal, cell)
    env = lm.LmazeVecEnv(N, variant=variant, layout=lay, seed=11, step_limit=PR.STEP_LIMIT, device=PR.dev())
    env.reset()
    goal_xy = None if goal is None else (goal // G, goal % G)
    if cell is not None:
        place(env, np.tile(np.array([cell // G, cell % G], np.int32), (N, 1)),
              None if goal is None else np.tile(np.array(goal_xy, np.int32), (N, 1)))
    table = PR.up(thr)
    out = env.rollout_sample(T, thresholds=table, key="ball", auto_reset=False, trajectory=True)
    rows = PR.rows_of(env, out, "ball")
    assert rows[1].any()
    RR.counts_follow_marginals(RR.running_counts(rows, G * G), mu, N, ALPHA, name)
    for g in (0.9, 1.0):                                                   # gamma is not validated: 1 is accepted
        got = env.occupancy(thresholds=table, key="ball", goal=goal_xy, start=PR.up(start), gamma=g, sweeps=T)
        d = got.d.cpu().numpy().astype(np.float64)
        want = RR.partial_sum(mu, g)
        err = np.abs(d - want).sum()
        bound = RR.partial_bound(g, T, max(want.sum(), d.sum()))
        print(name, "gamma", g, "sweeps", int(got.sweeps_run), "|| D32 - D ||_1", err, "bound", bound, "ratio", err / bound)
        assert int(got.sweeps_run) == T or g < 1
        assert err <= bound
