"""GPU: what action_probs() and vtrace() say, held against the rows the envs write and against evaluate().
test_gpu_offpolicy.py pins the kernels to offpolicy_ref bit for bit, and both could share a mistaken row convention; here the
target is checked to be an estimate of the target table's value (offpolicy_rollout_ref.py holds the cases, the derivations
and the bounds, and test_offpolicy_vs_rollouts_cpu.py runs the same checks on the references alone):
(A) one env per action sequence from every start cell, placed with set_state() and stepped by step(): the expectation of
    vs[0] and pg[0] under action_probs() of the behaviour table, summed exactly, is evaluate(target, sweeps=T, v_init=v) for an
    arbitrary critic v (lam = 1, no clipping), and the clipped, lam < 1 targets follow the float64 recursion over the
    successors the rows show; both forms, three table pairs, gamma 0.9 and 1; four mistakes in the conventions miss by > 100
    bounds;
(B) 262 144 envs, T = 16, rollout_sample(logits=) with auto-resets: vs[t] - v(key_t[t]) is centred per (t, cell) at t = 0, 7
    and 15 with the critic evaluate(logits=target).v; ratios omitted or the tables exchanged exceed the threshold three times;
(C) the rows of rollout_policy(policy=, epsilon=) with bytes above 3 and of rollout_policy(q=) have positive weight under the
    table that ran, and that table against itself has ratio exactly 1.
Nothing outside the tree is read."""
import importlib

import numpy as np
import pytest
import torch

import offpolicy_rollout_ref as X
import offpolicy_ref as R

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
DEV = torch.device("cuda", 0)
EPSILON = {0: 0.0, R.EPSILONS[1]: 0.1, R.EPSILONS[2]: 1.0}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


class Gpu:
    """offpolicy_rollout_ref's engine over the library: LmazeVecEnv's rows, action_probs(), vtrace(), evaluate()"""
    name = "gpu"

    def __init__(self):
        self._up, self._judge = {}, {}

    def record(self, table):
        """the table_policy() record of a Table, made once"""
        if id(table.table) not in self._up:
            self._up[id(table.table)] = (table.table, _dev(table.table))
        t = self._up[id(table.table)][1]
        if table.kind in ("logits", "thresholds"):
            return PKG.table_policy(**{table.kind: t})
        rec = PKG.table_policy(**{table.kind: t}, epsilon=EPSILON[table.eps32])
        assert rec.epsilon_u32 == table.eps32
        return rec

    def run(self, variant, lay, key, ball_xy, goal_xy, acts):
        T, N = acts.shape
        env = PKG.LmazeVecEnv(N, variant=variant, layout=lay, device=DEV, seed=1, step_limit=X.STEP_LIMIT)
        state = dict(ball_xy=ball_xy, reward=np.full(N, -0.01, np.float32), done=np.zeros(N, np.uint8), step_count=np.zeros(N, np.int32))
        if goal_xy is not None:
            state["goal_xy"] = goal_xy
        env.set_state(**state)
        a = _dev(acts)
        reward, done, keys = [], [], []
        for t in range(T):
            keys.append(env.state_keys(key))
            _, r, d, _ = env.step(a[t], render=False, auto_reset=False)
            reward.append(r.clone())
            done.append(d.clone())
        return X.Rows(_np(torch.stack(reward)), _np(torch.stack(done)).astype(bool), np.ascontiguousarray(acts, dtype=np.int32),
                      _np(torch.stack(keys)), _np(env.state_keys(key)), int(env.host_state()["step_count"].max()))

    @staticmethod
    def _closed(env, out, key):
        reward_t, done_t, act_t, key_t = (_np(x) for x in out[3:7])
        return X.Rows(reward_t, done_t.astype(bool), act_t, key_t, _np(env.state_keys(key)), int(env.host_state()["step_count"].max()))

    def sample_rows(self, variant, lay, key, N, T, seed, limit, logits):
        env = PKG.LmazeVecEnv(N, variant=variant, layout=lay, device=DEV, seed=seed, step_limit=limit)
        env.reset()
        return self._closed(env, env.rollout_sample(T, logits=_dev(logits), key=key, auto_reset=True, trajectory=True), key)

    def policy_rows(self, variant, lay, key, N, T, seed, limit, policy=None, q=None, eps32=0):
        env = PKG.LmazeVecEnv(N, variant=variant, layout=lay, device=DEV, seed=seed, step_limit=limit)
        env.reset()
        table = dict(policy=_dev(policy)) if q is None else dict(q=_dev(q))
        return self._closed(env, env.rollout_policy(T, epsilon=EPSILON[eps32], key=key, auto_reset=True, trajectory=True, **table), key)

    def probs(self, key, act, table):
        return _np(PKG.action_probs(_dev(key), _dev(act), self.record(table)))

    def vtrace_table(self, rows, v, behaviour, target, gamma, lam, rho_bar, c_bar, key_t=None, key_tail=True):
        out = PKG.vtrace(_dev(rows.reward), _dev(rows.done), gamma, lam, values=_dev(v), key_t=_dev(rows.key if key_t is None else key_t),
                         key_tail=_dev(rows.tail) if key_tail else None, actions_t=_dev(rows.act), behaviour=self.record(behaviour),
                         target=self.record(target), rho_bar=rho_bar, c_bar=c_bar, ratios=True)
        return tuple(_np(x) for x in out)

    def vtrace_rows(self, reward, done, value_t, tail, rho_t, gamma, lam, rho_bar, c_bar):
        vs, pg, _ = PKG.vtrace(_dev(reward), _dev(done), gamma, lam, value_t=_dev(value_t), tail=_dev(tail), rho_t=_dev(rho_t),
                               rho_bar=rho_bar, c_bar=c_bar)
        return _np(vs), _np(pg)

    def evaluate(self, variant, lay, key, problems, table, gamma, sweeps, v_init=None):
        """env.evaluate() of the whole table -- every goal problem of key="goal" -- and then the rows of `problems`"""
        at = (variant, lay.tobytes())
        if at not in self._judge:
            self._judge[at] = PKG.LmazeVecEnv(1, variant=variant, layout=lay, device=DEV)
        S = lay.size
        rec = self.record(table)
        kw = {table.kind: rec.table if table.kind != "logits" else self._up[id(table.table)][1]}
        if table.kind in ("policy", "q"):
            kw["epsilon"] = EPSILON[table.eps32]
        got = self._judge[at].evaluate(key=key, gamma=gamma, sweeps=sweeps, tol=0.0, v_init=None if v_init is None else _dev(v_init), **kw)
        q, v, run = _np(got.q).reshape(-1, S, 4), _np(got.v).reshape(-1, S), np.atleast_1d(_np(got.sweeps_run))
        if variant == "v0" or isinstance(problems, str):
            return q, v, run
        who = [int(g) for g in problems]
        return q[who], v[who], run[who]


GPU = Gpu()


# ------------------------------------------------------------- A
@pytest.mark.parametrize("gamma", X.GAMMAS)
@pytest.mark.parametrize("pair", X.PAIRS)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_expectation_over_every_sequence_is_evaluate(variant, pair, gamma):
    """every spawnable start cell, T = 5, the table form: its 4-row block is a ragged block of 1 and a full one"""
    X.check_expectation(GPU, variant, pair, gamma, 5)


@pytest.mark.parametrize("gamma", X.GAMMAS)
@pytest.mark.parametrize("pair", X.PAIRS)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_expectation_from_one_cell_in_the_rows_form(variant, pair, gamma):
    """one start cell, T = 9 (262 144 envs), the rows form: its 8-row block is crossed"""
    X.check_expectation(GPU, variant, pair, gamma, 9, form="rows")


def test_mistakes_in_the_row_conventions_miss_the_expectation():
    X.check_discrimination(GPU)


# ------------------------------------------------------------- B
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_vtrace_of_sampled_rows_is_centred_on_the_critic(variant):
    X.check_sampled(GPU, variant)


# ------------------------------------------------------------- C
@pytest.mark.parametrize("how", ["policy", "q"])
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_rows_of_rollout_policy_carry_weight_under_the_table_that_ran(variant, how):
    X.check_recorded(GPU, variant, how)
