"""What test_gpu_offpolicy_vs_rollouts.py and its CPU twin share: the cases, the rows, the float64 foldings and every bound and
threshold of the three parts that tie action_probs() and vtrace() to the rows the envs write and to evaluate().  A check takes
an ENGINE -- where rows, probabilities, V-trace targets and evaluated tables come from: the library on a GPU
(test_gpu_offpolicy_vs_rollouts.Gpu) or the references alone (Host below: the C oracle's rows, offpolicy_ref, evaluate_ref)
-- and asserts the same thing of either, so a bound that holds here is shown to hold for the references before a GPU is
asked.  Importing it needs no GPU.

An engine has
    run(variant, lay, key, ball_xy, goal_xy, acts)             Rows of prescribed actions int32[T, N], no reset
    sample_rows(variant, lay, key, N, T, seed, limit, logits)  Rows of rollout_sample(logits=), auto_reset
    policy_rows(variant, lay, key, N, T, seed, limit, policy, q, eps32)   Rows of rollout_policy(policy= or q=), auto_reset
    probs(key, act, table)                                     action_probs(): float32 shaped like key
    vtrace_table(rows, v, behaviour, target, gamma, lam, rho_bar, c_bar, key_t=None, key_tail=True)   (vs, pg, rho)
    vtrace_rows(reward, done, value_t, tail, rho_t, gamma, lam, rho_bar, c_bar)                       (vs, pg)
    evaluate(variant, lay, key, problems, table, gamma, sweeps, v_init=None)   (q [P,S,4], v [P,S], sweeps_run [P]) of the
                                                               goal cells `problems` (None: v0's one problem; "all")
with numpy on both sides of every call."""
import collections
import functools
import importlib

import numpy as np
from scipy.stats import norm

import evaluate_ref as E
import helpers as H
import occupancy_rollout_ref as RR
import offpolicy_ref as R
import oracle_lib as O
import solve_ref as SR
import tabular_ref as TR

F = np.float32
U = RR.U
INF = float("inf")
STEP_LIMIT = 1000                # far above any step count a row reaches: only the terminal rule sets done
MARGIN = 100                     # test_offpolicy_cpu.py's: a wrong variant misses by more than MARGIN bounds
ALPHA = 1e-6                     # the project's (test_gpu_planning_vs_rollouts.ALPHA)
R_MAX = float(np.abs(np.array(SR.DEFAULT_REWARDS)).max())

Table = collections.namedtuple("Table", "kind table eps32")          # kind: thresholds, policy, q or logits (temperature 1)
Rows = collections.namedtuple("Rows", "reward done act key tail step_max")    # [T,N] x 4, int32[N], the largest step_count


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def next_keys(rows):
    return np.concatenate([rows.key[1:], rows.tail[None]])


def no_truncation(rows, what):
    """done only where the terminal rule paid the goal reward, and no step count near the limit"""
    assert rows.step_max < STEP_LIMIT - 1, what
    assert (bits(rows.reward[rows.done]) == bits(F(SR.DEFAULT_REWARDS[2]))).all(), (what, "a done row without the goal reward")


@functools.lru_cache(maxsize=None)
def _tables_module():
    return importlib.import_module("gym-lmaze_amd._tables")


def logits_thresholds(logits):
    """uint32[S, 4]: the library's own host-side conversion of a logits table (temperature 1), what rollout_sample(logits=),
    table_policy(logits=) and evaluate(logits=) read"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(logits))
    th = _tables_module().threshold_table(None, t, None, 1.0, len(logits), 4, t.device, "host")
    return th.view(torch.int32).numpy().view(np.uint32)


def greedy_bytes(q):
    """uint8[S]: greedy_table(q), the bytes rollout_policy(q=) runs -- a row with a NaN becomes 4, no move"""
    import torch
    return _tables_module().greedy_table(torch.from_numpy(np.ascontiguousarray(q, dtype=F))).numpy()


def grid_probs(engine, table, entries):
    """float64[entries, 4]: action_probs of every (key, move) pair"""
    key = np.repeat(np.arange(entries, dtype=np.int32), 4).reshape(entries, 4)
    act = np.tile(np.arange(4, dtype=np.int32), entries).reshape(entries, 4)
    return engine.probs(key, act, table).astype(np.float64)


# ------------------------------------------------------------- the references as an engine
class Host:
    """Rows from the C oracle (occupancy_rollout_ref.HostEnv), offpolicy_ref in the kernels' place, evaluate_ref in evaluate()'s"""
    name = "host"

    def __init__(self):
        self._thr = {}

    def _plain(self, table):
        if table.kind != "logits":
            return table
        if id(table.table) not in self._thr:
            self._thr[id(table.table)] = (table.table, logits_thresholds(table.table))
        return Table("thresholds", self._thr[id(table.table)][1], 0)

    def _weights(self, table, key, act):
        t = self._plain(table)
        return R.weights(t.kind, t.table, key, act, t.eps32)

    def run(self, variant, lay, key, ball_xy, goal_xy, acts):
        T, N = acts.shape
        env = RR.HostEnv(variant, lay, N, 1, STEP_LIMIT)
        env.place(ball_xy, goal_xy)
        reward, done, keys = np.zeros((T, N), F), np.zeros((T, N), bool), np.zeros((T, N), np.int32)
        for t in range(T):
            keys[t] = env.keys(key)
            a = np.ascontiguousarray(acts[t], dtype=np.int32)
            if env.v3:
                O.step_v3(env.p, env.lay, a, env.ball, env.goal, env.step_count, env.reward, env.done)
            else:
                O.step_v0(env.p, env.lay, a, env.ball, env.step_count, env.reward, env.done, env.goal_count)
            reward[t], done[t] = env.reward, env.done != 0
        return Rows(reward, done, np.ascontiguousarray(acts, dtype=np.int32), keys, env.keys(key), int(env.step_count.max()))

    @staticmethod
    def _closed(env, out, key):
        reward, done, act, keys, nxt = out
        return Rows(reward, done, act, keys, np.ascontiguousarray(nxt[-1]), int(env.step_count.max()))

    def sample_rows(self, variant, lay, key, N, T, seed, limit, logits):
        env = RR.HostEnv(variant, lay, N, seed, limit)
        env.reset()
        return self._closed(env, env.rollout(T, key, True, thresholds=logits_thresholds(logits)), key)

    def policy_rows(self, variant, lay, key, N, T, seed, limit, policy=None, q=None, eps32=0):
        env = RR.HostEnv(variant, lay, N, seed, limit)
        env.reset()
        table = policy if q is None else greedy_bytes(q)
        return self._closed(env, env.rollout(T, key, True, policy=table, eps32=eps32), key)

    def probs(self, key, act, table):
        return R.probs(self._weights(table, key, act))

    def vtrace_table(self, rows, v, behaviour, target, gamma, lam, rho_bar, c_bar, key_t=None, key_tail=True):
        key = rows.key if key_t is None else key_t
        ratio = R.ratios(self._weights(target, key, rows.act), self._weights(behaviour, key, rows.act))
        vs, pg = R.vtrace_numpy(rows.reward, rows.done, TR.table_values(v, key), TR.table_values(v, rows.tail) if key_tail else None,
                                ratio, gamma, lam, rho_bar, c_bar)
        return vs, pg, ratio

    def vtrace_rows(self, reward, done, value_t, tail, rho_t, gamma, lam, rho_bar, c_bar):
        return R.vtrace_numpy(reward, done, value_t, tail, rho_t, gamma, lam, rho_bar, c_bar)

    def evaluate(self, variant, lay, key, problems, table, gamma, sweeps, v_init=None):
        G = lay.shape[0]
        S = G * G
        t = self._plain(table)
        if variant == "v0":
            cells, goals = [0], None
        else:
            cells = list(range(S)) if isinstance(problems, str) else [int(g) for g in problems]
            goals = [(g // G, g % G) for g in cells]
        width = (S,) if t.kind == "policy" else (S, 4)
        kw = {t.kind: np.stack([np.asarray(t.table).reshape((-1,) + width)[c] for c in cells])}
        if t.kind != "thresholds":
            kw["epsilon_u32"] = t.eps32
        v0 = None if v_init is None else np.stack([np.asarray(v_init, dtype=F).reshape(-1, S)[c] for c in cells])
        got = E.evaluate_many(variant, lay, goals, gamma, sweeps, v_init=v0, **kw)
        return got.q, got.v, np.asarray(got.sweeps_run)


# ------------------------------------------------------------- A: the exact expectation over every action sequence
A_GRID, A_MAZE_SEED, A_GOAL_SEED, A_V_SEED = 7, 3, 17, 3
CLIPS = ((0.95, 1.0, 1.0), (0.95, 2.0, 0.5))
PAIRS = ("min_law", "eps", "explore")
GAMMAS = (0.9, 1.0)
ACase = collections.namedtuple("ACase", "variant key lay G S entries goals cells base wall")


@functools.lru_cache(maxsize=None)
def a_case(variant):
    """One 7x7 maze of helpers.bordered_random_layouts with its 'S' cell made blank: v0 key="ball" (one problem, 49 keys),
    v3 key="goal" (V3_GOALS goal problems, 7^4 keys).  cells[j]: the spawnable cells of problem j; base[j]: its first key."""
    lay = H.bordered_random_layouts(1, A_GRID, A_MAZE_SEED)[0].copy()
    lay[lay == ord("S")] = ord("B")
    G = A_GRID
    S = G * G
    assert (lay[1:-1, 1:-1] == ord("W")).any() and not (lay == ord("S")).any() and (lay == ord("X")).sum() == 1
    wall = lay.reshape(-1) == ord("W")
    if variant == "v0":
        assert not SR.extract_model("v0", lay, None).sticky.any()
        return ACase("v0", "ball", lay, G, S, S, None, (RR.spawn_cells(lay, "v0"),), (0,), wall)
    goals = RR.v3_goals(lay, A_GOAL_SEED)
    for g in goals:
        assert not SR.extract_model("v3", lay, (g // G, g % G)).sticky.any()
    return ACase("v3", "goal", lay, G, S, S * S, goals, tuple(RR.spawn_cells(lay, "v3", g) for g in goals),
                 tuple(int(g) * S for g in goals), wall)


def value_table(case, seed=A_V_SEED):
    """An arbitrary critic: randn * 10 in float32, 0 on wall cells.  Not a fixed point of anything."""
    v = (np.random.RandomState(seed).randn(case.entries) * 10).astype(F)
    v[np.tile(case.wall, case.entries // case.S)] = 0.0
    return v


@functools.lru_cache(maxsize=None)
def table_pair(variant, name):
    """(behaviour, target) of a_case(variant)"""
    n = a_case(variant).entries
    rs = np.random.RandomState(11)
    by = rs.randint(0, 4, n).astype(np.uint8)
    if name == "min_law":
        return Table("thresholds", R.min_law_table(n, 1), 0), Table("thresholds", R.min_law_table(n, 2), 0)
    if name == "eps":
        return Table("policy", by, R.EPSILONS[1]), Table("q", (rs.randn(n, 4) * 3).astype(F), R.EPSILONS[1])
    assert name == "explore"             # an exploring rollout under a greedy learner: most ratios are exactly 0
    return Table("policy", by, R.EPSILONS[2]), Table("policy", by, 0)


_A_ROWS = {}


def a_rows(engine, variant, T, one_cell=False):
    """(rows, problem int[C], cell int[C]) -- one env for every action sequence of length T from every start: env index
    start * 4^T + sequence, the sequence's first action its most significant digit.  one_cell: problem 0's middle spawnable
    cell alone.  Made once per engine and read only."""
    at = (engine.name, variant, T, one_cell)
    if at not in _A_ROWS:
        case = a_case(variant)
        G, n = case.G, 4 ** T
        prob = np.concatenate([np.full(len(c), j) for j, c in enumerate(case.cells)])
        cell = np.concatenate(case.cells)
        if one_cell:
            prob, cell = prob[:1], case.cells[0][len(case.cells[0]) // 2:][:1]
        ball = np.repeat(np.stack([cell // G, cell % G], 1), n, axis=0).astype(np.int32)
        goal = None
        if case.goals is not None:
            g = case.goals[prob]
            goal = np.repeat(np.stack([g // G, g % G], 1), n, axis=0).astype(np.int32)
        seq = np.arange(n)
        acts = np.stack([np.tile((seq // 4 ** (T - 1 - t)) % 4, len(cell)) for t in range(T)]).astype(np.int32)
        rows = engine.run(variant, case.lay, case.key, ball, goal, acts)
        no_truncation(rows, (variant, T))
        start = np.asarray(case.base)[prob] + cell
        assert (rows.key[0].reshape(len(cell), n) == start[:, None]).all() and rows.done.any() and not rows.done[0].all()
        _A_ROWS[at] = (rows, prob, cell)
    return _A_ROWS[at]


def fold(p, x, C, T):
    """float64[C, 4]: sum over the actions behind the first of prod_t p_t x, times p_0 -- back to front over the sequence
    axis.  p float[T, C * 4^T], x float[C * 4^T]."""
    x = np.asarray(x, dtype=np.float64).reshape(C, -1)
    for t in range(T - 1, -1, -1):
        w = np.asarray(p[t], dtype=np.float64).reshape(C, 4 ** t, 4, 4 ** (T - 1 - t))
        assert (w == w[..., :1]).all()                     # the probability of row t does not know the later actions
        x = x.reshape(C, 4 ** t, 4) * w[..., 0]
        if t:
            x = x.sum(-1)
    return x.reshape(C, 4)


def reward_table(entries, rows):
    """float64[entries, 4]: the reward the rows show for a pair (NaN where none does); a pair always showed the same one"""
    idx = rows.key.astype(np.int64).reshape(-1) * 4 + rows.act.reshape(-1)
    r = rows.reward.astype(np.float64).reshape(-1)
    lo, hi = np.full(entries * 4, np.inf), np.full(entries * 4, -np.inf)
    np.minimum.at(lo, idx, r)
    np.maximum.at(hi, idx, r)
    seen = hi >= lo
    assert (lo == hi)[seen].all(), "a pair paid two different rewards"
    return np.where(seen, hi, np.nan).reshape(entries, 4)


def clipped_trace(case, rows, v, mu, pi, gamma, lam, rho_bar, c_bar, T):
    """float64[entries]: W_T, W_0 = 0, W_k(s) = sum_a mu(a|s) [rho delta + (1 - done) gamma c W_(k-1)(s')] over the successor
    table the rows themselves show.  A pair no row shows is NaN, and so is every key whose W_T would need it."""
    S, n = case.S, case.entries
    nxt, done, seen = RR.successors(n, S, [(rows.reward, rows.done, rows.act, rows.key, next_keys(rows))])
    r = reward_table(n, rows)
    g, lm = float(F(gamma)), float(F(lam))
    nkey = np.where(nxt >= 0, (np.arange(n)[:, None] // S) * S + nxt, 0)
    with np.errstate(all="ignore"):
        ratio = np.where(mu > 0, pi / np.where(mu > 0, mu, 1.0), 0.0)
    rho, c = np.minimum(ratio, rho_bar), lm * np.minimum(ratio, c_bar)
    v64 = v.astype(np.float64)
    delta = np.where(done, r - v64[:, None], r + g * v64[nkey] - v64[:, None])
    delta = np.where(seen, delta, np.nan)
    W = np.zeros(n)
    for _ in range(T):
        W = (mu * (rho * delta + np.where(done, 0.0, g * c * W[nkey]))).sum(1)
    return W


def a_bound(T, v, gamma, sweeps):
    """The bound of check_expectation(), derived there"""
    mag = (T + 1) * (R_MAX + (1 + float(F(gamma))) * float(np.abs(v).max()))
    return RR.rel(14 * T + 1 + T + 9 * sweeps) * mag


def check_expectation(engine, variant, pair, gamma, T, form="table", wrong=False):
    """The envs are deterministic given their actions, so the expectation of the V-trace target under the behaviour table is a
    finite sum: E_vs(s) = sum_seq prod_t p_t vs[0] and E_pg(s, a) = sum_(seq: a_0 = a) prod_t p_t pg[0], p = action_probs()
    of the behaviour table on the rows, vs / pg / rho = vtrace() on the rows, folded in float64.  For ANY critic v:
    (1) lam = 1, rho_bar = c_bar = inf:  E_vs(s) = ((T^pi)^T v)(s), which is evaluate(target, gamma, sweeps=T, tol=0,
        v_init=v).v, and E_pg(s, a) = pi(a|s) (q_T(s, a) - v(s)) with that call's q and pi the target's action_probs;
    (2) at CLIPS:  E_vs(s) - v(s) = W_T(s) of clipped_trace(), in float64 over the successors the rows show.
    form "table": values=, key_t=, key_tail=, behaviour=, target=; form "rows": value_t, tail and rho_t = fl(p_target /
    p_behaviour) gathered here.  Rows behind an env's first done row do not reach vs[0]; the fold sums their probabilities.

    The bound.  U = 2^-24; MAG0 = |r|_max + (1 + gamma) |v|_max bounds every |r + gamma v' - v|, and MAG = (T + 1) MAG0.
    A row of the walk rounds 8 times (c, boot, tg, td, delta, gc, trace, acc) and its ratio, which enters rho and c, 3 times
    (two conversions, a division): 14 per row, each of relative size U on a quantity no larger than the |acc| behind it, and
    vs = acc + v rounds once more.  Per sequence |acc| can reach prod ratio * T MAG0, but the fold weighs a sequence by
    prod mu, and mu * min(ratio, bar) <= mu * ratio = pi: an error made at row t reaches E_vs weighted by a product of pi's
    (those before t) and mu's (those after), which sum to 1, times the sum over the rows behind t of |rho (r + gamma v' - v)|
    under the same weights, <= T MAG0.  So the walk costs (14 T + 1) U MAG.  Each p_t = fl(w) 2^-34 is one rounding of an
    exact probability -- the four of a key sum to 1 within 4 U, which is all the rows behind a done row contribute -- so the
    fold costs T U |vs[0]| <= T U MAG in expectation.  A sweep of evaluate() rounds 9 times (3 in a probability, 2 in
    r + gamma v', a product, 3 sums) on quantities no larger than k |r|_max + |v|_max <= MAG, and a sweep is a contraction:
    9 T U MAG for T sweeps (none in (2), whose reference is float64 throughout).  pg makes no more roundings than vs and
    |pi| <= 1: the same bound.  With rel(n) = n U / (1 - n U):  err <= rel(24 T + 1) MAG in (1), rel(15 T + 1) MAG in (2).

    wrong: also the misses against (1) of four mistakes -- ratios omitted, the tables exchanged, key_tail dropped, key_t
    replaced by the next keys (table form).  Returns {name: (err or miss, bound)}."""
    case = a_case(variant)
    one = form == "rows"
    rows, prob, cell = a_rows(engine, variant, T, one_cell=one)
    C, S = len(cell), case.S
    start = np.asarray(case.base)[prob] + cell
    v = value_table(case)
    b, t = table_pair(variant, pair)
    what = "%s %s %s gamma=%g T=%d %s" % (engine.name, variant, pair, gamma, T, form)
    p = engine.probs(rows.key, rows.act, b)
    assert (p > 0).all(), what                                          # the behaviour table can have produced every row
    mu, pi = grid_probs(engine, b, case.entries), grid_probs(engine, t, case.entries)
    assert (np.abs(mu.sum(1) - 1) <= 4 * U).all() and (np.abs(pi.sum(1) - 1) <= 4 * U).all()
    if one:
        pt = engine.probs(rows.key, rows.act, t)
        rho_t = (pt / p).astype(F)
        value_t, tail = TR.table_values(v, rows.key), TR.table_values(v, rows.tail)

    def walk(lam, rho_bar, c_bar, b=b, t=t, key_t=None, key_tail=True):
        if one:
            return engine.vtrace_rows(rows.reward, rows.done, value_t, tail, rho_t, gamma, lam, rho_bar, c_bar)
        return engine.vtrace_table(rows, v, b, t, gamma, lam, rho_bar, c_bar, key_t=key_t, key_tail=key_tail)[:2]

    out = {}
    # (1)
    goals = None if case.goals is None else sorted(set(int(g) for g in case.goals[prob]))
    q, vT, run = engine.evaluate(variant, case.lay, case.key, goals, t, gamma, T, v_init=v)
    assert (np.asarray(run) == T).all(), (what, run)
    which = np.zeros(C, np.int64) if goals is None else np.searchsorted(goals, case.goals[prob])
    want_vs = vT.astype(np.float64)[which, cell]
    want_pg = pi[start] * (q.astype(np.float64)[which, cell] - v.astype(np.float64)[start][:, None])
    vs, pg = walk(1.0, INF, INF)
    bound = a_bound(T, v, gamma, T)
    err_vs = float(np.abs(fold(p, vs[0], C, T).sum(1) - want_vs).max())
    err_pg = float(np.abs(fold(p, pg[0], C, T) - want_pg).max())
    out["vs"], out["pg"] = (err_vs, bound), (err_pg, bound)
    # (2)
    for lam, rho_bar, c_bar in CLIPS:
        W = clipped_trace(case, rows, v, mu, pi, gamma, lam, rho_bar, c_bar, T)[start]
        assert np.isfinite(W).all(), (what, "a start whose trace needs a pair no row shows")
        vs, _ = walk(lam, rho_bar, c_bar)
        err = float(np.abs(fold(p, vs[0], C, T).sum(1) - v.astype(np.float64)[start] - W).max())
        out["clip %g/%g" % (rho_bar, c_bar)] = (err, a_bound(T, v, gamma, 0))
    for name, (err, bd) in out.items():
        print("%s: %s err %.3g bound %.3g" % (what, name, err, bd))
    for name, (err, bd) in out.items():
        assert err <= bd, (what, name, err, bd)
    if wrong:
        assert not one
        variants = (("no ratios", dict(t=b)), ("exchanged", dict(b=t, t=b)), ("no key_tail", dict(key_tail=False)),
                    ("shifted keys", dict(key_t=next_keys(rows))))
        for name, kw in variants:
            vs, _ = walk(1.0, INF, INF, **kw)
            with np.errstate(all="ignore"):
                miss = float(np.nanmax(np.abs(fold(p, vs[0], C, T).sum(1) - want_vs)))
            print("%s: %s miss %.3g = %.3g bounds" % (what, name, miss, miss / bound))
            out[name] = (miss, bound)
    return out


WRONG = ("no ratios", "exchanged", "no key_tail", "shifted keys")


def check_discrimination(engine, T=5):
    """Each of the four mistakes misses identity (1) by more than MARGIN bounds on both min_law cases at gamma = 0.9"""
    for variant in ("v0", "v3"):
        got = check_expectation(engine, variant, "min_law", 0.9, T, wrong=True)
        for name in WRONG:
            miss, bound = got[name]
            assert miss > MARGIN * bound, (variant, name, miss, bound)


# ------------------------------------------------------------- B: sampled rows with auto-resets
B_N, B_T, B_GRID, B_GAMMA, B_LAM, B_SWEEPS = 262144, 16, 11, 0.9, 0.95, 4096
B_STEPS = (0, 7, 15)
B_MIN = 256                      # a bin (t, cell) counts from this many envs on
# The target's logits are the behaviour's + B_SPREAD * randn, the randn table [S, 4] repeated for every goal problem.  At 0.5,
# and with a table drawn per goal problem at 1.0, the two mistakes reach 9 - 15 and 7 - 10 on the v3 case against the 17.6 asked
# for (a bin holds a ball cell under some 80 goals, and what a mistake adds to the mean changes sign from goal to goal), so
# the spread is 1.0 and the goals share the table; v0 reaches 59 - 98 at 0.5 already.
B_SPREAD = 1.0
# About one random problem in 150 ends in a two-cycle of the last bit and not at the exact stop; 8 is the first
# logits seed at which evaluate_ref reaches the exact stop in all 121 goal problems of the v3 case (and in v0's one).
B_SEED, B_ENV_SEED = 8, 23
B_FACTOR = 3                     # a mistake must exceed the threshold by this factor


def room(G=B_GRID):
    """The 11x11 open room of test_gpu_offpolicy's real-rollout test, as codes"""
    pkg = importlib.import_module("gym-lmaze_amd")
    return pkg.layouts.to_codes(pkg.layouts.open_room(G, (G // 2, G // 2))).copy()


def z_scores(x, cell, S, what):
    """Per bin (t, cell) of at least B_MIN envs z = mean sqrt(n) / sd.  x, cell: [len(B_STEPS), N].  Returns (the largest |z|,
    bins, (t, cell, n, z) of the worst); asserts that the bins left out hold at most 1 % of the rows of their t."""
    worst, bins = (None, None, 0, 0.0), 0
    for j, t in enumerate(B_STEPS):
        n = np.bincount(cell[j], minlength=S)
        s1 = np.bincount(cell[j], weights=x[j], minlength=S)
        s2 = np.bincount(cell[j], weights=x[j] * x[j], minlength=S)
        use = n >= B_MIN
        assert n[~use].sum() <= 0.01 * n.sum(), (what, t, int(n[~use].sum()))
        m = s1[use] / n[use]
        sd = np.sqrt((s2[use] - n[use] * m * m) / (n[use] - 1))
        assert (sd > 0).all(), what
        z = m * np.sqrt(n[use]) / sd
        bins += int(use.sum())
        k = int(np.abs(z).argmax())
        if abs(z[k]) > abs(worst[3]):
            worst = (t, int(np.flatnonzero(use)[k]), int(n[use][k]), float(z[k]))
    return abs(worst[3]), bins, worst


def check_sampled(engine, variant, spread=B_SPREAD):
    """N = 262 144 envs, T = 16, rollout_sample(logits=la) with auto-resets on the open room; the target is lb = la + spread *
    randn (spread = B_SPREAD = 1.0, see there), the critic v = evaluate(logits=lb, gamma=0.9).v at its exact stop, vs = vtrace(lam=0.95, rho_bar=inf, c_bar=1) in
    the table form.  v is the target's value, so E[rho (r + gamma v(s') - v(s)) | s] = 0 on every row, a done row cuts the
    trace where the env was reset, and E[vs[t] - v(key_t[t]) | key_t[t]] = 0: at t = 0, at t = 7 behind many auto-resets, and
    at t = 15, the row bootstrapped from key_tail = state_keys().  The envs are independent, so per bin (t, ball cell) with at
    least 256 envs z = mean sqrt(n) / sd is close to a standard normal, and max |z| <= norm.isf(ALPHA / (2 bins)).  The normal
    tail is an approximation (a t-like statistic of >= 256 bounded terms; the goal reward makes them skewed), which is why the
    threshold sits at ALPHA = 1e-6 and the mistakes below must clear it B_FACTOR times.  The rows are a function of the seed:
    the test cannot flake.
    v0 runs on the room with its 'S' cell made blank.  The two pairs that step onto an 'S' are refused by v0's step (the ball
    stays, the reward row repeats) while evaluate() drops them and renormalises, so there the critic is not the value of the
    rows' process and the identity is not claimed: on the room as it ships the references alone give z = -6.47 at t = 15 on
    cell (2, 1), beside the 'S', where few episodes end and the standard error is a hundredth.  v3 refuses no pair.
    Mistakes: ratios omitted, and the tables exchanged, each give max |z| above B_FACTOR thresholds.
    Returns (max |z|, threshold, {mistake: max |z|})."""
    key = "ball" if variant == "v0" else "goal"
    lay = room()
    G = lay.shape[0]
    S = G * G
    if variant == "v0":
        lay[lay == ord("S")] = ord("B")
    assert not SR.extract_model(variant, lay, (1, 1) if variant == "v3" else None).sticky.any()
    entries = S if key == "ball" else S * S
    rs = np.random.RandomState(B_SEED)
    la = rs.randn(entries, 4).astype(F)
    lb = (la + F(spread) * np.tile(rs.randn(S, 4), (entries // S, 1))).astype(F)
    old, new = Table("logits", la, 0), Table("logits", lb, 0)
    what = "%s %s sampled" % (engine.name, variant)
    rows = engine.sample_rows(variant, lay, key, B_N, B_T, B_ENV_SEED, STEP_LIMIT, la)
    no_truncation(rows, what)
    resets = int(rows.done[:B_STEPS[1]].sum())
    assert resets > B_N // 100 and ((rows.key >= 0) & (rows.key < entries)).all()
    _, v, run = engine.evaluate(variant, lay, key, "all", new, B_GAMMA, B_SWEEPS)
    assert (np.asarray(run) < B_SWEEPS).all(), (what, "a problem that did not reach the exact stop", np.asarray(run).max())
    v = np.ascontiguousarray(v, dtype=F).reshape(-1)
    assert v.shape == (entries,)
    steps = list(B_STEPS)
    cell = rows.key[steps].astype(np.int64) % S
    own = v.astype(np.float64)[rows.key[steps]]

    def stat(b, t, name):
        vs, _, rho = engine.vtrace_table(rows, v, b, t, B_GAMMA, B_LAM, INF, 1.0)
        z, bins, worst = z_scores(vs[steps].astype(np.float64) - own, cell, S, what)
        print("%s: %s max|z| %.3f bins %d worst (t, cell, n, z) %s largest ratio %.4g" % (what, name, z, bins, worst, float(rho.max())))
        return z, bins

    z, bins = stat(old, new, "v-trace")
    threshold = float(norm.isf(ALPHA / (2 * bins)))
    print("%s: threshold %.3f resets before t=7 %d spread %g" % (what, threshold, resets, spread))
    assert z <= threshold, (what, z, threshold)
    wrong = {"no ratios": stat(old, old, "no ratios")[0], "exchanged": stat(new, old, "exchanged")[0]}
    for name, zw in wrong.items():
        assert zw >= B_FACTOR * threshold, (what, name, zw, threshold)
    return z, threshold, wrong


# ------------------------------------------------------------- C: every recorded row has weight under the table that ran
C_N, C_T, C_LIMIT = 4096, 32, 20


def check_recorded(engine, variant, how):
    """rollout_policy() on the open room, 4 096 envs, T = 32, epsilon = 0.1.  how "policy": bytes, one in ten above 3 (the
    rollout records such a byte as the action); how "q": rollout_policy(q=), named as table_policy(policy=greedy_table(q)) --
    rows with a NaN become byte 4.  Every recorded (key, action) has positive weight under that table, by offpolicy_ref's
    integers and by action_probs(); the table against itself has ratio exactly 1 on every row, and its target is gae()'s."""
    key = "ball" if variant == "v0" else "goal"
    lay = room()
    S = lay.size
    entries = S if key == "ball" else S * S
    rs = np.random.RandomState(31)
    eps32 = R.EPSILONS[1]
    if how == "policy":
        by = np.where(rs.rand(entries) < 0.9, rs.randint(0, 4, entries), rs.choice([4, 7, 200, 255], entries)).astype(np.uint8)
        rows = engine.policy_rows(variant, lay, key, C_N, C_T, B_ENV_SEED, C_LIMIT, policy=by, eps32=eps32)
    else:
        q = (rs.randn(entries, 4) * 3).astype(F)
        q[rs.rand(entries) < 0.05, 2] = np.nan
        q[rs.rand(entries) < 0.05] = 1.0                                # ties: the first maximum
        by = greedy_bytes(q)
        assert (by == 4).any() and by.max() == 4
        rows = engine.policy_rows(variant, lay, key, C_N, C_T, B_ENV_SEED, C_LIMIT, q=q, eps32=eps32)
    table = Table("policy", by, eps32)
    what = "%s %s rollout_policy(%s=)" % (engine.name, variant, how)
    assert rows.done.any() and not rows.done.all() and ((rows.key >= 0) & (rows.key < entries)).all()
    w = R.weights("policy", by, rows.key, rows.act, eps32)
    assert (w > 0).all(), (what, "rows the table cannot have recorded", int((w == 0).sum()))
    above = rows.act > 3
    assert above.any() and (rows.act[above] == by[rows.key[above]]).all() and (rows.act[~above] >= 0).all(), what
    p = engine.probs(rows.key, rows.act, table)
    assert (bits(p) == bits(R.probs(w))).all() and (p > 0).all(), what
    v = (rs.randn(entries) * 10).astype(F)
    vs, _, rho = engine.vtrace_table(rows, v, table, table, 0.9, 0.95, INF, INF)
    assert (rho == 1).all(), (what, "a table against itself")
    _, tgt = TR.gae_numpy(rows.reward, rows.done, TR.table_values(v, rows.key), TR.table_values(v, rows.tail), 0.9, 0.95)
    assert (bits(vs) == bits(tgt)).all(), what
    print("%s: rows %d, recorded bytes above 3 %d, least weight %d / 2^34" % (what, w.size, int(above.sum()), int(w.min())))
