"""What test_gpu_occupancy_vs_rollouts.py and its CPU twin share: the successor table the rows of closed-loop rollouts show, the
flow identity of an occupancy over that table, the count of running envs per cell and step against the law occupancy sums, and
a host env -- the C oracle's reset and step under closed_loop_ref's draws, epoch for epoch as LmazeVecEnv spends them -- that
makes such rows without a GPU.  Importing it needs no GPU."""
import numpy as np
from scipy.stats import binom

import occupancy_ref as OR
import oracle_lib as O
from closed_loop_ref import explore_draw, sample_action
from env_table_ref import epsilon_greedy

U = 2.0 ** -24
ROUNDINGS = 11                   # test_occupancy_cpu.py's count of roundings per cell and sweep
V3_GOALS = 3                     # the goal problems of the v3 case that are covered and checked


def rel(n):
    return n * U / (1 - n * U)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------- where the cases put their envs
def spawn_cells(lay, variant, goal=None):
    """The cells reset() accepts, ascending: interior, not 'W', v0 not 'X', v3 not the goal cell"""
    G = lay.shape[-1]
    ok = lay != ord("W")
    if variant == "v0":
        ok &= lay != ord("X")
    ok[0, :] = ok[-1, :] = ok[:, 0] = ok[:, -1] = False
    ok = ok.reshape(-1).copy()
    if goal is not None:
        ok[goal] = False
    return np.flatnonzero(ok)


def v3_goals(lay, seed):
    """The goal cells of the V3_GOALS problems of the v3 case that are covered and checked"""
    return np.random.RandomState(seed).choice(spawn_cells(lay, "v3"), V3_GOALS, replace=False)


def v3_placement(lay, N, goals, seed):
    """(ball_xy int32[N,2], goal_xy int32[N,2]): env i gets goal i mod V3_GOALS and a ball on a cell its reset would accept, so
    that N / V3_GOALS envs walk each of the chosen problems"""
    rs = np.random.RandomState(seed)
    G = lay.shape[-1]
    gi = np.arange(N) % V3_GOALS
    ball = np.zeros(N, np.int64)
    for j, g in enumerate(goals):
        who = np.flatnonzero(gi == j)
        ball[who] = rs.choice(spawn_cells(lay, "v3", g), len(who))
    g = goals[gi]
    return np.stack([ball // G, ball % G], 1).astype(np.int32), np.stack([g // G, g % G], 1).astype(np.int32)


def v3_cover_placement(lay, N, goals):
    """(ball_xy, goal_xy): under every chosen goal one env on every interior cell that is not a wall, the goal cell among them;
    the envs left over as env 0"""
    G = lay.shape[-1]
    cells = spawn_cells(lay, "v3")
    ball, goal = np.tile(cells, len(goals)), np.repeat(goals, len(cells))
    assert len(ball) <= N
    ball, goal = np.resize(np.r_[ball, np.full(N - len(ball), ball[0])], N), np.r_[goal, np.full(N - len(goal), goal[0])]
    return np.stack([ball // G, ball % G], 1).astype(np.int32), np.stack([goal // G, goal % G], 1).astype(np.int32)


def per_env_placements(lays):
    """The per-env case: int32[K, N, 2], placement k puts env i's ball on its k-th spawnable cell (mod their number); K is the
    most any maze has, so every spawnable cell of every maze ('S' cells are among them) starts a step"""
    N, G = lays.shape[0], lays.shape[-1]
    cells = [spawn_cells(lays[i], "v0") for i in range(N)]
    K = max(len(c) for c in cells)
    at = np.stack([c[np.arange(K) % len(c)] for c in cells], 1)          # [K, N]
    return np.stack([at // G, at % G], 2).astype(np.int32)


def eps_u32(epsilon):
    return min(int(float(epsilon) * 4294967296.0), 4294967295)


def case_rows(ad, variant, layouts, key, N, lay, entries, thr, pol, T, epsilon):
    """The rows of one case of (a) from an adapter ad -- place(ball_xy, goal_xy=None), sample(T, thr, key) and
    greedy(T, pol, epsilon, key), both with auto_reset and returning rows_of()'s tuple.  First the two rollouts whose laws are
    checked.  On the shared v0 maze, where the reset spreads 8 192 envs over some 60 cells, they see every pair.  Elsewhere
    a problem has too few envs for that (one, on the per-env mazes; on v3 key="goal" 324 goal problems share the envs), so the
    v3 envs are first given V3_GOALS goals, the problems that are checked, and every pair is then seen by construction: one step
    of a table that holds one action everywhere, at epsilon = 0, from every cell in turn, for each of the four actions.  A
    transition does not depend on the table that chose the action.  Returns (rows, the goal cells or None)."""
    goals = None
    if variant == "v3":
        goals = v3_goals(lay, 17)
        ad.place(*v3_placement(lay, N, goals, 18))
    rows = [ad.sample(T, thr, key), ad.greedy(T, pol, epsilon, key)]
    places = []
    if variant == "v3":
        places = [v3_cover_placement(lay, N, goals)]
    if layouts == "per_env":
        places = [(ball, None) for ball in per_env_placements(lay)]
    for a in range(4):
        one = np.full(entries, a, np.uint8)
        for ball, goal in places:
            ad.place(ball, goal)
            rows.append(ad.greedy(1, one, 0.0, key))
    return rows, goals


def check_flows(w, key, N, rows, goals, start, gamma, tables, what):
    """flow_identity() on every problem of a case (key="goal": on the V3_GOALS goal problems) for each of tables = [(name,
    p float32[entries,4], d float32[entries] or None, d_sa float32[entries,4] or None)]; start float32[problems, S].
    Returns the pairs covered, summed over the problems."""
    S, G = w["S"], w["G"]
    nxt, done, seen = successors(w["entries"], S, rows)
    problems = [0] if key == "ball" else ([int(g) for g in goals] if key == "goal" else list(range(N)))
    pairs = 0
    for name, p, d, d_sa in tables:
        pairs = 0
        for pr in problems:
            sl = slice(pr * S, (pr + 1) * S)
            pairs += flow_identity(G, nxt[sl], done[sl], seen[sl], w["sticky"][sl], w["wall"][sl], p[sl], start[pr], gamma,
                                   None if d is None else d[sl], None if d_sa is None else d_sa[sl], "%s %s problem %d" % (what, name, pr))
    print(what, "problems", len(problems), "pairs covered", pairs, "rows", sum(r[1].size for r in rows), "pairs seen", int(seen.sum()))
    return pairs


# ------------------------------------------------------------- the successor table the rows show
def successors(entries, S, rows_list):
    """(nxt int64[entries,4], done bool[entries,4], seen bool[entries,4]) from rows (reward, done, action, key, next key) of
    any number of rollouts: nxt is the CELL a seen pair led to on the rows that did not set done (-1 where there is none).
    Asserted: a pair always gave the same done flag, and without done the same next key, in the key's own problem."""
    big = np.int64(1) << 40
    lo, hi = np.full(entries * 4, big), np.full(entries * 4, -1, np.int64)
    dlo, dhi = np.full(entries * 4, 2, np.int8), np.full(entries * 4, -1, np.int8)
    for _, done_t, act_t, key_t, next_t in rows_list:
        assert ((act_t >= 0) & (act_t <= 3)).all() and ((key_t >= 0) & (key_t < entries)).all()
        idx = key_t.astype(np.int64).reshape(-1) * 4 + act_t.reshape(-1)
        d = done_t.reshape(-1).astype(np.int8)
        np.minimum.at(dlo, idx, d)
        np.maximum.at(dhi, idx, d)
        live = d == 0
        k, n = key_t.reshape(-1)[live].astype(np.int64), next_t.reshape(-1)[live].astype(np.int64)
        assert (k // S == n // S).all(), "a running episode changed its problem"
        np.minimum.at(lo, idx[live], n)
        np.maximum.at(hi, idx[live], n)
    seen = dhi >= 0
    assert (dlo == dhi)[seen].all(), "a pair set done on one row and not on another"
    moving = seen & (dhi == 0)
    assert (lo == hi)[moving].all(), "a pair led to two different keys"
    nxt = np.where(moving, hi % S, -1)
    return nxt.reshape(entries, 4), (dhi == 1).reshape(entries, 4), seen.reshape(entries, 4)


def flow_identity(G, nxt, done, seen, sticky, wall, p, start, gamma, d=None, d_sa=None, what=""):
    """One problem.  nxt, done, seen [S,4]: what the rows show; sticky, wall: the model's; p float32[S,4]: the probabilities of
    the law that ran; start float32[S]; d float32[S], d_sa float32[S,4]: the occupancy under test (None: coverage only).
    The cells that count are those with start mass and those a row stood on or led to.  Coverage, a condition: every action of
    every such cell was seen.  Then, with win / src / wself gathered from the observed successors (a pair flows when it is
    usable and was never seen with done), one sweep of occupancy_ref applied to d gives d back in every bit, d is 0 on every
    other cell, and d_sa = fl(d p).  Returns the number of pairs covered."""
    S = G * G
    cells = np.arange(S)
    reached = seen.any(1)
    reached[nxt[nxt >= 0]] = True
    count = reached | (np.asarray(start) > 0)
    assert not (count & wall).any(), what
    missing = count[:, None] & ~seen
    assert not missing.any(), (what, "pairs not covered", int(missing.sum()), np.argwhere(missing)[:8].tolist())
    # v0's excluded pairs: the step refuses them -- the key did not move and done was not set
    st = sticky & seen
    assert not (st & done).any() and (nxt[st] == np.nonzero(st)[0]).all(), what
    if d is None:
        return int(count.sum()) * 4
    fl = seen & count[:, None] & ~sticky & ~done & ~wall[:, None]
    table = np.where(fl, nxt, cells[:, None])
    win, src, wself = OR.gather_successors(G, table, fl, wall, p)
    assert (bits(d)[~count] == 0).all(), (what, "mass on a cell no row reached", np.flatnonzero(bits(d) * ~count)[:8].tolist())
    again = OR.sweep(win, src, wself, wall, np.where(wall, np.float32(0), start).astype(np.float32), gamma, np.ascontiguousarray(d, np.float32))
    bad = bits(again) != bits(d)
    assert not bad.any(), (what, "cells a sweep over the observed transitions moves", int(bad.sum()), np.flatnonzero(bad)[:8].tolist(),
                           d[bad][:4].tolist(), again[bad][:4].tolist())
    with np.errstate(invalid="ignore", over="ignore"):
        want = (np.asarray(d, np.float32)[:, None] * p).astype(np.float32)
    bad = bits(want) != bits(d_sa)
    assert not bad.any(), (what, "d_sa is not fl(d p)", int(bad.sum()), np.argwhere(bad)[:8].tolist())
    return int(count.sum()) * 4


# ------------------------------------------------------------- (b): where the running envs are at step t
def running_counts(rows, S, T=None):
    """int64[T,S]: C_t[s], the envs on cell s before step t none of whose earlier rows has done set"""
    _, done_t, _, key_t, _ = rows
    T = done_t.shape[0] if T is None else T
    before = np.zeros(done_t.shape, bool)
    before[1:] = np.logical_or.accumulate(done_t, 0)[:-1]
    out = np.zeros((T, S), np.int64)
    for t in range(T):
        out[t] = np.bincount(key_t[t][~before[t]] % S, minlength=S)
    return out


def counts_follow_marginals(C, mu, N, alpha, what):
    """C_t[s] against Binomial(N, mu_t[s]) in every bin the law can reach, by the exact two-sided tail (twice the smaller
    one-sided tail, capped at 1) at alpha / bins; where mu_t[s] = 0 -- no path of t steps: every product behind a positive mu is
    of factors >= 2^-5 and far from underflow in float64 -- the count must be 0.  Returns (bins, the least tail)."""
    assert C.shape == mu.shape
    off = mu == 0
    assert (C[off] == 0).all(), (what, "envs where the law has no mass", np.argwhere(off & (C > 0))[:8].tolist())
    k, p = C[~off], np.minimum(mu[~off], 1.0)
    tail = np.minimum(1.0, 2 * np.minimum(binom.cdf(k, N, p), binom.sf(k - 1, N, p)))
    B = tail.size
    worst = int(tail.argmin())
    print(what, "bins", B, "least tail", float(tail.min()), "against", alpha / B, "count", int(k[worst]), "of", N, "law", float(p[worst]))
    assert tail.min() >= alpha / B, what
    return B, float(tail.min())


def partial_sum(mu, gamma):
    """float64[S]: D_T = sum_{j<T} g^j mu_j with g the float32 number the sweep works with"""
    g = float(np.float32(gamma))
    return (mu * (g ** np.arange(mu.shape[0]))[:, None]).sum(0)


def partial_bound(gamma, T, d_norm):
    """|| D32_T - D_T ||_1 after T sweeps from zero.  test_occupancy_cpu.py's d_bound() is the T -> infinity form of this and is
    infinite at gamma = 1.  A sweep computes D32_j = (1 + e0) start + gamma (P + dP)^T D32_(j-1) exactly, |e0| <= u and
    |dP| <= rel(ROUNDINGS - 1) P entry by entry (its count of roundings), so E_j = D32_j - D_j obeys
    || E_j ||_1 <= (u + rel(ROUNDINGS - 1)) m + gamma || E_(j-1) ||_1 <= rel(ROUNDINGS) m + gamma || E_(j-1) ||_1 with
    m = max(|| D_T ||_1, || D32_T ||_1) (the D_j only grow, start <= D_j, || P^T ||_1 <= 1, gamma <= 1) and E_0 = 0:
    || E_T ||_1 <= rel(ROUNDINGS) m sum_{j<T} gamma^j, which is below d_bound() for gamma < 1 and T rel(ROUNDINGS) m at 1."""
    g = float(np.float32(gamma))
    return rel(ROUNDINGS) * d_norm * float((g ** np.arange(T)).sum())


# ------------------------------------------------------------- rows without a GPU
class HostAdapter:
    """case_rows()'s adapter over a HostEnv"""

    def __init__(self, env):
        self.env = env

    def place(self, ball_xy, goal_xy=None):
        self.env.place(ball_xy, goal_xy)

    def sample(self, T, thr, key):
        return self.env.rollout(T, key, True, thresholds=thr)

    def greedy(self, T, pol, epsilon, key):
        return self.env.rollout(T, key, True, policy=pol, eps32=eps_u32(epsilon))


class HostEnv:
    """LmazeVecEnv's state and epochs on the host, stepped by the C oracle: the constructor resets once (epoch 0), reset()
    spends one epoch, a rollout of T steps T of them; env_base 0.  Only what the twin needs."""

    def __init__(self, variant, lay, N, seed, step_limit, rewards=(-1.0, -0.01, 100.0)):
        self.v3, self.N, self.seed, self.epoch = variant == "v3", N, seed, 0
        self.lay = np.ascontiguousarray(lay)
        self.per_env = self.lay.ndim == 3
        self.G = self.lay.shape[-1]
        self.p = O.params(O.VARIANT_V3 if self.v3 else O.VARIANT_V0, self.G, O.LAYOUT_PER_ENV if self.per_env else O.LAYOUT_SHARED,
                          step_limit, *rewards)
        self.ball, self.goal = np.zeros((N, 2), np.int32), np.zeros((N, 2), np.int32)
        self.step_count, self.reward, self.done = np.zeros(N, np.int32), np.zeros(N, np.float32), np.zeros(N, np.uint8)
        self.goal_count = np.zeros(N, np.int32)
        self.reset()

    def _reset(self, mask, epoch):
        O.reset(self.p, self.lay, mask, self.seed, epoch, self.ball, self.goal if self.v3 else None, self.step_count, self.reward,
                self.done)

    def reset(self):
        self._reset(None, self.epoch)
        self.epoch += 1

    def place(self, ball_xy, goal_xy=None):
        self.ball[:] = ball_xy
        if goal_xy is not None:
            self.goal[:] = goal_xy
        self.step_count[:] = 0
        self.done[:] = 0
        self.reward[:] = -0.01

    def keys(self, key):
        S = self.G * self.G
        k = self.ball[:, 0].astype(np.int64) * self.G + self.ball[:, 1]
        if key == "goal":
            k = k + (self.goal[:, 0].astype(np.int64) * self.G + self.goal[:, 1]) * S
        if key == "env":
            k = k + np.arange(self.N, dtype=np.int64) * S
        return k.astype(np.int32)

    def rollout(self, T, key, auto_reset, thresholds=None, policy=None, eps32=0):
        """rollout_sample(thresholds=) or rollout_policy(policy=, epsilon=eps32 / 2^32): rows as rows_of() gives them"""
        N = self.N
        reward_t, done_t = np.zeros((T, N), np.float32), np.zeros((T, N), bool)
        act_t, key_t = np.zeros((T, N), np.int32), np.zeros((T, N), np.int32)
        eg = np.arange(N, dtype=np.uint64)
        for t in range(T):
            if auto_reset and self.done.any():
                self._reset(self.done.copy(), self.epoch + t)
            k = self.keys(key)
            if thresholds is not None:
                act = sample_action(thresholds[k], explore_draw(self.seed, self.epoch + t, eg)[0])
            elif eps32:
                r = explore_draw(self.seed, self.epoch + t, eg)
                act = epsilon_greedy(policy[k], eps32, r[0], r[1])[0]
            else:
                act = policy[k].astype(np.int32)
            act = np.ascontiguousarray(act, dtype=np.int32)
            if self.v3:
                O.step_v3(self.p, self.lay, act, self.ball, self.goal, self.step_count, self.reward, self.done)
            else:
                O.step_v0(self.p, self.lay, act, self.ball, self.step_count, self.reward, self.done, self.goal_count)
            reward_t[t], done_t[t], act_t[t], key_t[t] = self.reward, self.done != 0, act, k
        self.epoch += T
        return reward_t, done_t, act_t, key_t, np.concatenate([key_t[1:], self.keys(key)[None]])
