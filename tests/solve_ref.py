"""Reference for lmaze_solve (include/lmaze.h): the model of a maze EXTRACTED from the C oracle's step -- the transition rule
is not restated here -- and the Jacobi sweep of the header in numpy float32, product and sum rounded separately, the first
maximum by a strict '>', the same stop rule.  Also steps_to_done(): a plain BFS over the model."""
import collections

import numpy as np

import oracle_lib as O

SENTINEL = np.float32(12345.0)      # the incoming reward: a pair that hands it back has no reward of its own
HUGE_LIMIT = 1 << 30                # no step limit triggers: v0 compares step_count (1) with ==, v3 with >
DEFAULT_REWARDS = (-1.0, -0.01, 100.0)

Model = collections.namedtuple("Model", "G nxt r terminal sticky wall")
Solved = collections.namedtuple("Solved", "q v policy sweeps_run delta")


def extract_model(variant, layout, goal=None, rewards=DEFAULT_REWARDS):
    """The (cell, action) model of one layout uint8[G,G]: one oracle env per pair of a non-wall cell, stepped once.  nxt
    int32[S,4], r float32[S,4], terminal / sticky bool[S,4], wall bool[S].  A wall cell is a state nothing is computed for
    (stepping from a border cell would look off the grid), its rows stay nxt = s, r = 0."""
    layout = np.ascontiguousarray(layout, dtype=np.uint8)
    G = layout.shape[0]
    S = G * G
    wall = layout.reshape(-1) == ord("W")
    cells = np.flatnonzero(~wall).astype(np.int32)
    n = len(cells) * 4
    ball = np.ascontiguousarray(np.repeat(np.stack([cells // G, cells % G], 1), 4, axis=0).astype(np.int32))
    start = ball.copy()
    action = np.ascontiguousarray(np.tile(np.arange(4, dtype=np.int32), len(cells)))
    step_count = np.zeros(n, np.int32)
    reward = np.full(n, SENTINEL, np.float32)
    done = np.zeros(n, np.uint8)
    v3 = variant in ("v3", O.VARIANT_V3)
    p = O.params(O.VARIANT_V3 if v3 else O.VARIANT_V0, G, O.LAYOUT_SHARED, HUGE_LIMIT, *rewards)
    if n:
        if v3:
            goal_xy = np.ascontiguousarray(np.tile(np.asarray(goal, np.int32).reshape(1, 2), (n, 1)))
            O.step_v3(p, layout, action, ball, goal_xy, step_count, reward, done)
        else:
            O.step_v0(p, layout, action, ball, step_count, reward, done)
    nxt = np.repeat(np.arange(S, dtype=np.int32)[:, None], 4, axis=1)
    r = np.zeros((S, 4), np.float32)
    sticky = np.zeros((S, 4), bool)
    nxt[cells] = (ball[:, 0] * G + ball[:, 1]).reshape(-1, 4)
    r[cells] = reward.reshape(-1, 4)
    stuck = (reward.view(np.uint32) == SENTINEL.view(np.uint32)) & (ball == start).all(1)
    sticky[cells] = stuck.reshape(-1, 4)
    terminal = (r == np.float32(rewards[2])) & ~sticky & ~wall[:, None]
    assert ((done.reshape(-1, 4) != 0) == terminal[cells]).all()          # the oracle's own done flag says the same
    return Model(G, nxt, r, terminal, sticky, wall)


def sweep(model, gamma, v_old):
    """One Jacobi sweep: (q float32[S,4], v float32[S], policy uint8[S]) from V_(k-1)."""
    g = np.float32(gamma)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = g * v_old[model.nxt]                  # float32 * float32, rounded
        q = np.where(model.terminal, model.r, model.r + prod).astype(np.float32)      # then the sum, rounded
    q[model.sticky] = -np.inf
    q[model.wall] = 0.0
    best = q[:, 0].copy()
    pol = np.zeros(len(best), np.uint8)
    for a in (1, 2, 3):
        better = q[:, a] > best
        best = np.where(better, q[:, a], best)
        pol = np.where(better, np.uint8(a), pol)
    none = model.sticky.all(1) | model.wall
    best[none] = 0.0
    pol[none] = 0
    return q, best.astype(np.float32), pol.astype(np.uint8)


def solve(model, gamma, sweeps, v_init=None):
    S = model.G * model.G
    v = np.zeros(S, np.float32) if v_init is None else np.ascontiguousarray(v_init, dtype=np.float32).reshape(S).copy()
    k = 0
    while True:
        k += 1
        q, v_new, pol = sweep(model, gamma, v)
        with np.errstate(invalid="ignore", over="ignore"):
            diff = (v_new - v).astype(np.float32)
        delta = (diff.view(np.uint32) & np.uint32(0x7FFFFFFF)).max().view(np.float32)      # a maximum of bit patterns
        same = (v_new.view(np.uint32) == v.view(np.uint32)).all()
        v = v_new
        if same or k == sweeps:
            return Solved(q, v, pol, np.int32(k), np.float32(delta))


def models_of(variant, layouts, goals, rewards=DEFAULT_REWARDS):
    """One model per problem: layouts[p] (or the one layout [G,G] for every goal) with goals[p]; the oracle is asked layout
    by layout, in shared mode, so its batches stay small."""
    layouts = np.asarray(layouts)
    shared = layouts.ndim == 2
    P = len(goals) if goals is not None else (1 if shared else layouts.shape[0])
    return [extract_model(variant, layouts if shared else layouts[p], None if goals is None else goals[p], rewards) for p in range(P)]


def solve_many(variant, layouts, goals, gamma, sweeps, rewards=DEFAULT_REWARDS, v_init=None):
    """solve() of every problem, stacked: the same sweep on all problems at once, over their non-wall states only (a wall
    state is 0 from the first sweep on and nobody's successor), each problem leaving when its own stop rule says so.
    test_solve_cpu.py holds it against solve() problem by problem."""
    models = models_of(variant, layouts, goals, rewards)
    P, S = len(models), models[0].G ** 2
    g = np.float32(gamma)
    v = np.zeros((P, S), np.float32) if v_init is None else np.ascontiguousarray(v_init, dtype=np.float32).reshape(P, S).copy()
    wall = np.stack([m.wall for m in models])
    rp, rs = np.nonzero(~wall)                                   # the rows: (problem, state), sorted by problem
    assert len(np.unique(rp)) == P, "a problem without a non-wall cell"
    at = rp * S + rs
    nxt = (rp[:, None] * S + np.stack([m.nxt for m in models])[rp, rs]).astype(np.int64)
    r = np.stack([m.r for m in models])[rp, rs]
    terminal = np.stack([m.terminal for m in models])[rp, rs]
    sticky = np.stack([m.sticky for m in models])[rp, rs]
    none = sticky.all(1)
    q_out = np.zeros((P, S, 4), np.float32)
    pol_out = np.zeros((P, S), np.uint8)
    run = np.zeros(P, np.int32)
    delta = np.zeros(P, np.uint32)
    # the wall states' only sweep that can change anything: the first, from v_init to 0
    wall_bits = np.where(wall, v.view(np.uint32), 0)
    wall_changed = (wall_bits != 0).any(1)
    wall_delta = (wall_bits & np.uint32(0x7FFFFFFF)).max(1)
    v[wall] = 0.0
    v = v.reshape(-1)
    active = np.ones(P, bool)
    rows = np.arange(len(at))
    k = 0
    while active.any():
        k += 1
        a_at, a_p = at[rows], rp[rows]
        with np.errstate(invalid="ignore", over="ignore"):
            prod = g * v[nxt[rows]]
            q = np.where(terminal[rows], r[rows], r[rows] + prod).astype(np.float32)
        q[sticky[rows]] = -np.inf
        best = q[:, 0].copy()
        pol = np.zeros(len(rows), np.uint8)
        for a in (1, 2, 3):
            better = q[:, a] > best
            best = np.where(better, q[:, a], best)
            pol = np.where(better, np.uint8(a), pol)
        best[none[rows]] = 0.0
        pol[none[rows]] = 0
        old = v[a_at]
        with np.errstate(invalid="ignore", over="ignore"):
            dbits = (best - old).astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
        starts = np.flatnonzero(np.r_[True, a_p[1:] != a_p[:-1]])
        who = a_p[starts]
        changed = np.logical_or.reduceat(best.view(np.uint32) != old.view(np.uint32), starts)
        d = np.maximum.reduceat(dbits, starts)
        if k == 1:
            changed |= wall_changed[who]
            d = np.maximum(d, wall_delta[who])
        v[a_at] = best
        stop = ~changed | (k == sweeps)
        if stop.any():
            leaving = np.zeros(P, bool)
            leaving[who[stop]] = True
            sel = leaving[a_p]
            q_out[a_p[sel], rs[rows][sel]] = q[sel]
            pol_out[a_p[sel], rs[rows][sel]] = pol[sel]
            run[who[stop]] = k
            delta[who[stop]] = d[stop]
            active &= ~leaving
            rows = rows[~sel]
    return Solved(q_out, v.reshape(P, S).copy(), pol_out, run, delta.view(np.float32))


def steps_to_done(model):
    """float64[S]: the fewest steps after which an env started on the cell can have done set -- a breadth-first search
    backwards from the states that own a terminal pair; inf where no terminal pair can be reached (walls included)."""
    S = model.G * model.G
    usable = ~model.sticky & ~model.wall[:, None]
    dist = np.full(S, np.inf)
    dist[(model.terminal & usable).any(1)] = 1
    frontier = np.flatnonzero(dist == 1)
    d = 1
    while len(frontier):
        d += 1
        hit = np.isin(model.nxt, frontier) & usable & ~model.terminal
        new = np.flatnonzero(hit.any(1) & np.isinf(dist))
        dist[new] = d
        frontier = new
    return dist


def greedy_lowers_distance(model, policy, dist):
    """bool[S], over the reachable states: the policy's pair is terminal from distance 1, or leads to distance - 1."""
    s = np.flatnonzero(np.isfinite(dist))
    a = policy[s].astype(np.int64)
    term = model.terminal[s, a]
    ok = np.where(term, dist[s] == 1, dist[model.nxt[s, a]] == dist[s] - 1)
    return ok & ~model.sticky[s, a]


def unreachable_goals(lays, goals, every=4):
    """v3 goals no step can pay for, written over goals[::every]: off the grid on each side and far off both, and on the
    border's corners (the look-ahead pays when the cell BEYOND the ball's new cell is the goal -- v3:264 -- so the ball would
    have to stand on a border cell beside the goal; the other wall cells CAN be paid for, from two cells away, see
    walled_goals).  Returns (goals, the problems overwritten)."""
    G = lays.shape[-1]
    goals = np.array(goals, dtype=np.int32, copy=True)
    who = np.arange(0, len(goals), every)
    kinds = ((-1, 3), (2, G), (G, 1), (4, -1), (-3, G + 2), (G + 40, -70), (0, 0), (G - 1, G - 1), (0, G - 1), (G - 1, 0))
    for j, p in enumerate(who):
        goals[p] = kinds[j % len(kinds)]
    return goals, who


def walled_goals(lays, goals, seed, every=4):
    """v3 goals on wall cells other than the corners, border and interior alike, written over goals[1::every]"""
    rs = np.random.RandomState(seed)
    G = lays.shape[-1]
    goals = np.array(goals, dtype=np.int32, copy=True)
    who = np.arange(1, len(goals), every)
    corners = {(0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1)}
    for p in who:
        cells = [tuple(c) for c in np.argwhere(lays[p] == ord("W")) if tuple(c) not in corners]
        goals[p] = cells[rs.randint(len(cells))]
    return goals, who


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
