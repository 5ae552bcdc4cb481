"""Reference for lmaze_score (include/lmaze.h), the specification in numpy: the model is solve_ref.extract_model's (taken from
the C oracle's step, not restated), optimal is solve_ref.steps_to_done with inf -> -1, and the walk takes the table's action
in every state, all start states at once, for S steps of array operations.  doubling() emulates the kernel's scheme -- the pair
(where the walk stands after 2^k steps, the steps it took), two absorbing sentinels, Jacobi rounds -- and reports how many
rounds it needed; sweeps() does the same for the min-plus distances."""
import collections

import numpy as np

import solve_ref as SR
from qlearn_ref import first_max

Scored = collections.namedtuple("Scored", "optimal steps summary")
ARRIVED, NEVER = -1, -2


def log2_ceil(n):
    return int(n - 1).bit_length()


def actions_of(policy=None, q=None):
    """int64[S]: the action of every state, from policy bytes as they are (above 3: no action) or from q's first maximum"""
    if q is not None:
        return first_max(np.asarray(q, np.float32).reshape(-1, 4))[1].astype(np.int64)
    return np.asarray(policy).reshape(-1).astype(np.int64)


def optimal(model):
    d = SR.steps_to_done(model)
    return np.where(np.isfinite(d), d, -1).astype(np.int32)


def first_step(model, act):
    """(to int64[S], arrived bool[S], never bool[S]) after one step of the table's walk from every state: a wall state, an
    action above 3, an excluded pair and a bump (a cycle of one) never arrive"""
    S = model.G ** 2
    s = np.arange(S)
    valid = (act >= 0) & (act <= 3) & ~model.wall
    a = np.where(valid, act, 0)
    sticky, term, to = model.sticky[s, a], model.terminal[s, a], model.nxt[s, a].astype(np.int64)
    arrived = valid & ~sticky & term
    never = ~valid | sticky | (~term & (to == s))
    return to, arrived, never


def walk(model, act):
    """int32[S]: the step at which the walk first sets done, -1 if it never does.  All start states walk together; a walk
    that has not arrived after S steps is in a cycle (an arriving walk visits distinct states)."""
    S = model.G ** 2
    to, arrived, never = first_step(model, act)
    steps = np.full(S, -1, np.int32)
    start = np.arange(S)                       # the start states still walking, and where each stands
    cur = start.copy()
    for t in range(1, S + 1):
        steps[start[arrived[cur]]] = t
        on = ~arrived[cur] & ~never[cur]
        start, cur = start[on], to[cur[on]]
        if not len(start):
            break
    return steps


def doubling(model, act):
    """(steps int32[S], rounds run): the kernel's pointer doubling, two buffers, at most ceil(log2 S) rounds, ended sooner by
    the round after which no pointer is a live state"""
    S = model.G ** 2
    to, arrived, never = first_step(model, act)
    ptr = np.where(arrived, ARRIVED, np.where(never, NEVER, to))
    length = np.ones(S, np.int64)
    rounds = 0
    for _ in range(log2_ceil(S)):
        live = ptr >= 0
        at = np.where(live, ptr, 0)
        p2, l2 = ptr[at], length[at]
        new_ptr = np.where(live, p2, ptr)
        new_len = np.where(live & (p2 != NEVER), length + l2, length)
        assert new_len.max() < 65536                                   # the packed field
        ptr, length = new_ptr, new_len
        rounds += 1
        if not (ptr >= 0).any():
            break
    return np.where(ptr == ARRIVED, length, -1).astype(np.int32), rounds


def sweeps(model):
    """(optimal int32[S], sweeps run): the kernel's Jacobi min-plus sweeps from d_0, the unchanged sweep counted"""
    S = model.G ** 2
    INF = 0x3FFFFFFF
    usable = ~model.sticky & ~model.wall[:, None]
    d = np.where((model.terminal & usable).any(1), 1, INF).astype(np.int64)
    k = 0
    while k < S:
        k += 1
        via = np.where(model.terminal, 0, d[model.nxt]) + 1
        new = np.minimum(INF, np.where(usable, via, INF).min(1))
        same = (new == d).all()
        d = new
        if same:
            break
    return np.where(d >= INF, -1, d).astype(np.int32), k


def summary(opt, steps=None):
    """int32[4]: reachable, arrived, shortest, excess"""
    reach = int((opt >= 1).sum())
    if steps is None:
        return np.array([reach, 0, 0, 0], np.int32)
    arr = steps >= 1
    return np.array([reach, int(arr.sum()), int((arr & (steps == opt)).sum()), int((steps[arr] - opt[arr]).sum())], np.int32)


def score(model, policy=None, q=None):
    opt = optimal(model)
    if policy is None and q is None:
        return Scored(opt, None, summary(opt))
    steps = walk(model, actions_of(policy, q))
    return Scored(opt, steps, summary(opt, steps))


def score_many(variant, layouts, goals=None, policy=None, q=None, rewards=SR.DEFAULT_REWARDS, problems=None):
    """score() of every problem, stacked: layouts [G,G] (every problem) or [P,G,G]; tables [P,S] / [P,S,4] or None"""
    layouts = np.asarray(layouts)
    shared = layouts.ndim == 2
    table = policy if policy is not None else q
    P = problems if problems is not None else (len(goals) if goals is not None else (len(table) if shared and table is not None
                                               else (1 if shared else layouts.shape[0])))
    out = []
    memo = {}
    for p in range(P):
        key = ((layouts if shared else layouts[p]).tobytes(), None if goals is None else tuple(int(g) for g in goals[p]))
        if key not in memo:
            memo[key] = SR.extract_model(variant, layouts if shared else layouts[p], None if goals is None else goals[p], rewards)
        out.append(score(memo[key], None if policy is None else policy[p], None if q is None else q[p]))
    return Scored(np.stack([o.optimal for o in out]), None if table is None else np.stack([o.steps for o in out]),
                  np.stack([o.summary for o in out]))


def serpentine(G):
    """uint8[G,G]: one corridor through every free cell, 'X' at its end: the odd rows are open from column 1 to G - 2, the
    even rows between them open one cell, at alternating ends.  Returns (layout, the corridor's cells in order, the goal
    last)."""
    W, B, X = ord("W"), ord("B"), ord("X")
    lay = np.full((G, G), W, np.uint8)
    path = []
    right = True
    x = 1
    while x <= G - 2:
        cols = list(range(1, G - 1)) if right else list(range(G - 2, 0, -1))
        path += [(x, y) for y in cols]
        if x + 2 <= G - 2:
            path.append((x + 1, cols[-1]))
        right = not right
        x += 2
    for cx, cy in path:
        lay[cx, cy] = B
    lay[path[-1]] = X
    return lay, path


def corridor_policy(G, path):
    """uint8[S]: from every corridor cell the action towards the next one (0 up, 1 down, 2 left, 3 right); 0 elsewhere"""
    pol = np.zeros(G * G, np.uint8)
    for (x, y), (nx, ny) in zip(path[:-1], path[1:]):
        pol[x * G + y] = {(-1, 0): 0, (1, 0): 1, (0, -1): 2, (0, 1): 3}[(nx - x, ny - y)]
    return pol
