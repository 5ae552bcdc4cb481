"""Reference for lmaze_evaluate (include/lmaze.h): policy evaluation over the model that solve_ref.extract_model takes from the C
oracle's step -- the transition rule is not restated here.  The header's rule in numpy: integer weights in units of 2^-34
(int64), the weight on an excluded pair dropped, p = float32(w') / float32(W) (both conversions and the division correctly
rounded), then the Jacobi sweep in float32 with every product and sum rounded on its own and the same three stops."""
import collections

import numpy as np

import solve_ref as SR

Evaluated = collections.namedtuple("Evaluated", "q v sweeps_run delta")
TWO32 = 1 << 32
FULL = 1 << 34                      # the weights of a state sum to this where nothing is excluded


def first_max(q):
    """uint8[...]: the first maximum of the last axis by a strict '>' from action 0 on; a NaN never wins, a NaN in word 0 stays"""
    q = np.asarray(q, np.float32)
    best = q[..., 0].copy()
    act = np.zeros(best.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        for a in (1, 2, 3):
            better = q[..., a] > best
            best = np.where(better, q[..., a], best)
            act = np.where(better, np.uint8(a), act)
    return act


def weights(policy=None, q=None, epsilon_u32=0, thresholds=None):
    """int64[..., 4]: the weights w_a of every state in units of 2^-34, before anything is excluded.  Exactly one input."""
    assert sum(x is not None for x in (policy, q, thresholds)) == 1
    if thresholds is not None:
        c = np.asarray(thresholds).astype(np.int64) & (TWO32 - 1)            # uint32 or int32 bits
        s = np.sort(c[..., :3], axis=-1)                                     # the sampler counts the words r reaches
        d = np.stack([s[..., 0], s[..., 1] - s[..., 0], s[..., 2] - s[..., 1], TWO32 - s[..., 2]], -1)
        return 4 * d
    greedy = first_max(q) if q is not None else np.asarray(policy, np.uint8)
    e = int(epsilon_u32)
    assert 0 <= e < TWO32
    hit = greedy[..., None] == np.arange(4, dtype=np.uint8)
    return np.int64(e) + np.where(hit, np.int64(4 * (TWO32 - e)), np.int64(0))


def usable(w, sticky, wall):
    """w' and W: the weight on an excluded pair (and every weight of a wall state) dropped, and the integer sum"""
    wp = np.where(sticky | wall[..., None], np.int64(0), w)
    return wp, wp.sum(-1)


def probabilities(w, sticky, wall):
    """float32[..., 4]: p_a = fl(fl(w'_a) / fl(W)), 0 where W == 0"""
    wp, W = usable(w, sticky, wall)
    num = wp.astype(np.float32)
    den = np.where(W == 0, np.int64(1), W).astype(np.float32)[..., None]
    return np.where((W == 0)[..., None], np.float32(0), num / den).astype(np.float32)


def expectation(p, q):
    """V(s) = sum_a p_a q_a in the order a = 0..3, from the first term itself, over the actions that carry weight"""
    v = np.zeros(p.shape[:-1], np.float32)
    first = np.ones(p.shape[:-1], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(4):
            use = p[..., a] != 0
            term = (p[..., a] * q[..., a]).astype(np.float32)                # rounded
            v = np.where(use, np.where(first, term, (v + term).astype(np.float32)), v)      # rounded
            first &= ~use
    return v.astype(np.float32)


def action_values(nxt, r, terminal, sticky, gamma, v_flat):
    """Q(s, .) of non-wall rows: solve_ref.sweep's, r for a terminal pair, else r + gamma * v[next], -inf where excluded"""
    g = np.float32(gamma)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = g * v_flat[nxt]
        q = np.where(terminal, r, r + prod).astype(np.float32)
    q[sticky] = -np.inf
    return q


def sweep(model, gamma, p, v_old):
    """One Jacobi sweep: (q float32[S,4], v float32[S]) from V_(k-1)"""
    q = action_values(model.nxt, model.r, model.terminal, model.sticky, gamma, v_old)
    q[model.wall] = 0.0
    v = expectation(p, q)
    v[model.wall] = 0.0
    return q, v


def tol_bits(tol):
    """None when tol never stops a solve (not > 0: zero, negative, NaN), else its float32 bit pattern"""
    t = np.float32(tol)
    return int(t.view(np.uint32)) if t > 0 else None


def evaluate(model, gamma, sweeps, tol=0.0, v_init=None, deltas=None, **table):
    """One problem, sweep by sweep: the definition.  table: policy= / q= with epsilon_u32=, or thresholds=.  deltas: a list
    that receives every sweep's delta."""
    S = model.G * model.G
    p = probabilities(weights(**table), model.sticky, model.wall)
    v = np.zeros(S, np.float32) if v_init is None else np.ascontiguousarray(v_init, dtype=np.float32).reshape(S).copy()
    tb = tol_bits(tol)
    k = 0
    while True:
        k += 1
        q, v_new = sweep(model, gamma, p, v)
        with np.errstate(invalid="ignore", over="ignore"):
            diff = (v_new - v).astype(np.float32)
        dbits = (diff.view(np.uint32) & np.uint32(0x7FFFFFFF)).max()
        same = (v_new.view(np.uint32) == v.view(np.uint32)).all()
        v = v_new
        if deltas is not None:
            deltas.append(np.uint32(dbits).view(np.float32))
        if same or (tb is not None and int(dbits) <= tb) or k == sweeps:
            return Evaluated(q, v, np.int32(k), np.uint32(dbits).view(np.float32))


def evaluate_many(variant, layouts, goals, gamma, sweeps, tol=0.0, rewards=SR.DEFAULT_REWARDS, v_init=None, models=None, **table):
    """evaluate() of every problem, stacked as solve_ref.solve_many stacks: the same sweep on all problems at once over their
    non-wall states, each problem leaving when its own stop rule says so.  The tables are [P, S(, 4)].  models: what
    solve_ref.models_of gave for these problems, when the caller holds it already.  test_evaluate_cpu.py holds this against
    evaluate() problem by problem."""
    if models is None:
        models = SR.models_of(variant, layouts, goals, rewards)
    P, S = len(models), models[0].G ** 2
    v = np.zeros((P, S), np.float32) if v_init is None else np.ascontiguousarray(v_init, dtype=np.float32).reshape(P, S).copy()
    wall = np.stack([m.wall for m in models])
    sticky_all = np.stack([m.sticky for m in models])
    p_all = probabilities(weights(**table), sticky_all, wall)
    assert p_all.shape == (P, S, 4)
    rp, rs = np.nonzero(~wall)                                   # the rows: (problem, state), sorted by problem
    assert len(np.unique(rp)) == P, "a problem without a non-wall cell"
    at = rp * S + rs
    nxt = (rp[:, None] * S + np.stack([m.nxt for m in models])[rp, rs]).astype(np.int64)
    r = np.stack([m.r for m in models])[rp, rs]
    terminal = np.stack([m.terminal for m in models])[rp, rs]
    sticky = sticky_all[rp, rs]
    p = p_all[rp, rs]
    q_out = np.zeros((P, S, 4), np.float32)
    run = np.zeros(P, np.int32)
    delta = np.zeros(P, np.uint32)
    # the wall states' only sweep that can change anything: the first, from v_init to 0
    wall_bits = np.where(wall, v.view(np.uint32), 0)
    wall_changed = (wall_bits != 0).any(1)
    wall_delta = (wall_bits & np.uint32(0x7FFFFFFF)).max(1)
    v[wall] = 0.0
    v = v.reshape(-1)
    tb = tol_bits(tol)
    rows = np.arange(len(at))
    k = 0
    while len(rows):
        k += 1
        a_at, a_p = at[rows], rp[rows]
        q = action_values(nxt[rows], r[rows], terminal[rows], sticky[rows], gamma, v)
        new = expectation(p[rows], q)
        old = v[a_at]
        with np.errstate(invalid="ignore", over="ignore"):
            dbits = (new - old).astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
        starts = np.flatnonzero(np.r_[True, a_p[1:] != a_p[:-1]])
        who = a_p[starts]
        changed = np.logical_or.reduceat(new.view(np.uint32) != old.view(np.uint32), starts)
        d = np.maximum.reduceat(dbits, starts)
        if k == 1:
            changed |= wall_changed[who]
            d = np.maximum(d, wall_delta[who])
        v[a_at] = new
        stop = ~changed | (k == sweeps)
        if tb is not None:
            stop |= d <= np.uint32(tb)
        if stop.any():
            leaving = np.zeros(P, bool)
            leaving[who[stop]] = True
            sel = leaving[a_p]
            q_out[a_p[sel], rs[rows][sel]] = q[sel]
            run[who[stop]] = k
            delta[who[stop]] = d[stop]
            rows = rows[~sel]
    return Evaluated(q_out, v.reshape(P, S).copy(), run, delta.view(np.float32))


def renormalised(w, sticky, wall):
    """bool[...]: the states whose policy puts weight on an excluded pair and keeps some on a usable one"""
    wp, W = usable(w, sticky, wall)
    return ~wall & ((w != wp).any(-1)) & (W > 0)


def exact_probabilities(w, sticky, wall):
    """float64[..., 4]: w' / W, 0 where W == 0"""
    wp, W = usable(w, sticky, wall)
    return np.where((W == 0)[..., None], 0.0, wp / np.where(W == 0, 1, W)[..., None].astype(np.float64))


def exact_values(model, gamma, w):
    """float64[S]: (I - gamma P_pi) v = r_pi over the non-wall states, with the exact probabilities w' / W; a terminal pair
    pays its reward and cuts the chain.  gamma and the rewards are the float32 numbers the sweep works with."""
    return exact_values_of(model, gamma, exact_probabilities(w, model.sticky, model.wall))


def exact_values_of(model, gamma, prob):
    """exact_values() with the probabilities float64[S,4] given directly (0 on every excluded pair and wall state)"""
    S = model.G * model.G
    gamma = float(np.float32(gamma))
    A = np.eye(S)
    b = np.zeros(S)
    for s in np.flatnonzero(~model.wall):
        for a in range(4):
            if prob[s, a] == 0:
                continue
            b[s] += prob[s, a] * float(model.r[s, a])
            if not model.terminal[s, a]:
                A[s, model.nxt[s, a]] -= gamma * prob[s, a]
    return np.linalg.solve(A, b)


def exact_action_values(model, gamma, v):
    """float64[S,4]: Q = r on a terminal pair, else r + gamma v[next]; 0 on wall states; an excluded pair keeps r + gamma v[s]
    (finite: it carries no probability)"""
    gamma = float(np.float32(gamma))
    q = np.where(model.terminal, model.r.astype(np.float64), model.r.astype(np.float64) + gamma * np.asarray(v, np.float64)[model.nxt])
    q[model.wall] = 0.0
    return q
