"""Reference for lmaze_occupancy (include/lmaze.h): the discounted occupancy over the model that solve_ref.extract_model takes
from the C oracle's step and the probabilities of evaluate_ref.probabilities -- neither the transition rule nor the weight rule
is restated here.  The header's gather (win, wself) from the model's successor table, then the Jacobi sweep in float32 with
every product and sum rounded on its own and lmaze_evaluate's three stops; and a float64 linear solve of the same equation."""
import collections

import numpy as np

import evaluate_ref as E
import solve_ref as SR

Occupancy = collections.namedtuple("Occupancy", "d d_sa sweeps_run delta")


def flows(model):
    """bool[S,4]: the pairs whose mass moves on -- usable, not terminal, of a non-wall cell"""
    return ~model.sticky & ~model.terminal & ~model.wall[:, None]


def gather(model, p):
    """(win float32[S,4], src int64[S,4], wself float32[S]) of one problem from its probabilities p float32[S,4]: win[c,a] is
    the probability of the one pair (src[c,a], a) that moves the ball onto c, wself the ordered sum of the pairs that flow
    and leave it in place"""
    return gather_successors(model.G, model.nxt, flows(model), model.wall, p)


def gather_successors(G, nxt, fl, wall, p):
    """gather() from a successor table alone, wherever it comes from -- the model's, or the one the rows of a rollout show
    (nxt int[S,4]: the cell a pair leads to; fl bool[S,4]: the pairs whose mass moves on, i.e. usable, of a non-wall cell and
    never seen with done set).  The geometry is asserted, not assumed: a pair that moves arrives one step(a) away, in the same
    row for a = 2, 3, on a cell that is not a wall, and no two sources share a (cell, action)."""
    S = G * G
    cells = np.arange(S)
    nxt = np.asarray(nxt).reshape(S, 4)
    moved = nxt != cells[:, None]
    win = np.zeros((S, 4), np.float32)
    src = np.repeat(cells[:, None], 4, axis=1).astype(np.int64)
    for a, step in enumerate((-G, G, -1, 1)):
        s = np.flatnonzero(fl[:, a] & moved[:, a])
        c = nxt[s, a].astype(np.int64)
        assert (c - s == step).all() and len(np.unique(c)) == len(c)          # next = s + step(a): one source per (c, a)
        if a >= 2:
            assert (c // G == s // G).all()                                    # in the same row
        assert not wall[c].any()
        win[c, a] = p[s, a]
        src[c, a] = s
    wself = np.zeros(S, np.float32)
    first = np.ones(S, bool)
    for a in range(4):
        use = fl[:, a] & ~moved[:, a]
        wself = np.where(use, np.where(first, p[:, a], (wself + p[:, a]).astype(np.float32)), wself).astype(np.float32)
        first &= ~use
    return win, src, wself


def sweep(win, src, wself, wall, start, gamma, d_old):
    """One Jacobi sweep over arrays [..., S(, 4)]; src indexes the flattened d_old"""
    g = np.float32(gamma)
    flat = d_old.reshape(-1)
    acc = np.zeros(d_old.shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(4):
            use = win[..., a] != 0
            term = (win[..., a] * flat[src[..., a]]).astype(np.float32)         # rounded
            acc = np.where(use, (acc + term).astype(np.float32), acc)          # rounded
        use = wself != 0
        term = (wself * d_old).astype(np.float32)
        acc = np.where(use, (acc + term).astype(np.float32), acc)
        disc = (g * acc).astype(np.float32)
        d = (start + disc).astype(np.float32)
    return np.where(wall, np.float32(0), d).astype(np.float32)


def _stop_bits(d_new, d_old):
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (d_new - d_old).astype(np.float32)
    return diff.view(np.uint32) & np.uint32(0x7FFFFFFF), d_new.view(np.uint32) != d_old.view(np.uint32)


def occupancy(model, gamma, sweeps, start, tol=0.0, d_init=None, deltas=None, history=None, **table):
    """One problem, sweep by sweep: the definition.  table: policy= / q= with epsilon_u32=, or thresholds=.  deltas, history:
    lists that receive every sweep's delta and D_k."""
    S = model.G * model.G
    p = E.probabilities(E.weights(**table), model.sticky, model.wall)
    win, src, wself = gather(model, p)
    start = np.where(model.wall, np.float32(0), np.ascontiguousarray(start, dtype=np.float32).reshape(S))     # not read on 'W'
    d = np.zeros(S, np.float32) if d_init is None else np.ascontiguousarray(d_init, dtype=np.float32).reshape(S).copy()
    tb = E.tol_bits(tol)
    k = 0
    while True:
        k += 1
        d_new = sweep(win, src, wself, model.wall, start, gamma, d)
        dbits, changed = _stop_bits(d_new, d)
        d = d_new
        if deltas is not None:
            deltas.append(np.uint32(dbits.max()).view(np.float32))
        if history is not None:
            history.append(d.copy())
        if not changed.any() or (tb is not None and int(dbits.max()) <= tb) or k == sweeps:
            with np.errstate(invalid="ignore", over="ignore"):
                d_sa = (d[:, None] * p).astype(np.float32)
            return Occupancy(d, d_sa, np.int32(k), np.uint32(dbits.max()).view(np.float32))


def occupancy_many(models, gamma, sweeps, start, tol=0.0, d_init=None, **table):
    """occupancy() of every problem, stacked: the same sweep on the problems still running, each leaving when its own stop rule
    says so.  The tables and start are [P, S(, 4)].  test_occupancy_cpu.py holds this against occupancy() problem by problem."""
    P, S = len(models), models[0].G ** 2
    wall = np.stack([m.wall for m in models])
    p = E.probabilities(E.weights(**table), np.stack([m.sticky for m in models]), wall)
    assert p.shape == (P, S, 4)
    parts = [gather(m, p[i]) for i, m in enumerate(models)]
    win = np.stack([x[0] for x in parts])
    src = np.stack([x[1] for x in parts])                       # within the problem
    wself = np.stack([x[2] for x in parts])
    start = np.where(wall, np.float32(0), np.ascontiguousarray(start, dtype=np.float32).reshape(P, S))
    d = np.zeros((P, S), np.float32) if d_init is None else np.ascontiguousarray(d_init, dtype=np.float32).reshape(P, S).copy()
    run = np.zeros(P, np.int32)
    delta = np.zeros(P, np.uint32)
    tb = E.tol_bits(tol)
    act = np.arange(P)
    k = 0
    while len(act):
        k += 1
        local = src[act] + (np.arange(len(act)) * S)[:, None, None]
        d_old = d[act]
        d_new = sweep(win[act], local, wself[act], wall[act], start[act], gamma, d_old)
        dbits, changed = _stop_bits(d_new, d_old)
        d[act] = d_new
        dmax = dbits.max(1)
        stop = ~changed.any(1) | (k == sweeps)
        if tb is not None:
            stop |= dmax <= np.uint32(tb)
        run[act[stop]] = k
        delta[act[stop]] = dmax[stop]
        act = act[~stop]
    with np.errstate(invalid="ignore", over="ignore"):
        d_sa = (d[:, :, None] * p).astype(np.float32)
    return Occupancy(d, d_sa, run, delta.view(np.float32))


def exact_occupancy(model, gamma, w, start):
    """float64[S]: (I - gamma P_pi^T) d = start over the non-wall states, with the exact probabilities w' / W; a terminal pair
    absorbs its mass.  gamma is the float32 number the sweep works with; d = 0 on walls."""
    prob = E.exact_probabilities(w, model.sticky, model.wall)
    return exact_occupancy_of(model, gamma, prob, start), prob


def transition(model, prob):
    """float64[S,S]: P[s, c], the probability that a step from s leaves the ball on c and the episode running -- prob
    float64[S,4] over the pairs that flow; a terminal pair, an excluded one and a wall state carry nothing"""
    S = model.G * model.G
    fl = flows(model)
    P = np.zeros((S, S))
    for a in range(4):
        s = np.flatnonzero(fl[:, a] & (prob[:, a] != 0))
        np.add.at(P, (s, model.nxt[s, a]), prob[s, a])
    return P


def exact_occupancy_of(model, gamma, prob, start):
    """exact_occupancy() with the probabilities float64[S,4] given directly (they are used as they are: 0 on an excluded pair
    is the caller's to see to)"""
    S = model.G * model.G
    gamma = float(np.float32(gamma))
    b = np.where(model.wall, 0.0, np.asarray(start, np.float64).reshape(S))
    return np.linalg.solve(np.eye(S) - gamma * transition(model, prob).T, b)


def step_marginals(model, prob, start, T):
    """float64[T,S]: mu_t = (P_pi^T)^t start, the law of the cell an env stands on before its step t with no done row before
    it (a terminal pair absorbs: mu_t sums to the chance that the episode still runs); mu_0 = start off the walls"""
    S = model.G * model.G
    Pt = transition(model, np.asarray(prob, np.float64)).T
    mu = np.zeros((T, S))
    mu[0] = np.where(model.wall, 0.0, np.asarray(start, np.float64).reshape(S))
    for t in range(1, T):
        mu[t] = Pt @ mu[t - 1]
    return mu


def pad_walls(layouts):
    """uint8[..., G+2, G+2]: the layouts inside one more ring of 'W'.  Stepping off the grid from a free border cell looks at a
    cell the oracle does not have; inside the ring the same step is a wall bump, which like the kernel's clamped target leaves
    the ball in place, usable and not terminal -- so where every free border cell is 'B' (v3: the goal on the grid) the padded
    model's flows and probabilities are the unpadded layout's."""
    layouts = np.asarray(layouts, np.uint8)
    out = np.full(layouts.shape[:-2] + (layouts.shape[-2] + 2, layouts.shape[-1] + 2), ord("W"), np.uint8)
    out[..., 1:-1, 1:-1] = layouts
    return out


def unpad_model(model):
    """The G x G model inside a pad_walls() model of side G + 2"""
    Gp = model.G
    G = Gp - 2
    inner = (np.arange(1, G + 1)[:, None] * Gp + np.arange(1, G + 1)[None, :]).reshape(-1)
    back = np.full(Gp * Gp, -1, np.int64)
    back[inner] = np.arange(G * G)
    nxt = back[model.nxt[inner]]
    assert (nxt >= 0).all()
    return SR.Model(G, nxt.astype(np.int32), model.r[inner], model.terminal[inner], model.sticky[inner], model.wall[inner])
