"""The sampling closed-loop foveal rollout (lmaze_foveal_rollout_sample, include/lmaze.h) restated on the host: the C oracle
(oracle_lib.foveal_reset / foveal_step) stepped T times, with the threshold conversion, the key, the draw and the sum of
compares in numpy.  Needs no GPU: test_gpu_foveal_rollout_sample.py compares the device against it, and
test_foveal_rollout_sample_cpu.py asserts here, from the oracle's side alone, that every case takes every path.

A case starts from foveal_policy_ref.start_state (N = 333, T = 24, step limit 9, a fifth of the envs done, step counts spread
up to the limit, a visit map with history)."""
import functools
from collections import namedtuple

import numpy as np

import foveal_policy_ref as P
import oracle_lib as O
from closed_loop_ref import explore_draw

N, T, STEP_LIMIT, SEED, ENV_BASE, EPOCH = P.N, P.T, P.STEP_LIMIT, P.SEED, P.ENV_BASE, P.EPOCH
STATE = P.STATE
LDS_RULE = 16384                     # bytes of table up to which it is staged in LDS

Shape = P.Shape                      # variant, G, layouts (0: the variant's shipped ones), where the launcher must put the table
SHAPES = (Shape("v1", 14, 0, "lds"),          # 3 136 B
          Shape("v1", 24, 1, "lds"),          # one random layout: 576 keys x 16 B = 9 216 B, under the rule's 16 384
          Shape("v1", 33, 1, "global"),       # 17 424 B: v1's kernels on the global side of the rule
          Shape("v2", 18, 0, "global"),       # the five shipped layouts: 155 520 B
          Shape("v4", 18, 0, "global"),
          Shape("v2", 12, 1, "lds"),          # 13 824 B
          Shape("v4", 12, 1, "lds"),
          Shape("v4", 12, 2, "global"))       # 27 648 B, the generic-grid kernels
# chosen with the oracle and numpy alone (test_foveal_rollout_sample_cpu.py asserts what they show): v1 at G = 14 never
# reaches the goal under seeds 1 and 2
SEEDS = {s: (3 if s.variant == "v1" and s.G != 24 else 1) for s in SHAPES}
# Goal rewards a case must show.  8 for every shape but v1 at G = 33: a 4-action walk over a 25 x 25 interior with one goal
# cell reaches it 4 or 5 times in 7 992 env-steps under the best of 40 seeds; the goal path itself is the same code on either
# side of the table rule and the other v1 shapes show it 8 times and more.
MIN_GOALS = {s: (4 if (s.variant, s.G) == ("v1", 33) else 8) for s in SHAPES}


def shape_id(s):
    return "%s-G%d-L%d-%s" % (s.variant, s.G, s.L, s.table)


def n_actions(variant):
    return 4 if variant == "v1" else 25


def row_words(A):
    """words per key: A - 1 thresholds, and for A = 4 the reserved fourth of the grid format"""
    return 4 if A == 4 else A - 1


def table_bytes(variant, G, L):
    return (1 if variant == "v1" else L) * G * G * row_words(n_actions(variant)) * 4


def thresholds(p):
    """_abi.sampling_thresholds(p, actions=A) in numpy float64: running sums by sequential adds,
    c_k = min(floor(a_k / s * 2^32 + 0.5), 2^32 - 1); A = 4 appends the reserved word 0."""
    p = np.asarray(p, np.float64)
    A = p.shape[1]
    sums = [p[:, 0].copy()]
    for k in range(1, A):
        sums.append(sums[-1] + p[:, k])
    s = sums[-1]
    c = [np.minimum(np.floor(a / s * 4294967296.0 + 0.5), 4294967295.0) for a in sums[:-1]]
    if A == 4:
        c.append(np.zeros_like(s))
    return np.stack(c, axis=1).astype(np.uint64).astype(np.uint32)


def sample_action(rows, r, n):
    """rule 3: the number of the row's first n words that the draw has reached, unsigned, whatever the row holds"""
    c = np.asarray(rows)[:, :n].astype(np.uint64)
    return (np.asarray(r, np.uint64)[:, None] >= c).sum(axis=1).astype(np.int32)


def widths(table, A):
    """[S, A]: how many of the 2^32 draws give each action under a MONOTONE table; 0 = an action of zero probability"""
    c = np.asarray(table)[:, :A - 1].astype(np.int64)
    edges = np.concatenate([np.zeros((c.shape[0], 1), np.int64), c, np.full((c.shape[0], 1), 1 << 32, np.int64)], axis=1)
    return np.diff(edges, axis=1)


def probs_of(shape, L, seed):
    """The weights of a case's policy: skewed, three entries in ten zero, one row in twenty one-hot, no row all zero."""
    rs = np.random.RandomState(seed + 2)
    S, A = L * shape.G * shape.G, n_actions(shape.variant)
    p = rs.rand(S, A) ** 4
    p[rs.rand(S, A) < 0.3] = 0.0
    hot = np.flatnonzero(rs.rand(S) < 0.05)
    p[hot] = 0.0
    p[hot, rs.randint(0, A, hot.size)] = 1.0
    p[p.sum(axis=1) == 0, 0] = 1.0
    return p


def raw_table(shape, L, seed):
    """unsorted random words: only the sum of compares gives the right action for them"""
    rs = np.random.RandomState(seed + 5)
    S, A = L * shape.G * shape.G, n_actions(shape.variant)
    return rs.randint(0, 1 << 32, (S, row_words(A)), dtype=np.uint64).astype(np.uint32)


Replay = namedtuple("Replay", "rows slots state obs visit coverage")


def replay(shape, lay, table, p, st, auto_reset, every, T=T, epoch=EPOCH, env_base=ENV_BASE, n=N):
    """T steps of the rule from st (changed in place), for the n envs from global index env_base.  rows: {name: [T,n]} of
    key, action, reward, done (v1: and the second stream); slots: [T // every, n, C, 5, 5] or None; coverage."""
    variant, G, L = shape.variant, shape.G, lay.shape[0]
    A = n_actions(variant)
    names = ("key", "action", "reward", "done") + (("foveal_reward", "foveal_done") if variant == "v1" else ())
    rows = {name: [] for name in names}
    slots = []
    cov = dict(fused_reset=0, goal=0, window_moved=0, taken=np.zeros(A, np.int64), zero_probability_taken=0)
    w = widths(table, A)
    env_global = np.uint64(env_base) + np.arange(n, dtype=np.uint64)
    st.obs.view(np.uint8)[...] = 0xEE                                  # the sentinel the device starts from
    for t in range(T):
        ep = epoch + t
        fresh = st.done.astype(bool) if auto_reset else np.zeros(n, bool)
        if auto_reset:
            O.foveal_reset(p, lay, st.done.copy(), 1, SEED, ep, st, env_base=env_base)
        key = P.keys_of(variant, G, L, st.layout_id, st.ball_xy)
        r = explore_draw(SEED, ep, env_global)[0]
        act = sample_action(table[key], r, A - 1)
        assert act.min() >= 0 and act.max() < A
        before = st.ball_xy.copy()
        O.foveal_step(p, lay, act, st)
        cov["fused_reset"] += int(fresh.sum())
        cov["goal"] += int((st.reward == np.float32(p.reward_goal)).sum())
        cov["window_moved"] += int((before != st.ball_xy).any(axis=1).sum())
        cov["taken"] += np.bincount(act, minlength=A)
        cov["zero_probability_taken"] += int((w[key, act] == 0).sum())
        rows["key"].append(key)
        rows["action"].append(act)
        for name in names[2:]:
            rows[name].append(getattr(st, name).copy())
        if every and (t + 1) % every == 0:
            slots.append(st.obs.copy())
    rows = {name: np.stack(v) for name, v in rows.items()}
    state = {name: getattr(st, name).copy() for name in STATE}
    return Replay(rows, np.stack(slots) if slots else None, state, st.obs.copy(), st.visit.copy(), cov)


def check_coverage(cov, auto_reset, min_goals=8, monotone=True):
    """what every case must show, from the oracle's side: fused resets (about 800), goal rewards, thousands of moved
    windows, every action taken at least 35 times and never one of zero probability.  monotone=False (raw random words):
    the rows are no distributions, only the resets and the moves are asked for."""
    if auto_reset:
        assert cov["fused_reset"] >= 600, cov
    else:
        assert cov["fused_reset"] == 0, cov
    assert cov["window_moved"] >= 1000, cov
    assert int(cov["taken"].sum()) == N * T
    if monotone:
        assert cov["goal"] >= min_goals, cov
        assert int(cov["taken"].min()) >= 35, cov
        assert cov["zero_probability_taken"] == 0, cov


def lay_of(shape, seed):
    """(layouts for the env or None, lay uint8[L,G,G])"""
    lays = P.layouts_of(shape, seed)
    if lays is None:
        from importlib import import_module
        spec = import_module("gym-lmaze_amd.foveal_env").FOVEAL_VARIANTS[shape.variant]
        codes = import_module("gym-lmaze_amd.layouts").to_codes
        return None, np.ascontiguousarray(np.stack([codes(t) for t in spec["layouts"]]))
    return lays, np.ascontiguousarray(np.stack(lays))


@functools.lru_cache(maxsize=None)
def case(shape, auto_reset, every, seed, raw=False):
    """(layouts for the env or None, lay, probs or None, table uint32[S, W], oracle params, the start state's copies, its visit
    map, the replay).  Shared between tests: read only."""
    lays, lay = lay_of(shape, seed)
    probs = None if raw else probs_of(shape, lay.shape[0], seed)
    table = raw_table(shape, lay.shape[0], seed) if raw else thresholds(probs)
    p, st = P.start_state(shape, lay, seed)
    start = {name: getattr(st, name).copy() for name in STATE}
    start_visit = st.visit.copy()
    out = replay(shape, lay, table, p, st, auto_reset, every)
    return lays, lay, probs, table, p, start, start_visit, out
