"""The sampling closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_sample, include/lmaze.h) restated on the host: the C
oracle's v5_reset (mask = done on entry), v5_planner_step (mask = done | foveal_done on entry) and v5_step composed T times, with
the two keys, the draw and the two sums of compares in numpy.  Needs no GPU: test_gpu_hier_rollout_sample.py compares the device
against it, and its seeds were chosen with it alone (test_hier_rollout_sample_cpu.py asserts what they show).

A case starts from hier_policy_ref.start_state (N = 333, T = 24, both step limits lowered to 4, a fifth of the envs done, a fifth
locally done, a few foveal goals moved away as a loaded state may have them)."""
import functools

import numpy as np

import oracle_lib as O
from closed_loop_ref import explore_draw
from foveal_sample_ref import sample_action, thresholds
from hier_policy_ref import (CKEYS, ENV_BASE, EPOCH, FOVEAL_STEP_LIMIT, N, SEED, STATE, STEP_LIMIT, T, Replay, Shape, controller_keys,  # noqa: F401
                             layouts_of, planner_keys, slots, start_state)

LDS_RULE = 16384                     # bytes of table up to which it is staged in LDS
CROW, PROW = 4, 24                   # words per controller key (c0, c1, c2, reserved) and per planner key
KINDS = ("uniform", "peaked", "raw")

# variant, grid, layouts (0: the shipped five), where the launcher must put the planner table
SHAPES = (Shape("v5", 18, 0, "global"),        # 155 520 B
          Shape("v6", 18, 0, "global"),
          Shape("v5", 12, 1, "lds"),           # 13 824 B
          Shape("v5", 12, 2, "global"))        # 27 648 B, the generic-grid kernels
PATHS = ("fused_reset", "planned", "local_goal", "global_goal", "window_left", "step_limit", "foveal_step_limit", "visit_update",
         "clamped")


def shape_id(s):
    return "%s-G%d-L%d" % (s.variant, s.G, s.L)


def controller_table_keys(ckey, G, L):
    return 100 * L * G * G if ckey == "cell" else 100


def controller_side(shape, L, ckey):
    """where the launcher must put the controller table: 1 600 bytes, or 1 600 L G G"""
    return "lds" if controller_table_keys(ckey, shape.G, L) * CROW * 4 <= LDS_RULE else "global"


def planner_side(shape, L):
    return "lds" if L * shape.G * shape.G * PROW * 4 <= LDS_RULE else "global"


def _weights(rs, S, A, kind):
    if kind == "uniform":
        return np.ones((S, A))
    logits = rs.randn(S, A) / 0.3                                       # softmax at temperature 0.3
    w = np.exp(logits - logits.max(axis=1, keepdims=True))
    w[rs.rand(S, A) < 0.2] = 0.0                                        # adjacent thresholds equal: actions never drawn
    w[w.sum(axis=1) == 0, 0] = 1.0
    return w


def _raw(rs, S, W):
    """arbitrary words: unsorted rows, one row in twenty all zero, one in twenty all 0xFFFFFFFF; nothing is validated"""
    t = rs.randint(0, 1 << 32, (S, W), dtype=np.uint64).astype(np.uint32)
    pick = rs.rand(S)
    t[pick < 0.05] = 0
    t[pick > 0.95] = 0xFFFFFFFF
    return t


def tables_of(shape, L, ckey, kind, seed):
    """(controller uint32[keys, 4], planner uint32[L G G, 24], controller weights or None, planner weights or None)"""
    rs = np.random.RandomState(seed * 7 + 3 + KINDS.index(kind))
    K, S = controller_table_keys(ckey, shape.G, L), L * shape.G * shape.G
    if kind == "raw":
        return _raw(rs, K, CROW), _raw(rs, S, PROW), None, None
    cw, pw = _weights(rs, K, 4, kind), _weights(rs, S, 25, kind)
    return thresholds(cw), thresholds(pw), cw, pw


def replay(shape, lay, ckey, controller, planner, p, st, T=T, epoch=EPOCH):
    """T steps of the rule from st (changed in place).  rows: {name: [T,N]}; obs_t / obs_local_t: the observations after EVERY
    step ([T,N,...]: slot j of obs_every = k is entry (j + 1) k - 1); coverage: how often each path was taken, and how often
    each action and each goal."""
    G, L = shape.G, lay.shape[0]
    names = ("key", "action", "goal", "goal_key", "reward", "done", "foveal_reward", "foveal_done")
    rows = {n: [] for n in names}
    obs_t, obs_local_t = [], []
    cov = dict.fromkeys(PATHS, 0)
    cov["actions"], cov["goals"] = np.zeros(4, np.int64), np.zeros(25, np.int64)
    env_global = np.uint64(ENV_BASE) + np.arange(N, dtype=np.uint64)
    st.obs.view(np.uint8)[...] = 0xEE                                  # the sentinel the device starts from
    st.obs_local.view(np.uint8)[...] = 0xEE
    for t in range(T):
        ep = epoch + t
        gd, ld = st.done.astype(bool), st.foveal_done.astype(bool)
        r = explore_draw(SEED, ep, env_global)                                                       # 1. on every env-step
        O.v5_reset(p, lay, gd.astype(np.uint8), 1, SEED, ep, st, env_base=ENV_BASE)                  # 2.
        plan = gd | ld                                                                               # 3.
        kp = planner_keys(G, L, st.layout_id, st.ball_xy)
        g = sample_action(planner[kp], r[2], PROW)
        assert g.min() >= 0 and g.max() <= 24
        O.v5_planner_step(p, lay, np.where(plan, g, 0).astype(np.int32), plan.astype(np.uint8), st)
        kc, raw = controller_keys(ckey, G, L, st.layout_id, st.ball_xy, st.fgoal_xy)                 # 4.
        a = sample_action(controller[kc], r[0], 3)                                                   # 5. the reserved word is not compared
        assert a.min() >= 0 and a.max() <= 3
        before, f1 = st.ball_xy.copy(), st.fovea_xy[:, 2:4].copy()
        O.v5_step(p, lay, a, st)
        moved = (before != st.ball_xy).any(axis=1)
        at_goal = (st.ball_xy == st.fgoal_xy).all(axis=1)
        outside = ((st.ball_xy[:, 0] < f1[:, 0] - 3) | (st.ball_xy[:, 0] > f1[:, 0] + 2) | (st.ball_xy[:, 1] < f1[:, 1] - 3) |
                   (st.ball_xy[:, 1] > f1[:, 1] + 2))
        cov["fused_reset"] += int(gd.sum())
        cov["planned"] += int(plan.sum())
        cov["local_goal"] += int((st.foveal_reward == np.float32(p.reward_goal)).sum())
        cov["global_goal"] += int((st.reward == np.float32(p.reward_goal)).sum())
        cov["window_left"] += int((moved & ~at_goal & outside).sum())
        cov["step_limit"] += int((st.step_count >= p.step_limit).sum())
        cov["foveal_step_limit"] += int(((st.foveal_step_count >= p.foveal_step_limit) & (st.done != 0)).sum())
        cov["visit_update"] += int((st.foveal_done != 0).sum())
        cov["clamped"] += int(((raw < 0) | (raw > 9)).any(axis=1).sum())
        cov["actions"] += np.bincount(a, minlength=4)
        cov["goals"] += np.bincount(g[plan], minlength=25)
        rows["key"].append(kc)
        rows["action"].append(a)
        rows["goal"].append(np.where(plan, g, -1).astype(np.int32))
        rows["goal_key"].append(np.where(plan, kp, -1).astype(np.int32))
        for n in names[4:]:
            rows[n].append(getattr(st, n).copy())
        obs_t.append(st.obs.copy())
        obs_local_t.append(st.obs_local.copy())
    rows = {n: np.stack(v) for n, v in rows.items()}
    state = {n: getattr(st, n).copy() for n in STATE}
    return Replay(rows, np.stack(obs_t), np.stack(obs_local_t), state, st.obs.copy(), st.obs_local.copy(), st.visit.copy(), cov)


def check_coverage(cov, kind):
    """what every case must show, from the oracle's side alone"""
    for path in PATHS:
        assert cov[path] > 0, (path, cov)
    assert (cov["actions"] > 0).all(), cov
    if kind != "raw":
        assert int((cov["goals"] > 0).sum()) >= 20, cov


@functools.lru_cache(maxsize=None)
def lay_of(shape, seed):
    """(layouts for the env or None, lay uint8[L,G,G])"""
    lays = layouts_of(shape, seed)
    if lays is None:
        from importlib import import_module
        spec = import_module("gym-lmaze_amd.foveal_env").FOVEAL_VARIANTS[shape.variant]
        codes = import_module("gym-lmaze_amd.layouts").to_codes
        return None, np.ascontiguousarray(np.stack([codes(t) for t in spec["layouts"]]))
    return lays, np.ascontiguousarray(np.stack(lays))


@functools.lru_cache(maxsize=None)
def case(shape, ckey, kind, seed):
    """(layouts for the env or None, lay, controller, planner, oracle params, the start state's copies, its visit map, the
    replay) -- shared: read only"""
    lays, lay = lay_of(shape, seed)
    controller, planner, _, _ = tables_of(shape, lay.shape[0], ckey, kind, seed)
    p, st = start_state(shape, lay, seed)
    start = {n: getattr(st, n).copy() for n in STATE}
    start_visit = st.visit.copy()
    out = replay(shape, lay, ckey, controller, planner, p, st)
    return lays, lay, controller, planner, p, start, start_visit, out


# seeds chosen on the CPU with the oracle alone so that check_coverage() holds for every kind and both controller keys of the shape
SEEDS = {s: 1 for s in SHAPES}
