"""The closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_policy, include/lmaze.h) restated on the host: the C oracle's
v5_reset (mask = done on entry), v5_planner_step (mask = done | foveal_done on entry) and v5_step composed T times, with the two
table lookups and the exploration draw in numpy.  Needs no GPU: test_gpu_hier_rollout_policy.py compares the device against it,
and its seeds were chosen with it alone.

A case starts from a state the oracle itself makes (reset, a few two-level warm-up steps for a visit map with history, step
counts spread up to the lowered limits, a fifth of the envs done, a fifth locally done, a few foveal goals moved away as a loaded
state may have them), so that every path of the rule is taken inside T = 24 steps of N = 333 envs -- Replay.coverage counts them,
expected_paths() says which a case must show."""
import functools
from collections import namedtuple

import numpy as np

import foveal_launch_matrix as M
import oracle_lib as O
from closed_loop_ref import explore_draw
from foveal_policy_ref import epsilon_u32, keys_of, select

SEED = 21
ENV_BASE = (1 << 33) + 1000          # both words of the global env index and of the epoch enter the draws
EPOCH = (1 << 35) + 77
N, T = 333, 24
STEP_LIMIT, FOVEAL_STEP_LIMIT = 4, 4  # lowered: the local limit (sc >= 4) and the global one (fsc >= 4) both fire inside T
VID = {"v5": O.VARIANT_V5, "v6": O.VARIANT_V6}
STATE = ("ball_xy", "goal_xy", "fgoal_xy", "layout_id", "step_count", "foveal_step_count", "reward", "foveal_reward", "done",
         "foveal_done", "ball1_xy", "fovea_xy", "last_xy", "foveal_goal")
CKEYS = ("offset", "cell")
EPS = ((0.0, 0.0), (0.25, 0.5), (1.0, 1.0))          # (controller, planner)

# variant, grid, layouts (0: the shipped ones), where the launcher must put the planner table
Shape = namedtuple("Shape", "variant G L planner")
SHAPES = (Shape("v5", 18, 0, "lds"), Shape("v6", 18, 0, "lds"),
          Shape("v5", 12, 2, "lds"),                                   # the generic-grid kernels, padded random layouts
          Shape("v5", 24, 16, "global"))                               # 16 x 576 = 9216 bytes of planner table: past the 8192 of the rule


def controller_side(shape, L, ckey):
    """where the launcher must put the controller table: 100 bytes, or 100 L G G"""
    return "lds" if (100 if ckey == "offset" else 100 * L * shape.G * shape.G) <= 8192 else "global"


def planner_keys(G, L, layout_id, ball_xy):
    """rule 3: the rule of state_keys()"""
    return keys_of("v5", G, L, layout_id, ball_xy)


def offsets(fgoal_xy, ball_xy):
    """rule 4: (d, the offsets before the clamp)"""
    raw = fgoal_xy.astype(np.int64) - ball_xy.astype(np.int64) + 4
    o = np.clip(raw, 0, 9)
    return (o[:, 0] * 10 + o[:, 1]).astype(np.int64), raw


def controller_keys(ckey, G, L, layout_id, ball_xy, fgoal_xy):
    d, raw = offsets(fgoal_xy, ball_xy)
    if ckey == "cell":
        d = d + planner_keys(G, L, layout_id, ball_xy).astype(np.int64) * 100
    return d.astype(np.int32), raw


def layouts_of(shape, seed):
    """the shape's layouts as the env takes them (None: the shipped ones)"""
    return None if shape.L == 0 else M.layouts(shape.G, shape.L, seed)


def tables_of(shape, L, ckey, seed):
    """random (controller, planner) tables with about a tenth of their ids out of range: > 3 and > 24"""
    rs = np.random.RandomState(seed + 1)
    cells = L * shape.G * shape.G
    ctl = rs.randint(0, 4, 100 * cells if ckey == "cell" else 100).astype(np.uint8)
    bad = rs.rand(ctl.size) < 0.1
    ctl[bad] = rs.choice(np.array([4, 7, 255], np.uint8), int(bad.sum()))
    pln = rs.randint(0, 25, cells).astype(np.uint8)
    bad = rs.rand(pln.size) < 0.1
    pln[bad] = rs.choice(np.array([25, 31, 200, 255], np.uint8), int(bad.sum()))
    return ctl, pln


def start_state(shape, lay, seed):
    """(oracle params, oracle state) a case starts from; lay uint8[L,G,G]"""
    G, L = shape.G, lay.shape[0]
    rs = np.random.RandomState(seed)
    p = O.foveal_params(VID[shape.variant], G, L)
    p.step_limit, p.foveal_step_limit = STEP_LIMIT, FOVEAL_STEP_LIMIT
    st = O.FovealState(VID[shape.variant], N, G)
    O.v5_reset(p, lay, None, 1, SEED, EPOCH - 8, st, env_base=ENV_BASE)
    for w in range(6):                                                  # a visit map with history (updated on localDone)
        O.v5_hier_step(p, lay, rs.randint(0, 4, N).astype(np.int32), rs.randint(0, 25, N).astype(np.int32), SEED, EPOCH - 7 + w,
                       st, env_base=ENV_BASE)
    st.step_count[...] = rs.randint(0, STEP_LIMIT, N)                   # spread up to the limits
    st.foveal_step_count[...] = rs.randint(1, FOVEAL_STEP_LIMIT, N)
    st.done[...] = rs.rand(N) < 0.2
    st.foveal_done[...] = rs.rand(N) < 0.2
    far = rs.rand(N) < 0.05                                             # a loaded state: foveal goals outside the offset range
    st.fgoal_xy[far] += rs.choice(np.array([-9, -7, 7, 11], np.int32), (int(far.sum()), 2))
    return p, st


Replay = namedtuple("Replay", "rows obs_t obs_local_t state obs obs_local visit coverage")
PATHS = ("fused_reset", "planned", "plan_explored", "plan_skipped", "ctrl_explored", "no_move", "local_goal", "global_goal",
         "window_left", "step_limit", "foveal_step_limit", "visit_update", "clamped")


def replay(shape, lay, ckey, controller, planner, p, st, eps, peps, T=T, epoch=EPOCH):
    """T steps of the rule from st (changed in place).  rows: {name: [T,N]}; obs_t / obs_local_t: the observations after
    EVERY step ([T,N,...]: slot j of obs_every = k is entry (j + 1) k - 1); coverage: how often each path was taken."""
    G, L = shape.G, lay.shape[0]
    eps_u, peps_u = epsilon_u32(eps), epsilon_u32(peps)
    names = ("key", "action", "goal", "goal_key", "reward", "done", "foveal_reward", "foveal_done")
    rows = {n: [] for n in names}
    obs_t, obs_local_t = [], []
    cov = dict.fromkeys(PATHS, 0)
    env_global = np.uint64(ENV_BASE) + np.arange(N, dtype=np.uint64)
    st.obs.view(np.uint8)[...] = 0xEE                                  # the sentinel the device starts from
    st.obs_local.view(np.uint8)[...] = 0xEE
    zero = np.zeros(N, np.uint64)
    for t in range(T):
        ep = epoch + t
        gd, ld = st.done.astype(bool), st.foveal_done.astype(bool)
        r = explore_draw(SEED, ep, env_global) if (eps_u | peps_u) else (zero, zero, zero, zero)   # 1. one draw, or none
        O.v5_reset(p, lay, gd.astype(np.uint8), 1, SEED, ep, st, env_base=ENV_BASE)                  # 2.
        plan = gd | ld                                                                               # 3.
        kp = planner_keys(G, L, st.layout_id, st.ball_xy)
        g, p_explored = select(planner[kp], r[2], r[3], peps_u, 25)
        O.v5_planner_step(p, lay, np.where(plan, g, 0).astype(np.int32), plan.astype(np.uint8), st)
        kc, raw = controller_keys(ckey, G, L, st.layout_id, st.ball_xy, st.fgoal_xy)                 # 4.
        a, c_explored = select(controller[kc], r[0], r[1], eps_u, 4)                                 # 5.
        before, f1 = st.ball_xy.copy(), st.fovea_xy[:, 2:4].copy()
        O.v5_step(p, lay, a, st)
        moved = (before != st.ball_xy).any(axis=1)
        at_goal = (st.ball_xy == st.fgoal_xy).all(axis=1)
        outside = ((st.ball_xy[:, 0] < f1[:, 0] - 3) | (st.ball_xy[:, 0] > f1[:, 0] + 2) | (st.ball_xy[:, 1] < f1[:, 1] - 3) |
                   (st.ball_xy[:, 1] > f1[:, 1] + 2))
        cov["fused_reset"] += int(gd.sum())
        cov["planned"] += int((plan & (g <= 24)).sum())
        cov["plan_explored"] += int((plan & p_explored).sum())
        cov["plan_skipped"] += int((plan & (g > 24)).sum())
        cov["ctrl_explored"] += int(c_explored.sum())
        cov["no_move"] += int((a > 3).sum())
        cov["local_goal"] += int((st.foveal_reward == np.float32(p.reward_goal)).sum())
        cov["global_goal"] += int((st.reward == np.float32(p.reward_goal)).sum())
        cov["window_left"] += int((moved & ~at_goal & outside).sum())
        cov["step_limit"] += int((st.step_count >= p.step_limit).sum())
        cov["foveal_step_limit"] += int(((st.foveal_step_count >= p.foveal_step_limit) & (st.done != 0)).sum())
        cov["visit_update"] += int((st.foveal_done != 0).sum())
        cov["clamped"] += int(((raw < 0) | (raw > 9)).any(axis=1).sum())
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


def slots(per_step, every):
    """the slots obs_every = every fills, of the per-step record"""
    return np.ascontiguousarray(per_step[every - 1::every][:per_step.shape[0] // every])


def expected_paths(eps, peps):
    """the paths a case with these rates must have taken (the others cannot occur in it)"""
    want = ["fused_reset", "planned", "local_goal", "global_goal", "window_left", "step_limit", "foveal_step_limit", "visit_update",
            "clamped"]
    if peps > 0:
        want.append("plan_explored")
    if peps < 1:                                   # greedy plannerSteps read the table's out-of-range ids
        want.append("plan_skipped")
    if eps > 0:
        want.append("ctrl_explored")
    if eps < 1:
        want.append("no_move")
    return want


@functools.lru_cache(maxsize=None)
def setup(shape, ckey, seed):
    """(layouts for the env or None, lay uint8[L,G,G], controller, planner)"""
    lays = layouts_of(shape, seed)
    if lays is None:
        from importlib import import_module
        spec = import_module("gym-lmaze_amd.foveal_env").FOVEAL_VARIANTS[shape.variant]
        codes = import_module("gym-lmaze_amd.layouts").to_codes
        lay = np.ascontiguousarray(np.stack([codes(t) for t in spec["layouts"]]))
    else:
        lay = np.ascontiguousarray(np.stack(lays))
    controller, planner = tables_of(shape, lay.shape[0], ckey, seed)
    return lays, lay, controller, planner


@functools.lru_cache(maxsize=None)
def case(shape, ckey, eps, peps, seed):
    """(layouts for the env or None, lay, controller, planner, oracle params, the start state's copies, the replay) -- shared:
    read only"""
    lays, lay, controller, planner = setup(shape, ckey, seed)
    p, st = start_state(shape, lay, seed)
    start = {n: getattr(st, n).copy() for n in STATE}
    start_visit = st.visit.copy()
    out = replay(shape, lay, ckey, controller, planner, p, st, eps, peps)
    return lays, lay, controller, planner, p, start, start_visit, out


# seeds chosen on the CPU with the oracle alone so that expected_paths() holds for every (eps, planner eps) and both controller
# keys of the shape
SEEDS = {s: 1 for s in SHAPES}
