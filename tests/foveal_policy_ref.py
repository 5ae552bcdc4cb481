"""The closed-loop foveal rollout (lmaze_foveal_rollout_policy, include/lmaze.h) restated on the host: the C oracle
(oracle_lib.foveal_reset / foveal_step) stepped T times, with the table lookup and the exploration draw in numpy.  Needs no
GPU: test_gpu_foveal_rollout_policy.py compares the device against it, and its seeds were chosen with it alone.

A case starts from a state the oracle itself makes (reset, v1 foveal goals, a few warm-up steps for a visit map with history,
step counts spread up to a lowered limit, a fifth of the envs done), so that every path of the rule is taken inside T = 24
steps of N = 333 envs -- Replay.coverage counts them, expected_paths() says which a case must show."""
import functools
from collections import namedtuple

import numpy as np

import foveal_launch_matrix as M
import oracle_lib as O
from closed_loop_ref import explore_draw

SEED = 21
ENV_BASE = (1 << 33) + 1000          # both words of the global env index and of the epoch enter the draws
EPOCH = (1 << 35) + 77
N, T, STEP_LIMIT = 333, 24, 9
VID = {"v1": O.VARIANT_V1, "v2": O.VARIANT_V2, "v4": O.VARIANT_V4}
STATE = ("ball_xy", "goal_xy", "fgoal_xy", "layout_id", "step_count", "foveal_step_count", "reward", "foveal_reward", "done",
         "foveal_done", "ball1_xy", "fovea_xy", "last_xy", "foveal_goal")

# variant, grid, layouts (0: the variant's shipped ones), where the launcher must put the table
Shape = namedtuple("Shape", "variant G L table")
SHAPES = (Shape("v1", 14, 0, "lds"), Shape("v2", 18, 0, "lds"), Shape("v4", 18, 0, "lds"),
          Shape("v2", 12, 2, "lds"), Shape("v4", 12, 2, "lds"),       # the generic-grid kernels, padded random layouts
          Shape("v4", 24, 16, "global"))                               # 16 x 576 = 9216 bytes of table: past the 8192 of the rule


def epsilon_u32(eps):
    return min(int(np.floor(float(eps) * 2.0 ** 32)), 2 ** 32 - 1)


def n_actions(variant):
    return 4 if variant == "v1" else 25


def keys_of(variant, G, L, layout_id, ball_xy):
    """rule 2: layout row (0 for v1) and ball, each clamped into the table"""
    b = np.clip(ball_xy.astype(np.int64), 0, G - 1)
    k = b[:, 0] * G + b[:, 1]
    if variant != "v1":
        k = k + np.clip(layout_id.astype(np.int64), 0, L - 1) * (G * G)
    return k.astype(np.int32)


def select(greedy, r_x, r_y, eps_u32, A):
    """rule 3: the table's id, or floor(r.y * A / 2^32) where r.x < epsilon_u32 (epsilon_u32 == 0: never)"""
    greedy = np.asarray(greedy, dtype=np.int64)
    if eps_u32 == 0:
        return greedy.astype(np.int32), np.zeros(greedy.shape, bool)
    explored = np.asarray(r_x, np.uint64) < np.uint64(eps_u32)
    uniform = ((np.asarray(r_y, np.uint64) * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
    return np.where(explored, uniform, greedy).astype(np.int32), explored


def layouts_of(shape, seed):
    """the shape's layouts as the env takes them (None: the variant's shipped ones)"""
    return None if shape.L == 0 else M.layouts(shape.G, shape.L, seed)


def table_of(shape, L, seed):
    """a random table with about a tenth of its ids outside the action range"""
    rs = np.random.RandomState(seed + 1)
    A = n_actions(shape.variant)
    tab = rs.randint(0, A, L * shape.G * shape.G).astype(np.uint8)
    bad = rs.rand(tab.size) < 0.1
    tab[bad] = rs.choice(np.array([4, 7, 255] if shape.variant == "v1" else [25, 31, 200, 255], np.uint8), int(bad.sum()))
    return tab


def start_state(shape, lay, seed):
    """(oracle params, oracle state) a case starts from; lay uint8[L,G,G]"""
    variant, G = shape.variant, shape.G
    L = lay.shape[0]
    rs = np.random.RandomState(seed)
    p = O.foveal_params(VID[variant], G, L)
    p.step_limit = STEP_LIMIT
    st = O.FovealState(VID[variant], N, G)
    O.foveal_reset(p, lay, None, 1, SEED, EPOCH - 1, st, env_base=ENV_BASE)
    if variant == "v1":
        c = int(np.flatnonzero(lay[0].reshape(-1) == ord("X"))[0])      # v1's goal is the 'X' cell; no step or reset moves it
        st.goal_xy[...] = (c // G, c % G)
        free = np.flatnonzero((lay[0].reshape(-1) == ord("B")) | (lay[0].reshape(-1) == ord("S")))
        cells = rs.choice(free, N)                                      # anywhere in the maze: reset() alone starts everybody on 'S'
        st.ball_xy[:, 0], st.ball_xy[:, 1] = cells // G, cells % G
        O.v1_set_foveal_goal(p, lay, rs.randint(0, 5, (N, 2)).astype(np.int32), (rs.rand(N) < 0.7).astype(np.uint8), st)
    for _ in range(3):                                                  # a visit map with history (v4)
        O.foveal_step(p, lay, rs.randint(0, n_actions(variant), N).astype(np.int32), st)
    st.step_count[...] = rs.randint(0, STEP_LIMIT + 1, N)               # spread up to the limit
    st.done[...] = rs.rand(N) < 0.2
    return p, st


Replay = namedtuple("Replay", "rows slots state obs visit coverage")


def replay(shape, lay, table, p, st, eps, auto_reset, every, T=T, epoch=EPOCH):
    """T steps of the rule from st (changed in place).  rows: {name: [T,N]} of key, action, reward, done (v1: and the second
    stream); slots: [T // every, N, C, 5, 5] or None; coverage: how often each path of the rule was taken."""
    variant, G, L = shape.variant, shape.G, lay.shape[0]
    A, eps_u = n_actions(variant), epsilon_u32(eps)
    names = ("key", "action", "reward", "done") + (("foveal_reward", "foveal_done") if variant == "v1" else ())
    rows = {n: [] for n in names}
    slots = []
    cov = dict(fused_reset=0, explored=0, out_of_range=0, skipped=0, nostep=0, goal=0, window_moved=0)
    env_global = np.uint64(ENV_BASE) + np.arange(N, dtype=np.uint64)
    st.obs.view(np.uint8)[...] = 0xEE                                  # the sentinel the device starts from
    for t in range(T):
        ep = epoch + t
        fresh = st.done.astype(bool) if auto_reset else np.zeros(N, bool)
        if auto_reset:
            O.foveal_reset(p, lay, st.done.copy(), 1, SEED, ep, st, env_base=ENV_BASE)
        key = keys_of(variant, G, L, st.layout_id, st.ball_xy)
        r = explore_draw(SEED, ep, env_global) if eps_u else (None, None)
        act, explored = select(table[key], r[0], r[1], eps_u, A)
        before = st.ball_xy.copy()
        O.foveal_step(p, lay, act, st)
        bad = (act < 0) | (act >= A)
        cov["fused_reset"] += int(fresh.sum())
        cov["explored"] += int(explored.sum())
        cov["out_of_range"] += int(bad.sum())
        if variant != "v1":
            cov["skipped"] += int((bad & ~fresh).sum())
            cov["nostep"] += int((bad & fresh).sum())
        cov["goal"] += int(((st.reward == np.float32(p.reward_goal)) & ~bad).sum())
        cov["window_moved"] += int((before != st.ball_xy).any(axis=1).sum())
        rows["key"].append(key)
        rows["action"].append(act)
        for n in names[2:]:
            rows[n].append(getattr(st, n).copy())
        if every and (t + 1) % every == 0:
            slots.append(st.obs.copy())
    rows = {n: np.stack(v) for n, v in rows.items()}
    state = {n: getattr(st, n).copy() for n in STATE}
    return Replay(rows, np.stack(slots) if slots else None, state, st.obs.copy(), st.visit.copy(), cov)


def expected_paths(variant, eps, auto_reset):
    """the paths a case with these parameters must have taken (the others cannot occur in it)"""
    want = ["goal", "window_moved"]
    if auto_reset:
        want.append("fused_reset")
    if eps > 0:
        want.append("explored")
    if eps < 1:                                    # greedy steps read the table's out-of-range ids
        want.append("out_of_range")
        if variant != "v1":
            want.append("skipped")
            if auto_reset:
                want.append("nostep")
    return want


@functools.lru_cache(maxsize=None)
def case(shape, eps, auto_reset, every, seed):
    """(layouts for the env or None, lay uint8[L,G,G], table, oracle params, the start state's copies, the replay)"""
    lays = layouts_of(shape, seed)
    if lays is None:
        from importlib import import_module
        spec = import_module("gym-lmaze_amd.foveal_env").FOVEAL_VARIANTS[shape.variant]
        codes = import_module("gym-lmaze_amd.layouts").to_codes
        lay = np.ascontiguousarray(np.stack([codes(t) for t in spec["layouts"]]))
    else:
        lay = np.ascontiguousarray(np.stack(lays))
    table = table_of(shape, lay.shape[0], seed)
    p, st = start_state(shape, lay, seed)
    start = {n: getattr(st, n).copy() for n in STATE}
    start_visit = st.visit.copy()
    out = replay(shape, lay, table, p, st, eps, auto_reset, every)
    return lays, lay, table, p, start, start_visit, out


# seeds chosen on the CPU with the oracle alone so that expected_paths() holds for every (eps, auto_reset) of the shape
SEEDS = {s: 1 for s in SHAPES}
