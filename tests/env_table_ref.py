"""The closed-loop rollouts with a table per env (include/lmaze.h lmaze_env_rollout_policy / lmaze_env_rollout_sample;
rollout_policy(key="env") / rollout_sample(key="env")) restated on the host: the key rule i * G*G + ball cell, random tables
per env, the replay of one call against the C oracle stepped T times, and the plan-then-act case on the oracle's own model
of every maze.  The draws, the sampling rule and the envs are closed_loop_ref.py's.  Importing it needs no GPU."""
import functools

import numpy as np
import torch

import oracle_lib as O
import solve_ref as SR
from closed_loop_ref import DEV, explore_draw, layouts, make_env, philox, sample_action, to_numpy  # noqa: F401
from helpers import bordered_random_layouts, f32_bits, random_free_cells


# ------------------------------------------------------------- the tables: random per env, so a neighbour's row shows at once
def policy_tables(N, G, seed):
    """uint8[N, G*G]: mostly the four moves, some ids no step knows (no move): 4, 7, 200, 255."""
    rs = np.random.RandomState(seed)
    n = N * G * G
    return np.where(rs.rand(n) < 0.9, rs.randint(0, 4, n), rs.choice([4, 7, 200, 255], n)).astype(np.uint8).reshape(N, G * G)


def threshold_tables(N, G, seed):
    """uint32[N, G*G, 4]: cumulative rows, and every third row as drawn -- not monotone; word 3 is noise."""
    rs = np.random.RandomState(seed)
    rows = rs.randint(0, 1 << 32, (N * G * G, 4), dtype=np.uint64).astype(np.uint32)
    mono = np.arange(len(rows)) % 3 != 0
    rows[mono, :3] = np.sort(rows[mono, :3], axis=1)
    assert (np.diff(rows[~mono, :3].astype(np.int64), axis=1) < 0).any()
    return rows.reshape(N, G * G, 4)


def env_keys(ball_xy, G, first=0):
    """i * G*G + clamp(ball_x) * G + clamp(ball_y) for the envs first, first + 1, ..."""
    b = np.clip(ball_xy, 0, G - 1)
    return ((np.arange(len(b), dtype=np.int64) + first) * G * G + b[:, 0] * G + b[:, 1]).astype(np.int32)


def epsilon_greedy(entry, eps32, rx, ry):
    """The epsilon-greedy decision alone, a pure function of (table entry, eps32, r.x, r.y) as arrays or scalars: explore when
    r.x < eps32 and then take r.y >> 30, else the entry.  Returns (action int32, explore bool).  policy_law.py counts the
    draws of every action through this function; greedy_action() below replays the GPU with it."""
    entry = np.asarray(entry).astype(np.int32)
    rx, ry = np.asarray(rx, dtype=np.uint64), np.asarray(ry, dtype=np.uint64)
    explore = rx < np.uint64(eps32)
    return np.where(explore, (ry >> np.uint64(30)).astype(np.int32), entry).astype(np.int32), explore


def greedy_action(table, eps32, seed, epoch0):
    """action(key, t, env_global) of rollout_policy(key="env"): the flat table's entry, or, exploring, r.y >> 30.
    .explored counts the exploring env-steps."""
    flat = np.ascontiguousarray(table).reshape(-1)

    def action(key_ref, t, eg):
        act = flat[key_ref].astype(np.int32)
        if eps32:
            r = explore_draw(seed, epoch0 + t, eg)
            act, explore = epsilon_greedy(act, eps32, r[0], r[1])
            action.explored += int(explore.sum())
        return act
    action.explored = 0
    return action


def sampled_action(rows, seed, epoch0):
    flat = np.ascontiguousarray(rows).reshape(-1, 4)

    def action(key_ref, t, eg):
        return sample_action(flat[key_ref], explore_draw(seed, epoch0 + t, eg)[0])
    return action


# ------------------------------------------------------------- one call against the oracle
def replay(env, lay, kind, T, auto_reset, k, rollout, action, window=None):
    """closed_loop_ref.replay with the env key: one rollout of env against the oracle stepped T times from the env's
    host_state().  rollout(obs_t) makes the call (trajectory=True, obs_every=k) and returns what it returned; action(key,
    t, env_global) is the policy restated.  window = (first env, count): the oracle replays that range of the batch only.
    Every step's key, action, reward bits and done, every recorded slot, the final state byte for byte and the final planes
    are compared.  Returns the call's rows as numpy, its outputs and the number of resets."""
    N, G, v3 = env.num_envs, env.grid, env.variant == "v3"
    lo, cnt = window if window else (0, N)
    sl = slice(lo, lo + cnt)
    st = {name: np.array(v[sl], copy=True) for name, v in env.host_state().items()}
    p = O.params(O.VARIANT_V3 if v3 else O.VARIANT_V0, G, O.LAYOUT_PER_ENV if kind == "per_env" else O.LAYOUT_SHARED,
                 env.step_limit, *env.rewards)
    lay_c = np.ascontiguousarray(lay[sl] if kind == "per_env" else lay)
    epoch0 = env._epoch
    S = T // k if k else 0
    obs_t = torch.full((S, N, G, G), 113, dtype=env.obs.dtype, device=DEV) if k else None
    env.obs.fill_(113)
    out = rollout(obs_t)
    assert len(out) == 7 and env._epoch == epoch0 + T
    reward_t, done_t, actions_t, key_t = (np.ascontiguousarray(to_numpy(x[:, sl])) for x in out[3:])
    slots = np.ascontiguousarray(to_numpy(obs_t[:, sl])) if k else None
    obs_ref = np.zeros((cnt, G, G), np.int32)
    eg = np.arange(cnt, dtype=np.uint64) + np.uint64(env.env_base + lo)          # the draws go by the global index,
    n_reset = 0
    for t in range(T):
        if auto_reset and st["done"].any():
            n_reset += int(st["done"].sum())
            O.reset(p, lay_c, st["done"].copy(), env.seed, epoch0 + t, st["ball_xy"], st["goal_xy"], st["step_count"],
                    st["reward"], st["done"], env_base=env.env_base + lo)
        key_ref = env_keys(st["ball_xy"], G, first=lo)                            # the rows by the local one
        act = action(key_ref, t, eg)
        if v3:
            O.step_v3(p, lay_c, act, st["ball_xy"], st["goal_xy"], st["step_count"], st["reward"], st["done"], obs_ref)
        else:
            O.step_v0(p, lay_c, act, st["ball_xy"], st["step_count"], st["reward"], st["done"], st["goal_count"], obs_ref)
        assert (key_t[t] == key_ref).all(), ("key", t)
        assert (actions_t[t] == act).all(), ("action", t)
        assert (f32_bits(reward_t[t]) == f32_bits(st["reward"])).all(), ("reward", t)
        assert (done_t[t].view(np.uint8) == st["done"]).all(), ("done", t)
        if k and (t + 1) % k == 0:
            assert (slots[(t + 1) // k - 1] == obs_ref.astype(slots.dtype)).all(), ("slot", t)
    if T:
        h = env.host_state()
        for name in h:
            assert (np.ascontiguousarray(h[name][sl]).view(np.uint8) == np.ascontiguousarray(st[name]).view(np.uint8)).all(), name
        got = to_numpy(env.obs[sl])
        assert (got == obs_ref.astype(got.dtype)).all(), "final planes"
    if k and T % k:
        assert slots.shape[0] == T // k
    return dict(rows=(reward_t, done_t, actions_t, key_t), out=out, resets=n_reset)


# ------------------------------------------------------------- plan, then act: on the oracle's own model of every maze
PLAN_N = 777
PLAN_GAMMA, PLAN_SWEEPS = 0.99, 4096


@functools.lru_cache(maxsize=None)
def plan_case(variant, G):
    """PLAN_N random mazes, a start cell in each (not 'W', not 'X') and, v3, a goal cell (not 'W'): the model of every maze
    extracted from the oracle (solve_ref), the fewest steps to done from every cell, and T, the largest finite one among
    the starts.  Read only."""
    lay = bordered_random_layouts(PLAN_N, G, 900 + G)
    start = random_free_cells(lay, 5 + G)
    goals = random_free_cells(lay, 7 + G, forbid=(ord("W"),)) if variant == "v3" else None
    models = SR.models_of(variant, lay, goals)
    dist = np.stack([SR.steps_to_done(m) for m in models])
    cell = start[:, 0] * G + start[:, 1]
    d0 = dist[np.arange(PLAN_N), cell]
    return dict(lay=lay, start=start, goals=goals, models=models, cell=cell, dist=d0, T=int(d0[np.isfinite(d0)].max()))


def follow(case, policy, T):
    """int[N]: the step (0-based) of every env's first done when env i follows policy[i] (uint8[N, G*G]) on its own model
    from its start cell for T steps, -1 where it never gets there.  Ids above 3 and sticky pairs do not move."""
    models = case["models"]
    nxt = np.stack([m.nxt for m in models])
    terminal = np.stack([m.terminal for m in models])
    sticky = np.stack([m.sticky for m in models])
    i = np.arange(len(models))
    s = case["cell"].copy()
    first = np.full(len(models), -1)
    for t in range(T):
        a = policy[i, s].astype(np.int64)
        moves = a < 4
        a = np.minimum(a, 3)
        moves &= ~sticky[i, s, a]
        done = moves & terminal[i, s, a]
        first[(first < 0) & done] = t
        s = np.where(moves, nxt[i, s, a], s)
    return first


def missed(case, first):
    """bool over the reachable envs: the first done is not at the fewest steps"""
    reach = np.isfinite(case["dist"])
    return first[reach] != case["dist"][reach] - 1
