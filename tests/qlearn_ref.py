"""Q-learning inside the one-launch rollout (include/lmaze.h lmaze_env_rollout_qlearn; rollout_qlearn()) restated on the host:
the C oracle stepped T times, as env_table_ref.replay does, and the float32 update spelled with explicit np.float32
operations -- the first maximum by a chain of strict '>' (never argmax / max), the product rounded before the sum.  The
draws are closed_loop_ref.py's.  Importing it needs no GPU."""
import functools

import numpy as np

import oracle_lib as O
import solve_ref as SR
from closed_loop_ref import explore_draw
from helpers import bordered_random_layouts, f32_bits


# ------------------------------------------------------------- the arithmetic of csrc/lmaze_learn.h
def first_max(rows):
    """(value float32[n], action int32[n]) of rows float32[n, 4]: the first maximum by a strict > from action 0 on.  A NaN
    never wins a compare and nothing beats a NaN in column 0."""
    rows = np.asarray(rows, dtype=np.float32)
    best = rows[:, 0].copy()
    act = np.zeros(len(rows), np.int32)
    with np.errstate(invalid="ignore"):
        for a in (1, 2, 3):
            better = rows[:, a] > best
            best = np.where(better, rows[:, a], best)
            act = np.where(better, np.int32(a), act)
    return best.astype(np.float32), act.astype(np.int32)


def q_target(r, done, gamma, v_next):
    """r where done, else r + gamma * v_next: the product rounded to float32, then the sum"""
    r, v_next = np.asarray(r, dtype=np.float32), np.asarray(v_next, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        boot = (np.float32(gamma) * v_next).astype(np.float32)
        return np.where(np.asarray(done) != 0, r, (r + boot).astype(np.float32)).astype(np.float32)


def q_update(q_sa, alpha, target):
    """(q_sa + alpha * (target - q_sa), target - q_sa): three float32 roundings"""
    q_sa, target = np.asarray(q_sa, dtype=np.float32), np.asarray(target, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        delta = (target - q_sa).astype(np.float32)
        step = (np.float32(alpha) * delta).astype(np.float32)
        return (q_sa + step).astype(np.float32), delta


# ------------------------------------------------------------- T steps of N learners on the oracle
def learn(variant, G, kind, lay, st, q, T, alpha, gamma, eps32, auto_reset, seed, epoch0, env_base, step_limit=100,
          rewards=SR.DEFAULT_REWARDS, first=0, k=0):
    """T steps of the rule of include/lmaze.h on the host state st (a dict of numpy arrays as host_state() gives them,
    stepped in place) and the table q float32[n, G*G, 4] (updated in place; row 0 is env `first` of the batch whose keys the
    rows name).  The draws go by env_base + i.  Returns the rows [T, n] -- key, act, reward, done, td -- the slots recorded
    every k steps, the planes after the last step and the number of resets."""
    v3 = variant == "v3"
    n, S = len(st["ball_xy"]), G * G
    assert q.shape == (n, S, 4) and q.dtype == np.float32
    p = O.params(O.VARIANT_V3 if v3 else O.VARIANT_V0, G, O.LAYOUT_PER_ENV if kind == "per_env" else O.LAYOUT_SHARED, step_limit,
                 *rewards)
    lay_c = np.ascontiguousarray(lay)
    rows = {name: np.zeros((T, n), dt) for name, dt in (("key", np.int32), ("act", np.int32), ("reward", np.float32),
                                                        ("done", np.uint8), ("td", np.float32))}
    obs = np.zeros((n, G, G), np.int32)
    slots, resets = [], 0
    eg = np.arange(n, dtype=np.uint64) + np.uint64(env_base)
    i = np.arange(n)
    for t in range(T):
        if auto_reset and st["done"].any():
            resets += int(st["done"].sum())
            O.reset(p, lay_c, st["done"].copy(), seed, epoch0 + t, st["ball_xy"], st["goal_xy"], st["step_count"], st["reward"],
                    st["done"], env_base=env_base)
        b = np.clip(st["ball_xy"], 0, G - 1)
        c = b[:, 0] * G + b[:, 1]
        _, act = first_max(q[i, c])
        if eps32:
            r = explore_draw(seed, epoch0 + t, eg)
            act = np.where(r[0] < np.uint64(eps32), (r[1] >> np.uint64(30)).astype(np.int32), act).astype(np.int32)
        act = np.ascontiguousarray(act, dtype=np.int32)
        if v3:
            O.step_v3(p, lay_c, act, st["ball_xy"], st["goal_xy"], st["step_count"], st["reward"], st["done"], obs)
        else:
            O.step_v0(p, lay_c, act, st["ball_xy"], st["step_count"], st["reward"], st["done"], st["goal_count"], obs)
        c2 = st["ball_xy"][:, 0] * G + st["ball_xy"][:, 1]
        v_next, _ = first_max(q[i, c2])                                # the table as it stands before this step's write
        target = q_target(st["reward"], st["done"], gamma, v_next)
        q[i, c, act], delta = q_update(q[i, c, act], alpha, target)
        rows["key"][t], rows["act"][t], rows["td"][t] = ((i + first) * S + c).astype(np.int32), act, delta
        rows["reward"][t], rows["done"][t] = st["reward"], st["done"]
        if k and (t + 1) % k == 0:
            slots.append(obs.copy())
    return dict(rows=rows, slots=slots, obs=obs, resets=resets)


def replay(env, lay, kind, T, q, alpha, gamma, epsilon, auto_reset, k, rollout, td=True):
    """One rollout_qlearn() call of env against learn() from the env's host_state().  q: the device table [N, G*G, 4];
    rollout(obs_t, td_t) makes the call (obs_every=k) and returns what it returned.  Everything is compared bit for bit: the
    table afterwards, td_t, the actions_t / key_t / reward_t / done_t rows, the recorded slots, the final state byte for byte
    and the final planes.  Returns learn()'s result and the call's outputs."""
    import torch
    from closed_loop_ref import DEV, to_numpy
    N, G = env.num_envs, env.grid
    st = {name: np.array(v, copy=True) for name, v in env.host_state().items()}
    q_ref = np.array(to_numpy(q), copy=True).reshape(N, G * G, 4)
    epoch0 = env._epoch
    eps32 = min(int(float(epsilon) * 4294967296.0), 4294967295)
    S = T // k if k else 0
    obs_t = torch.full((S, N, G, G), 113, dtype=env.obs.dtype, device=DEV) if k else None
    td_t = torch.full((T, N), 7.0, dtype=torch.float32, device=DEV) if td else None
    env.obs.fill_(113)
    out = rollout(obs_t, td_t)
    assert len(out) == 7 and env._epoch == epoch0 + T
    ref = learn(env.variant, G, kind, lay, st, q_ref, T, alpha, gamma, eps32, auto_reset, env.seed, epoch0, env.env_base,
                env.step_limit, env.rewards, k=k)
    reward_t, done_t, actions_t, key_t = (to_numpy(x) for x in out[3:])
    r = ref["rows"]
    assert (key_t == r["key"]).all() and (actions_t == r["act"]).all()
    assert (f32_bits(reward_t) == f32_bits(r["reward"])).all() and (done_t.view(np.uint8) == r["done"]).all()
    if td:
        assert (f32_bits(to_numpy(td_t)) == f32_bits(r["td"])).all(), "td_t"
    assert (f32_bits(to_numpy(q).reshape(N, G * G, 4)) == f32_bits(q_ref)).all(), "q"
    if k:
        assert obs_t.shape[0] == len(ref["slots"]) == T // k
        for j, want in enumerate(ref["slots"]):
            assert (to_numpy(obs_t[j]) == want).all(), ("slot", j)
    if T:
        h = env.host_state()
        for name in h:
            assert (np.ascontiguousarray(h[name]).view(np.uint8) == np.ascontiguousarray(st[name]).view(np.uint8)).all(), name
        assert (to_numpy(env.obs) == ref["obs"]).all(), "final planes"
    return ref, out


# ------------------------------------------------------------- tables and mazes of the tests
def random_table(N, G, seed):
    """float32[N, G*G, 4]: finite values of both signs from a small set, so ties are everywhere; no NaN, no -0.0"""
    rs = np.random.RandomState(seed)
    return rs.choice(np.array([-2.0, -0.5, 0.0, 0.25, 0.25, 1.0, 3.5], np.float32), (N, G * G, 4)).astype(np.float32)


def pocket_layouts(N, G=8):
    """uint8[N, G, G]: 'W' border, a 5x5 interior block of free cells -- and one cell of it, another in every maze, walled in
    on all four sides.  Returns (layouts, the pocket cells int32[N, 2])."""
    assert G == 8
    lay = np.full((N, G, G), ord("W"), np.uint8)
    lay[:, 1:6, 1:6] = ord("B")
    cell = np.zeros((N, 2), np.int32)
    for i in range(N):
        x, y = 2 + i % 3, 2 + (i // 3) % 3
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            lay[i, x + dx, y + dy] = ord("W")
        cell[i] = (x, y)
    lay[:, 1, 1] = ord("S")
    lay[:, 5, 5] = ord("X")
    return lay, cell


# ------------------------------------------------------------- it learns: the case of the GPU test, computed once on the CPU
LEARN_N, LEARN_G, LEARN_SEED, LEARN_LAYOUT_SEED = 24, 8, 33, 4242
LEARN_ALPHA, LEARN_GAMMA, LEARN_EPSILON, LEARN_T, LEARN_LAUNCHES = 0.5, 0.99, 0.2, 64, 64
LEARN_ENV_BASE, LEARN_EPOCH = 0, 1


def learn_start(N):
    """Every env done, so the first step's fused reset places it"""
    return dict(ball_xy=np.ones((N, 2), np.int32), goal_xy=np.full((N, 2), -1, np.int32), step_count=np.zeros(N, np.int32),
                reward=np.zeros(N, np.float32), done=np.ones(N, np.uint8), goal_count=np.zeros(N, np.int32))


def greedy_share(lay, q):
    """(reached in the fewest steps, start cells that can reach done) over all mazes: from every cell that can reach 'X',
    the greedy first-max walk on the oracle's model of the maze, for steps_to_done steps"""
    good = total = 0
    for i, m in enumerate(SR.models_of("v0", lay, None)):
        dist = SR.steps_to_done(m)
        _, pol = first_max(q[i])
        for s in np.flatnonzero(np.isfinite(dist)):
            cur, ok = s, False
            for t in range(int(dist[s])):
                a = pol[cur]
                if m.sticky[cur, a]:
                    break
                if m.terminal[cur, a]:
                    ok = t == int(dist[s]) - 1
                    break
                cur = m.nxt[cur, a]
            good += ok
            total += 1
    return good, total


@functools.lru_cache(maxsize=None)
def learn_case():
    """24 bordered random 8x8 mazes, v0, from a zero table: LEARN_LAUNCHES x LEARN_T steps of learn().  Read only."""
    lay = bordered_random_layouts(LEARN_N, LEARN_G, LEARN_LAYOUT_SEED)
    st = learn_start(LEARN_N)
    q = np.zeros((LEARN_N, LEARN_G ** 2, 4), np.float32)
    eps32 = min(int(LEARN_EPSILON * 4294967296.0), 4294967295)
    learn("v0", LEARN_G, "per_env", lay, st, q, LEARN_T * LEARN_LAUNCHES, LEARN_ALPHA, LEARN_GAMMA, eps32, True, LEARN_SEED,
          LEARN_EPOCH, LEARN_ENV_BASE)
    good, total = greedy_share(lay, q)
    return dict(lay=lay, q=q, st=st, good=good, total=total)
