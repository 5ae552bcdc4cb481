"""GPU: the closed-loop one-launch rollouts (lmaze_rollout_policy / lmaze_rollout_policy_u8) against the C oracle, step by
step -- never against the library's own open-loop rollout.  Bit-exact: keys, actions, float32 bit patterns of reward, done,
every recorded slot, the final state, planes and goal counts.  No env-step is left out of a comparison."""
import importlib

import numpy as np
import pytest
import torch

from closed_loop_ref import DEV, explore_draw, make_env as _env, replay, to_numpy as _np
from closed_loop_ref import test_numpy_philox_is_the_oracles  # noqa: F401  (collected here: the replay draws with philox)
from helpers import bordered_random_layouts, f32_bits

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
ABI = importlib.import_module("gym-lmaze_amd._abi")


def _table(G, key, seed):
    """Mostly the four moves, some ids no step knows (no move): 4, 7, 200, 255."""
    rs = np.random.RandomState(seed)
    n = G ** 4 if key == "goal" else G * G
    return np.where(rs.rand(n) < 0.9, rs.randint(0, 4, n), rs.choice([4, 7, 200, 255], n)).astype(np.uint8)


def _replay(kind, variant, G, N, T, eps, auto_reset, k, key, hint=0, seed=21, step_limit=7, table=None, env=None, lay=None):
    """One rollout_policy() call against the oracle stepped T times from the env's host_state() (closed_loop_ref.replay);
    returns the oracle's sequences (pre-step ball after the reset, action, step count, reward, done: [T, N] each) and the
    call's outputs."""
    if env is None:
        env, lay = _env(kind, variant, G, N, seed=seed, step_limit=step_limit, hint=hint)
    tab = _table(G, key, G * 7 + N) if table is None else table
    epoch0, eps32 = env._epoch, ABI.epsilon_u32(eps)
    explored = [0]

    def action(key_ref, t, eg):
        act = tab[key_ref].astype(np.int32)
        if eps32:
            r = explore_draw(env.seed, epoch0 + t, eg)
            explore = r[0] < np.uint64(eps32)
            explored[0] += int(explore.sum())
            act = np.where(explore, (r[1] >> np.uint64(30)).astype(np.int32), act).astype(np.int32)
        return act

    r = replay(env, lay, kind, T, auto_reset, k, key,
               lambda obs_t: env.rollout_policy(T, policy=torch.from_numpy(tab).to(DEV), epsilon=eps, key=key, auto_reset=auto_reset,
                                                trajectory=True, obs_t=obs_t, obs_every=k), action)
    return dict(r, explored=explored[0], eps32=eps32)


KINDS = ["shared", "u8", "per_env"]
KEYS = {"v0": ["ball"], "v3": ["ball", "goal"]}


# ------------------------------------------------------------- 1. every kernel form, grid size and ragged batch
@pytest.mark.parametrize("G", [8, 11, 12, 18, 32])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_every_step_against_the_oracle(variant, kind, G):
    """N = 777 and 4 099: a partial last workgroup at every envs-per-workgroup size.  v3 with both key modes."""
    resets = explored = 0
    for N, T, eps, auto_reset, k in [(777, 13, 0.0, False, 0), (4099, 11, 0.25, True, 3), (777, 10, 1.0, True, 1),
                                     (4099, 7, 0.25, False, 1)]:
        for key in KEYS[variant]:
            r = _replay(kind, variant, G, N, T, eps, auto_reset, k, key)
            resets += r["resets"]
            explored += r["explored"]
            if eps == 1.0:
                assert r["explored"] == N * T              # r.x < 2^32 - 1 always, short of a 2^-32 event
            if eps == 0.25:
                assert 0.2 * N * T < r["explored"] < 0.3 * N * T
    assert resets > 777 and explored > 0


# ------------------------------------------------------------- 2. epsilon x fused reset x recording, crossed
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("G", [8, 11, 12, 18, 32])
@pytest.mark.parametrize("variant,kind,key", [("v0", "shared", "ball"), ("v3", "shared", "goal"), ("v0", "u8", "ball"),
                                              ("v3", "u8", "goal"), ("v0", "per_env", "ball"), ("v3", "per_env", "goal"),
                                              ("v3", "per_env", "ball")])
def test_epsilon_reset_recording_crossed(variant, kind, G, key, eps, auto_reset, k):
    _replay(kind, variant, G, 777, 14, eps, auto_reset, k, key)


# ------------------------------------------------------------- 3. every value of launch_hint bits 12-14; bits 8 and 15
@pytest.mark.parametrize("sel", range(1, 8))
@pytest.mark.parametrize("variant,kind,G,key", [("v0", "shared", 11, "ball"), ("v3", "shared", 12, "goal"), ("v3", "u8", 11, "ball"),
                                                ("v0", "u8", 18, "ball"), ("v0", "per_env", 11, "ball"),
                                                ("v3", "per_env", 18, "goal")])
def test_envs_per_workgroup_hints(variant, kind, G, key, sel):
    _replay(kind, variant, G, 4099, 9, 0.25, True, 2, key, hint=sel << 12)


@pytest.mark.parametrize("hint", [0x100, 1 << 15, 0x100 | (1 << 15) | (3 << 12)])
@pytest.mark.parametrize("variant,kind", [("v0", "shared"), ("v3", "per_env"), ("v0", "u8")])
def test_bit_8_is_not_read_and_bit_15_changes_nothing(variant, kind, hint):
    _replay(kind, variant, 11, 4099, 8, 0.25, True, 3, "ball", hint=hint)


def test_per_env_lds_clamp_at_64():
    """Per-env layouts at G = 64 with 64 envs per workgroup asked for: 32, the table inside the 160 KiB."""
    _replay("per_env", "v0", 64, 300, 6, 0.25, True, 2, "ball", hint=5 << 12)


# ------------------------------------------------------------- 4. a streaming size
@pytest.mark.parametrize("variant,kind,key", [("v0", "shared", "ball"), ("v3", "shared", "goal"), ("v0", "u8", "ball")])
def test_streaming_size(variant, kind, key):
    """1M x 11x11: 484 MB of int32 planes per step, beyond every cache."""
    r = _replay(kind, variant, 11, 1 << 20, 4, 0.25, True, 3, key, step_limit=3)
    assert r["resets"] > 1 << 18


def test_t_zero_and_single_step():
    for kind in KINDS:
        env, lay = _env(kind, "v0", 11, 777)
        before = {k: v.copy() for k, v in env.host_state().items()}
        tab = torch.zeros(121, dtype=torch.uint8, device=DEV)
        epoch = env._epoch
        assert len(env.rollout_policy(0, policy=tab)) == 3
        assert env._epoch == epoch
        for k, v in env.host_state().items():
            assert (v == before[k]).all()
        _replay(kind, "v0", 11, 777, 1, 0.25, True, 1, "ball", env=env, lay=lay)


def test_off_grid_state_keys_are_clamped_onto_the_grid():
    """State injected off the grid: the key takes the coordinates as the transition does, clamped, so no lookup leaves the
    table (include/lmaze.h).  The oracle replay above only ever sees on-grid state."""
    G, N = 11, 777
    for variant, key in (("v0", "ball"), ("v3", "goal")):
        env, _ = _env("shared", variant, G, N)
        rs = np.random.RandomState(4)
        ball = rs.randint(-5, G + 5, (N, 2)).astype(np.int32)
        goal = rs.randint(-5, G + 5, (N, 2)).astype(np.int32)
        env.set_state(ball_xy=ball, goal_xy=goal if variant == "v3" else None)
        tab = _table(G, key, 2)
        out = env.rollout_policy(1, policy=torch.from_numpy(tab).to(DEV), key=key, auto_reset=False, trajectory=True)
        b, g = np.clip(ball, 0, G - 1), np.clip(goal, 0, G - 1)
        want = b[:, 0] * G + b[:, 1] + ((g[:, 0] * G + g[:, 1]) * G * G if key == "goal" else 0)
        assert (_np(out[6])[0] == want).all() and (_np(out[5])[0] == tab[want]).all()


# ------------------------------------------------------------- 5. a known answer that owes nothing to the oracle
@pytest.mark.parametrize("kind", ["shared", "u8"])
@pytest.mark.parametrize("G,seed", [(11, 1), (18, 2), (12, None)])
def test_bfs_table_reaches_the_goal_in_bfs_distance(kind, G, seed):
    """v0, shared layout, epsilon 0, no reset: with a shortest-path table computed here by BFS, every env's first goal
    reward arrives at exactly its BFS distance from its start cell and no wall reward occurs before it.  v0 enters 'B' and
    'X' cells only (lmaze_env.py:172-195): an 'S' cell can be left but never entered."""
    lay = bordered_random_layouts(1, G, 900 + seed, p_wall=0.2)[0] if seed is not None else PKG.layouts.to_codes(PKG.layouts.V0_GRID_12)
    W, B, X = ord("W"), ord("B"), ord("X")
    INF = 1 << 20
    dist = np.full((G, G), INF, np.int64)
    table = np.full((G, G), 255, np.uint8)
    gx, gy = (int(v[0]) for v in np.nonzero(lay == X))
    dist[gx, gy] = 0
    frontier = [(gx, gy)]
    moves = [(-1, 0), (1, 0), (0, -1), (0, 1)]             # action ids 0-3 (lmaze_env.py:153-170): x is the row
    while frontier:
        nxt = []
        for vx, vy in frontier:                            # (vx, vy) can be entered; which cells step onto it?
            for a, (ox, oy) in enumerate(moves):
                ux, uy = vx - ox, vy - oy
                if 0 <= ux < G and 0 <= uy < G and lay[ux, uy] != W and dist[ux, uy] == INF:
                    dist[ux, uy] = dist[vx, vy] + 1
                    table[ux, uy] = a
                    if lay[ux, uy] == B:                   # only 'B' cells are walked through
                        nxt.append((ux, uy))
        frontier = nxt
    N = 4099
    env = PKG.LmazeVecEnv(N, variant="v0", layout=lay, seed=4, step_limit=10000, obs_dtype="u8" if kind == "u8" else "int32")
    start = env.host_state()["ball_xy"].copy()
    d = dist[start[:, 0], start[:, 1]]
    reach = d < INF
    assert reach.sum() > N // 2 and d[reach].min() >= 1
    T = int(d[reach].max()) + 3
    out = env.rollout_policy(T, policy=torch.from_numpy(table.reshape(-1)).to(DEV), epsilon=0.0, auto_reset=False, trajectory=True)
    reward_t = _np(out[3])
    goal, wall = reward_t == np.float32(env.rewards[2]), reward_t == np.float32(env.rewards[0])
    first = np.where(goal.any(axis=0), goal.argmax(axis=0) + 1, INF)          # 1-based step of the first goal reward
    assert (first[reach] == d[reach]).all()
    assert (first[~reach] == INF).all()
    steps = np.arange(1, T + 1)[:, None]
    assert not (wall & (steps <= first[None, :]))[:, reach].any()
    assert (_np(env.goal_count)[reach] >= 1).all()


# ------------------------------------------------------------- 6. the rows are the whole trajectory
@pytest.mark.parametrize("variant,kind,key", [("v0", "shared", "ball"), ("v3", "per_env", "goal"), ("v3", "u8", "ball")])
def test_rows_and_final_ball_reproduce_the_state_sequence(variant, kind, key):
    """(key_t, actions_t, reward_t, done_t) and the final ball_xy give back the oracle's state sequence of a sample of envs:
    the ball every step acted on (after its reset), the ball every step left behind, the step count, reward and done."""
    G, N, T = 11, 777, 40
    r = _replay(kind, variant, G, N, T, 0.25, True, 0, key)
    reward_t, done_t, actions_t, key_t = r["rows"]
    seq, final = r["seq"], r["final"]
    for i in np.random.RandomState(3).choice(N, 64, replace=False):
        cell = key_t[:, i] % (G * G)
        pre = np.stack([cell // G, cell % G], axis=1)                          # the ball step t acted on
        assert (pre == seq["ball"][:, i]).all()
        if key == "goal":                                                      # no step moves the goal: the last key holds it
            goal = int(key_t[-1, i]) // (G * G)
            assert (goal // G, goal % G) == tuple(final["goal_xy"][i])
        d = done_t[:, i].view(np.uint8)
        for t in range(T):
            post = pre[t + 1] if t + 1 < T else final["ball_xy"][i]            # what step t left behind ...
            if t + 1 < T and d[t]:
                continue                                                       # ... unless the next step's reset moved it
            ox = int(actions_t[t, i] == 1) - int(actions_t[t, i] == 0)
            oy = int(actions_t[t, i] == 3) - int(actions_t[t, i] == 2)
            moved = tuple(post) != tuple(pre[t])
            assert tuple(post) in (tuple(pre[t]), (pre[t][0] + ox, pre[t][1] + oy)), (i, t)
            if reward_t[t, i] == np.float32(-1.0):
                assert not moved, (i, t)                                       # a wall: the ball stays
        # step counts: zeroed by every reset, which the done row places
        sc = seq["sc"][:, i]
        for t in range(1, T):
            assert sc[t] == (1 if d[t - 1] else sc[t - 1] + 1), (i, t)
        assert (f32_bits(reward_t[:, i]) == f32_bits(seq["reward"][:, i])).all() and (d == seq["done"][:, i]).all()
        assert (actions_t[:, i] == seq["act"][:, i]).all()
        assert sc[-1] == final["step_count"][i]


# ------------------------------------------------------------- 7. recording changes nothing else
@pytest.mark.parametrize("variant,kind,key", [("v0", "shared", "ball"), ("v3", "shared", "goal"), ("v0", "u8", "ball"),
                                              ("v3", "per_env", "goal")])
def test_recording_on_and_off_give_the_same_rows(variant, kind, key):
    G, N, T = 11, 4099, 12
    tab = torch.from_numpy(_table(G, key, 9)).to(DEV)
    outs = []
    for k in (0, 1, 5):
        env, _ = _env(kind, variant, G, N)
        obs_t = torch.empty((T // k, N, G, G), dtype=env.obs.dtype, device=DEV) if k else None
        out = env.rollout_policy(T, policy=tab, epsilon=0.25, key=key, trajectory=True, obs_t=obs_t, obs_every=k)
        outs.append((env, out))
        if k:
            assert torch.equal(obs_t[-1] if T % k == 0 else env.obs, env.obs)
    e0, o0 = outs[0]
    for e, o in outs[1:]:
        for x, y in zip(o0[3:], o[3:]):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        assert torch.equal(e0._state, e._state) and torch.equal(e0.obs, e.obs) and e0._epoch == e._epoch


# ------------------------------------------------------------- 8. the Python surface
def test_q_ties_pick_the_first_maximum():
    G, N = 11, 777
    q = torch.zeros((G * G, 4), dtype=torch.float32, device=DEV)
    q[0] = torch.tensor([1.0, 3.0, 3.0, 2.0])              # two maxima: the first, 1
    q[1] = torch.tensor([5.0, 5.0, 5.0, 5.0])              # all equal: 0
    q[2] = torch.tensor([-1.0, -2.0, -0.5, -0.5])          # 2
    q[3] = torch.tensor([0.0, -0.0, -1.0, -1.0])           # 0.0 == -0.0: 0
    q[4] = torch.tensor([float("-inf"), float("-inf"), float("-inf"), 7.0])
    q[5] = torch.tensor([1.0, float("nan"), 0.0, 0.0])     # a NaN row: the id A = 4, no move
    q[6:] = torch.rand((G * G - 6, 4), device=DEV).round(decimals=1)            # plenty of ties
    tab = PKG.LmazeVecEnv.greedy_table(q)
    assert tab.dtype == torch.uint8 and tab[:6].tolist() == [1, 0, 2, 0, 3, 4]
    qn = _np(q)
    want = np.array([next((a for a in range(4) if qn[s, a] == np.nanmax(qn[s])), 4) for s in range(6, G * G)], np.uint8)
    assert (_np(tab)[6:] == want).all()
    # q= is policy=greedy_table(q)
    a, _ = _env("shared", "v0", G, N)
    b, _ = _env("shared", "v0", G, N)
    oa = a.rollout_policy(9, q=q, epsilon=0.25, trajectory=True)
    ob = b.rollout_policy(9, policy=tab, epsilon=0.25, trajectory=True)
    for x, y in zip(oa[3:], ob[3:]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(a._state, b._state)
    assert (oa[5][0] == tab[oa[6][0].long()].to(torch.int32)).sum() > N // 2     # most actions are the table's


def test_epoch_advances_by_t_and_results_follow_it():
    G, N = 11, 777
    tab = torch.from_numpy(_table(G, "ball", 1)).to(DEV)
    for auto_reset in (False, True):
        env, _ = _env("shared", "v0", G, N)
        e0 = env._epoch
        out = env.rollout_policy(5, policy=tab, epsilon=0.5, auto_reset=auto_reset)
        assert len(out) == 3 and out[0] is env.obs and env._epoch == e0 + 5
        env.rollout_policy(3, policy=tab, auto_reset=auto_reset)               # epsilon 0: the epochs are used up all the same
        assert env._epoch == e0 + 8
    # the same call at another epoch explores elsewhere
    a, _ = _env("shared", "v0", G, N)
    b, _ = _env("shared", "v0", G, N)
    b._epoch += 1
    xa = a.rollout_policy(6, policy=tab, epsilon=0.5, auto_reset=False, trajectory=True)[5]
    xb = b.rollout_policy(6, policy=tab, epsilon=0.5, auto_reset=False, trajectory=True)[5]
    assert not torch.equal(xa, xb)


def test_python_surface_refusals():
    G, N = 11, 64
    env, _ = _env("shared", "v0", G, N)
    v3, _ = _env("shared", "v3", G, N)
    tab = torch.zeros(G * G, dtype=torch.uint8, device=DEV)
    q = torch.zeros((G * G, 4), device=DEV)
    rows = torch.empty((6, N), dtype=torch.int32, device=DEV)
    ok = torch.empty((2, N, G, G), dtype=torch.int32, device=DEV)
    bad = [dict(), dict(policy=tab, q=q),                                                    # exactly one of the two
           dict(policy=tab.to(torch.int32)), dict(policy=tab[:-1]), dict(policy=tab.cpu()), dict(policy=tab.repeat(2)[::2]),
           dict(policy=torch.zeros(G ** 4, dtype=torch.uint8, device=DEV)),                  # the goal-keyed size, ball key
           dict(policy=tab, key="goal"), dict(policy=tab, key="cell"),                       # v0 keeps no goal
           dict(q=q[:, :0]), dict(q=q.to(torch.int32)), dict(q=q.cpu()), dict(q=q[:5]), dict(q=q.reshape(-1)),
           dict(policy=tab, epsilon=-0.1), dict(policy=tab, epsilon=1.5), dict(policy=tab, epsilon=float("nan")),
           dict(policy=tab, actions_t=rows[:5], trajectory=True), dict(policy=tab, key_t=rows.to(torch.int64)),
           dict(policy=tab, obs_t=ok, obs_every=0), dict(policy=tab, obs_t=None, obs_every=3), dict(policy=tab, obs_every=-1),
           dict(policy=tab, obs_t=ok[:1], obs_every=3), dict(policy=tab, obs_every=None)]
    epoch = env._epoch
    for kw in bad:
        with pytest.raises(ValueError):
            env.rollout_policy(6, **kw)
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError):
            env.rollout_policy(T, policy=tab)
    with pytest.raises(ValueError):
        v3.rollout_policy(6, policy=tab, key="goal")                                        # G**2 entries, G**4 wanted
    assert env._epoch == epoch                                                               # a refusal consumes nothing
    big = PKG.LmazeVecEnv(1 << 20, variant="v0", layout=PKG.layouts.open_room(11, (5, 5)), online_autotune=True)
    assert big.tuning_progress() is not None
    with pytest.raises(ValueError, match="device-resident epoch or while the online tuner runs"):
        big.rollout_policy(2, policy=tab)
    del big
    out = env.rollout_policy(6, policy=tab, trajectory=True, actions_t=rows, obs_t=ok, obs_every=3)
    assert len(out) == 7 and out[5] is rows and out[6].shape == (6, N) and out[6].dtype == torch.int32
    assert len(v3.rollout_policy(6, policy=torch.zeros(G ** 4, dtype=torch.uint8, device=DEV), key="goal")) == 3
