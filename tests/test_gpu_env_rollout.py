"""GPU: the closed-loop one-launch rollouts with a table per env (rollout_policy(key="env") / rollout_sample(key="env");
lmaze_env_rollout_policy / lmaze_env_rollout_sample) against the C oracle, step by step -- never against the library's
other rollouts.  Bit-exact: keys, actions, float32 bit patterns of reward, done, every recorded slot, the final state and
planes.  The tables are random per env, so a read from a neighbour's row shows at once."""
import importlib

import numpy as np
import pytest
import torch

import env_table_ref as R
import solve_ref as SR
from closed_loop_ref import DEV, fields, make_env as _env, to_numpy as _np
from closed_loop_ref import test_numpy_philox_is_the_oracles  # noqa: F401  (collected here: the replay draws with philox)

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
ABI = importlib.import_module("gym-lmaze_amd._abi")
FORMS = ["policy", "sample"]


def _dev(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _replay(kind, variant, G, N, T, eps, auto_reset, k, form, hint=0, env=None, lay=None, window=None, flat=False):
    """One rollout_policy(key="env") / rollout_sample(key="env") call against the oracle stepped T times from the env's
    host_state() (env_table_ref.replay).  flat: the table is passed as [N*G*G(, 4)] instead of [N, G*G(, 4)]."""
    if env is None:
        env, lay = _env(kind, variant, G, N, hint=hint)
    if form == "policy":
        tab = R.policy_tables(N, G, G * 7 + N)
        action = R.greedy_action(tab, ABI.epsilon_u32(eps), env.seed, env._epoch)
        t = _dev(tab.reshape(-1) if flat else tab)

        def rollout(obs_t):
            return env.rollout_policy(T, policy=t, epsilon=eps, key="env", auto_reset=auto_reset, trajectory=True, obs_t=obs_t,
                                      obs_every=k)
    else:
        tab = R.threshold_tables(N, G, G * 5 + N)
        action = R.sampled_action(tab, env.seed, env._epoch)
        t = _dev(tab.reshape(-1, 4) if flat else tab)

        def rollout(obs_t):
            return env.rollout_sample(T, thresholds=t, key="env", auto_reset=auto_reset, trajectory=True, obs_t=obs_t, obs_every=k)
    r = R.replay(env, lay, kind, T, auto_reset, k, rollout, action, window=window)
    return dict(r, explored=getattr(action, "explored", 0), env=env, table=tab)


# ------------------------------------------------------------- 1. every kernel form, grid size and ragged batch
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("G", [8, 11, 18, 32])
@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("kind", ["per_env", "shared"])
def test_every_step_against_the_oracle(kind, variant, G, form):
    """N = 777 and 4 099: a ragged last workgroup at every envs-per-workgroup size; 121 and 324 cells leave the staged
    copy a byte tail."""
    resets = 0
    for N, T, eps, auto_reset, k in [(777, 13, 0.0, False, 0), (4099, 11, 0.25, True, 3), (777, 10, 1.0, True, 1)]:
        r = _replay(kind, variant, G, N, T, eps, auto_reset, k, form, flat=N == 4099)
        resets += r["resets"]
        if form == "policy":
            acts = r["rows"][2]
            if eps == 0.0:
                assert r["explored"] == 0 and (acts > 3).any()          # the ids no step knows are passed through
            if eps == 1.0:
                assert r["explored"] == N * T                           # r.x < 2^32 - 1 always, short of a 2^-32 event
            if eps == 0.25:
                assert 0.2 * N * T < r["explored"] < 0.3 * N * T
    assert resets > 777


# ------------------------------------------------------------- 2. every value of launch_hint bits 12-14; bits 8 and 15
HINT_SHAPES = [("per_env", "v0", 11), ("per_env", "v3", 18), ("shared", "v0", 11)]


@pytest.mark.parametrize("sel", range(1, 8))
@pytest.mark.parametrize("kind,variant,G", HINT_SHAPES)
def test_envs_per_workgroup_hints(kind, variant, G, sel):
    for form in FORMS:
        r = _replay(kind, variant, G, 4099, 9, 0.25, True, 2, form, hint=sel << 12)
        line = ABI.describe_env_rollout(r["env"].params, 4099, 9, obs_every=2, form=form)
        assert fields(line)["envs_per_workgroup"] == min(4 << (sel - 1), 64 if kind == "per_env" else 256), line


@pytest.mark.parametrize("hint", [0x100, 1 << 15, 0x100 | (1 << 15) | (3 << 12)])
@pytest.mark.parametrize("kind,variant,G", HINT_SHAPES)
def test_bit_8_is_not_read_and_bit_15_changes_nothing(kind, variant, G, hint):
    for form in FORMS:
        _replay(kind, variant, G, 4099, 9, 0.25, True, 2, form, hint=hint)


def test_per_env_lds_clamp_at_64():
    """Per-env layouts at G = 64 with 64 envs per workgroup asked for: what fits 160 KiB with the staged tables counted --
    the run is at whatever the describe line names (16 envs: 2 x 64 KiB), the sampling form at the layouts' own 32."""
    for form, want in (("policy", 16), ("sample", 32)):
        r = _replay("per_env", "v0", 64, 300, 6, 0.25, True, 2, form, hint=5 << 12)
        f = fields(ABI.describe_env_rollout(r["env"].params, 300, 6, obs_every=2, form=form))
        assert f["envs_per_workgroup"] == want and f["lds"] <= 160 << 10, f


# ------------------------------------------------------------- 3. the 64-env workgroup with a ragged tail
def test_64_envs_per_workgroup_and_a_ragged_tail():
    """65 573 x 11x11 per-env (65 573 mod 64 = 37): 64 envs per workgroup by size, 7 744 staged table bytes each; the oracle
    replays the first and the last 2 048 envs."""
    N, G, T = 65573, 11, 6
    for window in ((0, 2048), (N - 2048, 2048)):
        r = _replay("per_env", "v0", G, N, T, 0.25, True, 3, "policy", window=window)
        assert fields(ABI.describe_env_rollout(r["env"].params, N, T, obs_every=3))["envs_per_workgroup"] == 64
        assert (r["rows"][3][0] // (G * G) == np.arange(window[0], window[0] + 2048)).all()


# ------------------------------------------------------------- 4. T = 0, T = 1, state off the grid
@pytest.mark.parametrize("kind", ["per_env", "shared"])
def test_t_zero_and_single_step(kind):
    N, G = 777, 11
    for form in FORMS:
        env, lay = _env(kind, "v0", G, N)
        before = {k: v.copy() for k, v in env.host_state().items()}
        epoch = env._epoch
        if form == "policy":
            out = env.rollout_policy(0, policy=torch.zeros((N, G * G), dtype=torch.uint8, device=DEV), key="env")
        else:
            out = env.rollout_sample(0, thresholds=torch.zeros((N, G * G, 4), dtype=torch.int32, device=DEV), key="env")
        assert len(out) == 3 and env._epoch == epoch
        for k, v in env.host_state().items():
            assert (v == before[k]).all()
        _replay(kind, "v0", G, N, 1, 0.25, True, 1, form, env=env, lay=lay)


@pytest.mark.parametrize("kind", ["per_env", "shared"])
def test_off_grid_state_keys_are_clamped_onto_the_grid(kind):
    """State injected off the grid: the key takes the coordinates as the transition does, clamped, so no lookup leaves the
    env's own rows (include/lmaze.h).  The oracle replay above only ever sees on-grid state."""
    G, N = 11, 777
    for variant in ("v0", "v3"):
        env, _ = _env(kind, variant, G, N)
        rs = np.random.RandomState(4)
        ball = rs.randint(-5, G + 5, (N, 2)).astype(np.int32)
        goal = rs.randint(-5, G + 5, (N, 2)).astype(np.int32)
        env.set_state(ball_xy=ball, goal_xy=goal if variant == "v3" else None)
        want = R.env_keys(ball, G)
        assert (_np(env.state_keys("env")) == want).all()
        tab = R.policy_tables(N, G, 2)
        out = env.rollout_policy(1, policy=_dev(tab), key="env", auto_reset=False, trajectory=True)
        assert (_np(out[6])[0] == want).all() and (_np(out[5])[0] == tab.reshape(-1)[want]).all()
        env.set_state(ball_xy=ball, done=np.zeros(N, np.uint8))
        rows = R.threshold_tables(N, G, 3)
        e0 = env._epoch
        out = env.rollout_sample(1, thresholds=_dev(rows), key="env", auto_reset=False, trajectory=True)
        eg = np.arange(N, dtype=np.uint64) + np.uint64(env.env_base)
        assert (_np(out[6])[0] == want).all() and (_np(out[5])[0] == R.sampled_action(rows, env.seed, e0)(want, 0, eg)).all()


# ------------------------------------------------------------- 5. plan, then act
@pytest.mark.parametrize("G", [8, 11])
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_plan_then_act(variant, G):
    """777 random mazes, a table solved for each (v3: for its current goal_xy), followed with no exploration and no reset:
    every env's first done falls at exactly the fewest steps of its start cell in the oracle's model of ITS maze, and an
    unreachable start never gets there.  The control -- every env follows its neighbour's table -- must miss that for more
    than half of the reachable envs (in the oracle's model: 92-98 % of them, tests/test_env_rollout_cpu.py)."""
    case = R.plan_case(variant, G)
    N, T = R.PLAN_N, case["T"]
    env = PKG.LmazeVecEnv(N, per_env_layouts=case["lay"], variant=variant, seed=3, step_limit=1 << 20)
    # the reward too: v0 keeps it through a refused move onto 'S', and a kept reward_goal reads as done
    state = dict(ball_xy=case["start"], step_count=np.zeros(N, np.int32), done=np.zeros(N, np.uint8), reward=np.zeros(N, np.float32))
    if variant == "v3":
        state["goal_xy"] = case["goals"]
    env.set_state(**state)
    s = env.solve(gamma=R.PLAN_GAMMA, sweeps=R.PLAN_SWEEPS)
    assert tuple(s.q.shape) == (N, G * G, 4) and int(s.sweeps_run.max()) < R.PLAN_SWEEPS
    reach = np.isfinite(case["dist"])

    def first_done(**table):
        env.set_state(**state)
        out = env.rollout_policy(T, epsilon=0.0, key="env", auto_reset=False, trajectory=True, **table)
        done_t = _np(out[4]).astype(bool)
        return np.where(done_t.any(0), done_t.argmax(0), -1), _np(out[3])
    first, reward_t = first_done(q=s.q)
    assert not R.missed(case, first).any(), np.flatnonzero(reach)[R.missed(case, first)][:8]
    assert (first[~reach] < 0).all() and reach.sum() > 600 and (~reach).sum() > 20
    assert (reward_t[first[reach], np.flatnonzero(reach)].view(np.uint32) == np.float32(env.rewards[2]).view(np.uint32)).all()
    assert (first == R.follow(case, _np(s.policy), T)).all()
    rolled = torch.roll(s.policy, 1, 0).contiguous()
    first, _ = first_done(policy=rolled)
    assert (first == R.follow(case, _np(rolled), T)).all()
    assert R.missed(case, first).mean() > 0.5, R.missed(case, first).mean()


# ------------------------------------------------------------- 6. the rows feed the learners unchanged
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_rows_feed_gae_and_table_stats(variant):
    G, N, T = 11, 777, 12
    env, lay = _env("per_env", variant, G, N)
    s = env.solve(sweeps=64)
    out = env.rollout_policy(T, q=s.q, epsilon=0.25, key="env", auto_reset=True, trajectory=True)
    reward_t, done_t, act_t, key_t = out[3:]
    values = s.v.reshape(-1).contiguous()
    tail_keys = env.state_keys("env")
    assert tail_keys.dtype == torch.int32 and (_np(tail_keys) == R.env_keys(_np(env.ball_xy), G)).all()
    adv_a, tgt_a = PKG.gae(reward_t, done_t, 0.99, 0.95, values=values, key_t=key_t, key_tail=tail_keys)
    adv_b, tgt_b = PKG.gae(reward_t, done_t, 0.99, 0.95, value_t=values[key_t.long()].contiguous(), tail=values[tail_keys.long()].contiguous())
    assert torch.equal(adv_a.view(torch.int32), adv_b.view(torch.int32)) and torch.equal(tgt_a.view(torch.int32), tgt_b.view(torch.int32))
    count, total = PKG.table_stats(key_t, act_t, reward_t, keys=N * G * G)
    ok = act_t < 4
    want = torch.bincount((key_t.long() * 4 + act_t.long())[ok], minlength=N * G * G * 4).reshape(N * G * G, 4)
    assert torch.equal(count, want) and int(count.sum()) == int(ok.sum()) > 0
    # every env's samples fall into its own rows
    assert (_np(key_t) // (G * G) == np.arange(N)).all()


# ------------------------------------------------------------- 7. tie to the ball-keyed path; recording on and off
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_one_table_repeated_is_the_ball_keyed_rollout(variant):
    G, N, T = 11, 777, 12
    a, _ = _env("shared", variant, G, N)
    b, _ = _env("shared", variant, G, N)
    tab = R.policy_tables(1, G, 9)[0]
    rows = R.threshold_tables(1, G, 9)[0]
    for ea, eb in ((a.rollout_policy(T, policy=_dev(np.tile(tab, (N, 1))), epsilon=0.25, key="env", trajectory=True),
                    b.rollout_policy(T, policy=_dev(tab), epsilon=0.25, key="ball", trajectory=True)),
                   (a.rollout_sample(T, thresholds=_dev(np.tile(rows, (N, 1, 1))), key="env", trajectory=True),
                    b.rollout_sample(T, thresholds=_dev(rows), key="ball", trajectory=True))):
        for i in (0, 1, 2, 3, 4, 5):
            assert torch.equal(ea[i].view(torch.uint8), eb[i].view(torch.uint8)), i
        assert torch.equal(ea[6], eb[6] + (torch.arange(N, device=DEV, dtype=torch.int32) * G * G)[None, :])
        for name, v in a.host_state().items():
            assert (v == b.host_state()[name]).all(), name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,variant", [("per_env", "v0"), ("per_env", "v3"), ("shared", "v3")])
def test_recording_on_and_off_give_the_same_rows(kind, variant, form):
    G, N, T = 11, 777, 11
    tab = _dev(R.policy_tables(N, G, 1) if form == "policy" else R.threshold_tables(N, G, 1))
    got = []
    for k in (0, 1, 5):
        env, _ = _env(kind, variant, G, N)
        obs_t = torch.empty((T // k, N, G, G), dtype=torch.int32, device=DEV) if k else None
        if form == "policy":
            out = env.rollout_policy(T, policy=tab, epsilon=0.25, key="env", trajectory=True, obs_t=obs_t, obs_every=k)
        else:
            out = env.rollout_sample(T, thresholds=tab, key="env", trajectory=True, obs_t=obs_t, obs_every=k)
        got.append(([_np(x).copy() for x in out], {n: v.copy() for n, v in env.host_state().items()}))
    for out, state in got[1:]:
        for x, y in zip(out, got[0][0]):
            assert (x.view(np.uint8) == y.view(np.uint8)).all()
        for n, v in state.items():
            assert (v == got[0][1][n]).all(), n


# ------------------------------------------------------------- 8. the Python surface's refusals
def test_python_surface_refusals():
    G, N = 11, 64
    env, _ = _env("per_env", "v0", G, N)
    S = G * G
    pol = torch.zeros((N, S), dtype=torch.uint8, device=DEV)
    thr = torch.zeros((N, S, 4), dtype=torch.int32, device=DEV)
    epoch = env._epoch
    bad_policies = [torch.zeros((N, S + 1), dtype=torch.uint8, device=DEV), torch.zeros(S, dtype=torch.uint8, device=DEV),
                    torch.zeros((N + 1, S), dtype=torch.uint8, device=DEV), torch.zeros((S, N), dtype=torch.uint8, device=DEV),
                    torch.zeros((N, S), dtype=torch.int32, device=DEV), torch.zeros((N, S), dtype=torch.uint8),
                    torch.zeros((N, 2 * S), dtype=torch.uint8, device=DEV)[:, ::2], torch.zeros(N * S + 1, dtype=torch.uint8, device=DEV)[1:]]
    for bad in bad_policies:
        with pytest.raises(ValueError):
            env.rollout_policy(4, policy=bad, key="env")
    for bad in (torch.zeros((N, S + 1, 4), device=DEV), torch.zeros((N, S, 4)), torch.zeros((S, 4), device=DEV),
                torch.zeros((N, S, 4), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError):
            env.rollout_policy(4, q=bad, key="env")
    with pytest.raises(ValueError):
        env.rollout_policy(4, policy=pol, q=torch.zeros((N, S, 4), device=DEV), key="env")
    for bad in (torch.zeros((N, S, 3), dtype=torch.int32, device=DEV), torch.zeros((S, 4), dtype=torch.int32, device=DEV),
                torch.zeros((N, S, 4), dtype=torch.int32), torch.zeros((N, S, 4), dtype=torch.float32, device=DEV),
                torch.zeros((N, S, 8), dtype=torch.int32, device=DEV)[:, :, ::2],
                torch.zeros(N * S * 4 + 1, dtype=torch.int32, device=DEV)[1:].view(N * S, 4)):
        with pytest.raises(ValueError):
            env.rollout_sample(4, thresholds=bad, key="env")
    for bad in (torch.zeros((N, S, 3), device=DEV), torch.zeros((N, S, 4)), torch.zeros((N, S, 4), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError):
            env.rollout_sample(4, probs=bad, key="env")
        with pytest.raises(ValueError):
            env.rollout_sample(4, logits=bad, key="env")
    with pytest.raises(ValueError):
        env.rollout_sample(4, probs=-torch.ones((N, S, 4), device=DEV), key="env")
    for key in ("cell", "envs", 2):
        with pytest.raises(ValueError):
            env.rollout_policy(4, policy=pol, key=key)
        with pytest.raises(ValueError):
            env.state_keys(key)
    with pytest.raises(ValueError):
        env.rollout_policy(4, policy=pol, key="env", key_t=torch.zeros((3, N), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        env.rollout_policy(4, policy=pol, key="env", epsilon=1.5)
    with pytest.raises(ValueError, match="key must be 'ball' or 'goal'"):
        env.solve(key="env")
    u8, _ = _env("u8", "v0", G, N)
    for call in (lambda: u8.rollout_policy(4, policy=pol, key="env"), lambda: u8.rollout_sample(4, thresholds=thr, key="env")):
        with pytest.raises(ValueError, match="int32 planes"):
            call()
    assert env._epoch == epoch                              # a refusal consumes no epoch
    # and what is accepted: both shapes of every table, float probs and logits
    env.rollout_policy(2, policy=pol.reshape(-1), key="env")
    env.rollout_policy(2, q=torch.rand((N * S, 4), device=DEV), key="env")
    env.rollout_sample(2, thresholds=thr.reshape(-1, 4), key="env")
    env.rollout_sample(2, probs=torch.rand((N, S, 4), device=DEV) + 0.1, key="env")
    env.rollout_sample(2, logits=torch.randn((N * S, 4), device=DEV), key="env", temperature=0.5)
    assert env._epoch == epoch + 10
