"""GPU: the one-launch foveal rollout (lmaze_foveal_rollout) against T step launches, the reference fixtures and the C
oracle.  Bit-exact: integers and float32 bit patterns (rewards incl. -0.0, visit map, planes), and the host epoch."""
import importlib

import numpy as np
import pytest
import torch

import oracle_lib as O
from conftest import golden_files
from helpers import f32_bits, load_golden, ref_reward_bits

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
DEV = torch.device("cuda", 0)
HI = {"v1": 6, "v2": 27, "v4": 27}          # action ids drawn from [-1, HI): out-of-range ids included


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.uint32)


def _same_env(a, b, what=""):
    ha, hb = a.host_state(), b.host_state()
    for k in ha:
        assert (np.ascontiguousarray(ha[k]).view(np.uint8) == np.ascontiguousarray(hb[k]).view(np.uint8)).all(), (what, k)
    assert (_bits(a.obs) == _bits(b.obs)).all(), (what, "obs")
    if a.obs_local is not None:
        assert (_bits(a.obs_local) == _bits(b.obs_local)).all(), (what, "obs_local")
    if a._has_visit:
        assert (_bits(a.visit) == _bits(b.visit)).all(), (what, "visit")
        assert torch.equal(a._visit_clock, b._visit_clock), (what, "visit_clock")
    assert a._epoch == b._epoch, (what, "epoch")


def _pair(variant, n, seed, near_limit=True):
    envs = [PKG.LmazeFovealVecEnv(n, variant=variant, device=DEV, seed=seed) for _ in range(2)]
    if near_limit:        # some episodes end inside the rollout
        rs = np.random.RandomState(seed)
        lim = int(envs[0].params.step_limit)
        sc = np.where(rs.rand(n) < 0.3, lim - rs.randint(0, 4, n), rs.randint(0, 5, n)).astype(np.int32)
        for e in envs:
            e.set_state(step_count=sc)
    return envs


def _step_rows(env, acts, auto_reset, goals=None):
    rows = []
    for t in range(acts.shape[0]):
        if goals is not None:
            env.hier_step(acts[t], goals[t])
        else:
            env.step(acts[t], auto_reset=auto_reset)
        r = [env.reward.clone(), env.done.clone()]
        if env.variant in ("v1", "v5", "v6"):
            r += [env.foveal_reward.clone(), env.foveal_done.clone()]
        rows.append(r)
    return rows


def _check_rows(out, rows, what):
    T = len(rows)
    assert out[3].shape == (T, out[1].shape[0]) and out[3].dtype == torch.float32 and out[4].dtype == torch.bool
    for t in range(T):
        assert (_bits(out[3][t]) == _bits(rows[t][0])).all(), (what, "reward_t", t)
        assert torch.equal(out[4][t].to(torch.uint8), rows[t][1].to(torch.uint8)), (what, "done_t", t)
        if len(rows[t]) > 2:
            assert (_bits(out[5][t]) == _bits(rows[t][2])).all(), (what, "foveal_reward_t", t)
            assert torch.equal(out[6][t].to(torch.uint8), rows[t][3].to(torch.uint8)), (what, "foveal_done_t", t)


# ---------------------------------------------------------------- 1. T launches vs one launch
@pytest.mark.parametrize("variant", ["v1", "v2", "v4"])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("n,T", [(1, 1), (63, 7), (64, 50), (1000, 37), (5000, 120), (65536, 16)])
def test_rollout_equals_step_launches(variant, auto_reset, n, T):
    one, ref = _pair(variant, n, seed=n + T)
    g = torch.Generator(device=DEV).manual_seed(n * 7 + T)
    for call in range(2):            # the second rollout continues from where the first one ended
        acts = torch.randint(-1, HI[variant], (T, n), dtype=torch.int32, device=DEV, generator=g)
        out = one.rollout(acts, auto_reset=auto_reset, trajectory=True)
        assert len(out) == (7 if variant == "v1" else 5)
        rows = _step_rows(ref, acts, auto_reset)
        _check_rows(out, rows, (variant, auto_reset, n, T, call))
        _same_env(one, ref, (variant, auto_reset, n, T, call))


# ---------------------------------------------------------------- 2. v5 / v6 two-level step
@pytest.mark.parametrize("variant", ["v5", "v6"])
@pytest.mark.parametrize("n,T", [(1, 3), (333, 40), (5000, 64)])
def test_two_level_rollout_equals_hier_steps(variant, n, T):
    one, ref = _pair(variant, n, seed=11 + n, near_limit=False)
    rs = np.random.RandomState(n)
    fd = torch.from_numpy(rs.rand(n) < 0.7).to(DEV)
    dn = torch.from_numpy(rs.rand(n) < 0.2).to(DEV)
    for e in (one, ref):
        e.foveal_done.copy_(fd.to(e.foveal_done.dtype))
        e.done.copy_(dn.to(e.done.dtype))
    g = torch.Generator(device=DEV).manual_seed(T)
    for call in range(2):
        acts = torch.randint(-1, 5, (T, n), dtype=torch.int32, device=DEV, generator=g)
        goals = torch.randint(-2, 27, (T, n), dtype=torch.int32, device=DEV, generator=g)
        out = one.rollout(acts, goals=goals, trajectory=True)
        assert len(out) == 7
        rows = _step_rows(ref, acts, False, goals=goals)
        _check_rows(out, rows, (variant, n, T, call))
        _same_env(one, ref, (variant, n, T, call))


def test_plain_v5_rollout_equals_steps():
    one, ref = _pair("v5", 700, seed=3, near_limit=False)
    acts = torch.randint(-1, 5, (30, 700), dtype=torch.int32, device=DEV)
    out = one.rollout(acts, trajectory=True)
    rows = _step_rows(ref, acts, False)
    _check_rows(out, rows, "v5 plain")
    _same_env(one, ref, "v5 plain")


# ---------------------------------------------------------------- 3. reference fixtures, one rollout per run of steps
def _replay_segments(g, variant):
    env = PKG.LmazeFovealVecEnv(1, variant=variant, layouts=list(g["layouts"]), device=DEV)
    n, T = 0, len(g["actions"])
    t = 0
    while t < T:
        if g["reset_before"][t]:
            env.set_state(ball_xy=g["ball_before"][t:t + 1], goal_xy=g["goal_before"][t:t + 1],
                          layout_id=g["layout_id"][t:t + 1])
            env.reset(place=False)
            n += 1
        end = t + 1
        while end < T and not g["reset_before"][end]:
            end += 1
        acts = torch.as_tensor(np.asarray(g["actions"][t:end], dtype=np.int32).reshape(-1, 1), device=DEV)
        out = env.rollout(acts, trajectory=True)
        for k in range(end - t):
            assert f32_bits(_np(out[3][k]))[0] == ref_reward_bits(g["reward"][t + k]), (t + k)
            assert int(out[4][k, 0]) == int(g["done"][t + k]), (t + k)
        h = env.host_state()
        assert h["step_count"][0] == g["step_count"][end - 1] and tuple(h["ball_xy"][0]) == tuple(g["ball"][end - 1])
        assert (_bits(_np(env.obs)[0]) == _bits(g["planes"][end - 1])).all(), end - 1
        if "visit" in g:
            assert (_bits(_np(env.visit)[0]) == _bits(g["visit"][end - 1])).all(), end - 1
        t = end


@pytest.mark.parametrize("name", golden_files("v2_") + golden_files("v4_"))
def test_rollout_matches_reference_fixture(name):
    _replay_segments(load_golden(name), name[:2])


@pytest.mark.parametrize("name", golden_files("v1_"))
def test_v1_rollout_matches_reference_fixture(name):
    """v1: segments split at reset and setFovealGoal; both reward streams' rows against the reference's."""
    g = load_golden(name)
    env = PKG.LmazeFovealVecEnv(1, variant="v1", layouts=[g["layout"]], device=DEV, reset=False)
    T, t = len(g["actions"]), 0
    while t < T:
        if g["reset_before"][t]:
            env.reset()
        if g["setgoal_before"][t]:
            env.set_foveal_goal(g["setgoal_ij"][t:t + 1])
        end = t + 1
        while end < T and not g["reset_before"][end] and not g["setgoal_before"][end]:
            end += 1
        acts = torch.as_tensor(np.asarray(g["actions"][t:end], dtype=np.int32).reshape(-1, 1), device=DEV)
        out = env.rollout(acts, trajectory=True)
        assert len(out) == 7
        for k in range(end - t):
            assert f32_bits(_np(out[3][k]))[0] == ref_reward_bits(g["reward"][t + k]), (t + k)
            assert int(out[4][k, 0]) == int(g["done"][t + k]), (t + k)
            assert f32_bits(_np(out[5][k]))[0] == ref_reward_bits(g["foveal_reward"][t + k]), (t + k)
            assert int(out[6][k, 0]) == int(g["foveal_done"][t + k]), (t + k)
        h = env.host_state()
        e = end - 1
        assert h["step_count"][0] == g["step_count"][e] and h["foveal_step_count"][0] == g["foveal_step_count"][e], e
        assert tuple(h["ball_xy"][0]) == tuple(g["ball"][e]), e
        assert (_bits(_np(env.obs)[0]) == _bits(g["planes"][e])).all(), e
        t = end


@pytest.mark.parametrize("name", golden_files("v5_") + golden_files("v6_"))
def test_v56_rollout_matches_reference_fixture(name):
    """v5/v6: segments split at reset and plannerStep; each run of plain steps is one rollout(trajectory=True) (the plain
    v5/v6 step's rollout is T launches, include/lmaze.h lmaze_foveal_rollout); all four row streams against the reference's."""
    g = load_golden(name)
    env = PKG.LmazeFovealVecEnv(1, variant="v5", layouts=list(g["layouts"]), device=DEV, reset=False)
    ev, arg = np.asarray(g["ev_type"]), np.asarray(g["ev_arg"])
    T, t = len(ev), 0
    while t < T:
        if ev[t] == 0:
            env.set_state(ball_xy=g["ball0"][t:t + 1], goal_xy=g["goal"][t:t + 1], layout_id=g["layout_id"][t:t + 1])
            env.reset(place=False)
            t += 1
            continue
        if ev[t] == 1:
            env.planner_step([int(arg[t])])
            t += 1
            continue
        end = t + 1
        while end < T and ev[end] == 2:
            end += 1
        acts = torch.as_tensor(arg[t:end].astype(np.int32).reshape(-1, 1), device=DEV)
        out = env.rollout(acts, trajectory=True)
        for k in range(end - t):
            assert f32_bits(_np(out[3][k]))[0] == ref_reward_bits(g["global_reward"][t + k]), (t + k)
            assert int(out[4][k, 0]) == int(g["global_done"][t + k]), (t + k)
            assert f32_bits(_np(out[5][k]))[0] == ref_reward_bits(g["local_reward"][t + k]), (t + k)
            assert int(out[6][k, 0]) == int(g["local_done"][t + k]), (t + k)
        e = end - 1
        h = env.host_state()
        assert tuple(h["ball_xy"][0]) == tuple(g["ball0"][e]) and h["step_count"][0] == g["step_count"][e], e
        assert (_bits(_np(env.visit)[0]) == _bits(g["visit"][e])).all(), e
        if not g["raised"][e]:
            assert (_bits(_np(env.obs)[0]) == _bits(g["fov_planes"][e])).all(), e
            assert (_bits(_np(env.obs_local)[0]) == _bits(g["loc_planes"][e])).all(), e
        t = end


# ---------------------------------------------------------------- 4. the oracle, long and fused
@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_fused_rollouts_match_oracle(variant):
    N = 1024
    env = PKG.LmazeFovealVecEnv(N, variant=variant, device=DEV, seed=21)
    layc = env.layouts.cpu().numpy()
    vid = O.VARIANT_V2 if variant == "v2" else O.VARIANT_V4
    p = O.foveal_params(vid, env.grid, env.n_layouts)
    st = O.FovealState(vid, N, env.grid)
    h = env.host_state()
    for k in ("ball_xy", "goal_xy", "layout_id", "step_count", "reward", "done"):
        getattr(st, k)[...] = h[k]
    if env._has_visit:
        st.visit[...] = _np(env.visit)
    rs = np.random.RandomState(5)
    for call in range(6):
        acts = rs.randint(0, 25, (250, N)).astype(np.int32)
        epoch = env._epoch
        out = env.rollout(torch.from_numpy(acts).to(DEV), auto_reset=True, trajectory=True)
        rew, done = _np(out[3]), _np(out[4])
        for t in range(250):
            O.foveal_reset(p, layc, st.done.copy(), 1, 21, epoch + t, st)
            O.foveal_step(p, layc, acts[t], st)
            assert (rew[t].view(np.uint32) == st.reward.view(np.uint32)).all(), (call, t)
            assert (done[t].astype(np.uint8) == st.done).all(), (call, t)
        h = env.host_state()
        for k in ("ball_xy", "goal_xy", "layout_id", "step_count", "done"):
            assert (h[k] == getattr(st, k)).all(), (call, k)
        assert (_bits(env.obs) == st.obs.view(np.uint32)).all(), call
        if env._has_visit:
            assert (_bits(env.visit) == st.visit.view(np.uint32)).all(), call


# ---------------------------------------------------------------- 5. v4 visit-map renormalisation inside a rollout
def test_v4_renormalisation_inside_rollout():
    N, T = 512, 700
    one, ref = _pair("v4", N, seed=8, near_limit=False)
    rs = np.random.RandomState(8)
    acts = rs.randint(0, 25, (T, N)).astype(np.int32)
    acts[rs.rand(T, N) < 0.2] = 99                # untouched this step: the envs' clocks stagger
    acts_t = torch.from_numpy(acts).to(DEV)
    for e in (one, ref):
        e.set_state(step_count=np.full(N, -10 ** 6, np.int32))   # no episode ends: the clocks run far
    clocks = []
    for c in range(7):
        one.rollout(acts_t[c * 100:(c + 1) * 100])
        clocks.append(_np(one._visit_clock) & 0xff)
    for t in range(T):
        ref.step(acts_t[t])
    _same_env(one, ref, "renorm")
    # wrapped: some env's clock went down between two calls, in more than one workgroup of 32
    wrapped = np.zeros(N, bool)
    for a, b in zip(clocks, clocks[1:]):
        wrapped |= b < a
    assert len(set(np.flatnonzero(wrapped) // 32)) > 1
    # and the oracle's dense plane
    env = ref
    layc = env.layouts.cpu().numpy()
    p = O.foveal_params(O.VARIANT_V4, env.grid, env.n_layouts)
    st = O.FovealState(O.VARIANT_V4, N, env.grid)
    st0 = PKG.LmazeFovealVecEnv(N, variant="v4", device=DEV, seed=8)
    h = st0.host_state()
    for k in ("ball_xy", "goal_xy", "layout_id", "reward", "done"):
        getattr(st, k)[...] = h[k]
    st.step_count[...] = -10 ** 6
    st.visit[...] = _np(st0.visit)
    for t in range(T):
        O.foveal_step(p, layc, acts[t], st)
    assert (_bits(one.visit) == st.visit.view(np.uint32)).all()
    assert (_bits(one.obs) == st.obs.view(np.uint32)).all()


# ---------------------------------------------------------------- 6. launch hints never change results
@pytest.mark.parametrize("n", [5000, 70000])
@pytest.mark.parametrize("variant", ["v1", "v2", "v4"])
def test_launch_hints_do_not_change_results(variant, n):
    T = 12
    acts = torch.randint(-1, HI[variant], (T, n), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    base = None
    for hint in (0, 0x20, 0x30, 0x35, 0x140, 0x220, 0x145):
        env = _pair(variant, n, seed=2)[0]
        env.params.launch_hint = hint
        out = env.rollout(acts, auto_reset=True, trajectory=True)
        got = (env, _bits(out[3]), _np(out[4]))
        if base is None:
            base = got
            continue
        assert (got[1] == base[1]).all() and (got[2] == base[2]).all(), hex(hint)
        _same_env(got[0], base[0], hex(hint))


# ---------------------------------------------------------------- 7. streaming size
@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_rollout_at_1m_envs(variant):
    n, T = 1 << 20, 8
    one, ref = (PKG.LmazeFovealVecEnv(n, variant=variant, device=DEV, seed=1) for _ in range(2))
    acts = torch.randint(0, 25, (T, n), dtype=torch.int32, device=DEV)
    out = one.rollout(acts, auto_reset=True, trajectory=True)
    rows = _step_rows(ref, acts, True)
    _check_rows(out, rows, variant)
    ha, hb = one.host_state(), ref.host_state()
    for k in ha:
        assert (ha[k] == hb[k]).all(), k
    for sl in (slice(0, 4096), slice(n - 4096, n)):
        assert (_bits(one.obs[sl]) == _bits(ref.obs[sl])).all()
    assert one._epoch == ref._epoch


# ---------------------------------------------------------------- 8. the Python surface
def test_rollout_python_surface():
    env = PKG.LmazeFovealVecEnv(256, variant="v2", device=DEV, seed=4)
    before = env.host_state()["ball_xy"].copy()
    epoch = env._epoch
    out = env.rollout(torch.empty((0, 256), dtype=torch.int32, device=DEV), auto_reset=True, trajectory=True)
    assert out[3].shape == (0, 256) and env._epoch == epoch and (env.host_state()["ball_xy"] == before).all()
    acts = torch.randint(0, 25, (4, 256), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        env.rollout(acts, auto_reset=True, device_epoch=True, trajectory=True)
    with pytest.raises(ValueError):
        env.rollout(acts[:, :100].contiguous())
    with pytest.raises(ValueError):
        env.rollout(acts.to(torch.int64))
    env.rollout(acts, auto_reset=True)
    assert env._epoch == epoch + 4
    env.rollout(acts)
    assert env._epoch == epoch + 4


@pytest.mark.parametrize("variant", ["v2", "v5"])
def test_capture_replays_equal_eager_rollouts(variant):
    n, T = 3000, 6
    cap, eager = (PKG.LmazeFovealVecEnv(n, variant=variant, device=DEV, seed=6) for _ in range(2))
    acts = torch.randint(0, 25 if variant == "v2" else 4, (T, n), dtype=torch.int32, device=DEV)
    goals = torch.randint(0, 25, (T, n), dtype=torch.int32, device=DEV) if variant == "v5" else None
    graph = cap.capture_rollout(acts, goals=goals, auto_reset=goals is None)
    for _ in range(3):
        graph.replay()
        eager.rollout(acts, goals=goals, auto_reset=goals is None)
        torch.cuda.synchronize()
        _same_env(cap, eager, variant)
