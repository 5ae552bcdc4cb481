"""GPU: rollouts that record observations (lmaze_rollout_obs, lmaze_foveal_rollout_obs) against T step launches and the
reference fixtures.  Bit-exact: integer planes, float32 bit patterns, state, rows and the host epoch."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden_files
from helpers import compact_to_ref_bits, load_golden

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
DEV = torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.uint32)


def _same_state(a, b, what=""):
    ha, hb = a.host_state(), b.host_state()
    for k in ha:
        assert (np.ascontiguousarray(ha[k]).view(np.uint8) == np.ascontiguousarray(hb[k]).view(np.uint8)).all(), (what, k)
    assert a._epoch == b._epoch, (what, "epoch")


def _grid_env(kind, variant, G, N, seed=2):
    if kind == "per_env":
        lays = PKG.layouts.random_walled(N, G, DEV, seed=7 + G)
        return PKG.LmazeVecEnv(N, variant=variant, per_env_layouts=lays, seed=seed, env_base=5)
    lay = PKG.layouts.open_room(G, (G // 2, G // 2))
    return PKG.LmazeVecEnv(N, variant=variant, layout=lay, seed=seed, env_base=5)


# ---------------------------------------------------------------- 1. grid: recording rollout == T step launches
GRID_SHAPES = [("shared", 8, 65536, 7),        # rollout_shared_wave8_kernel
               ("shared", 11, 3000, 7),        # rollout_shared_kernel, small
               ("shared", 11, 5001, 8),        # ragged N
               ("per_env", 11, 777, 7),        # rollout_perenv_kernel
               ("per_env", 32, 1001, 5),
               ("shared", 11, 4096, 1)]        # T == 1: the step-launch fallback


@pytest.mark.parametrize("kind,G,N,T", GRID_SHAPES)
@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_grid_recording_equals_step_launches(kind, G, N, T, variant, auto_reset, k):
    rec, ref, plain = (_grid_env(kind, variant, G, N) for _ in range(3))
    for e in (rec, ref, plain):                 # some episodes end inside the rollout
        e.step_count.fill_(e.params.step_limit - 3)
    gen = torch.Generator(device="cuda").manual_seed(G * 1000 + N + T)
    acts = torch.randint(-1, 5, (T, N), dtype=torch.int32, device="cuda", generator=gen)
    obs_t = torch.full((T // k, N, G, G), -7, dtype=torch.int32, device=DEV)
    out = rec.rollout(acts, auto_reset=auto_reset, trajectory=True, obs_t=obs_t, obs_every=k)
    assert len(out) == 5
    pout = plain.rollout(acts, auto_reset=auto_reset, trajectory=True)
    for t in range(T):
        o, _, _, _ = ref.step(acts[t], auto_reset=auto_reset)
        if (t + 1) % k == 0:
            assert torch.equal(obs_t[(t + 1) // k - 1], o), t
    _same_state(rec, ref, "steps")
    _same_state(rec, plain, "plain")
    assert torch.equal(rec.obs, plain.obs) and torch.equal(rec.obs, ref.obs)
    assert torch.equal(out[3].view(torch.int32), pout[3].view(torch.int32)) and torch.equal(out[4], pout[4])


@pytest.mark.parametrize("kind,G,N,T", GRID_SHAPES)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_grid_final_planes_only(kind, G, N, T, variant):
    rec, plain = _grid_env(kind, variant, G, N), _grid_env(kind, variant, G, N)
    acts = torch.randint(-1, 5, (T, N), dtype=torch.int32, device="cuda")
    rec.obs.fill_(-1)
    rec.rollout(acts, auto_reset=True, obs_every=0)
    plain.rollout(acts, auto_reset=True)
    _same_state(rec, plain)
    assert torch.equal(rec.obs, plain.obs)


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("auto_reset", [False, True])
def test_grid_recording_streaming_size(variant, auto_reset):
    N, G, T, k = 1 << 20, 11, 4, 3
    rec, ref = _grid_env("shared", variant, G, N), _grid_env("shared", variant, G, N)
    for e in (rec, ref):
        e.step_count.fill_(e.params.step_limit - 2)
    acts = torch.randint(-1, 5, (T, N), dtype=torch.int32, device="cuda")
    obs_t = torch.empty((T // k, N, G, G), dtype=torch.int32, device=DEV)
    rec.rollout(acts, auto_reset=auto_reset, obs_t=obs_t, obs_every=k)
    for t in range(T):
        o, _, _, _ = ref.step(acts[t], auto_reset=auto_reset)
        if (t + 1) % k == 0:
            assert torch.equal(obs_t[(t + 1) // k - 1], o), t
    _same_state(rec, ref)
    assert torch.equal(rec.obs, ref.obs)
    del obs_t, rec, ref
    fin, ref = _grid_env("shared", variant, G, N), _grid_env("shared", variant, G, N)
    for e in (fin, ref):
        e.step_count.fill_(e.params.step_limit - 2)
    fin.rollout(acts, auto_reset=auto_reset, obs_every=0)
    ref.rollout(acts, auto_reset=auto_reset)
    _same_state(fin, ref)
    assert torch.equal(fin.obs, ref.obs)


def test_grid_recording_step_launch_hint():
    """launch_hint bit 8 forces T step launches: each gets its slot, nothing, or obs."""
    N, G, T, k = 3000, 11, 7, 2
    rec, ref = _grid_env("shared", "v0", G, N), _grid_env("shared", "v0", G, N)
    rec.params.launch_hint = 0x100
    acts = torch.randint(-1, 5, (T, N), dtype=torch.int32, device="cuda")
    obs_t = torch.empty((T // k, N, G, G), dtype=torch.int32, device=DEV)
    rec.rollout(acts, obs_t=obs_t, obs_every=k)
    for t in range(T):
        o, _, _, _ = ref.step(acts[t], auto_reset=True)
        if (t + 1) % k == 0:
            assert torch.equal(obs_t[(t + 1) // k - 1], o), t
    _same_state(rec, ref)
    assert torch.equal(rec.obs, ref.obs)


# ---------------------------------------------------------------- 2. the u8 env (T step launches)
@pytest.mark.parametrize("G", [11, 12])
@pytest.mark.parametrize("k", [1, 3, 0])
def test_u8_recording_is_the_int32_trajectory_narrowed(G, k):
    N, T = 2000, 7
    lay = PKG.layouts.open_room(G, (G // 2, G // 2))
    narrow = PKG.LmazeVecEnv(N, variant="v3", layout=lay, seed=3, obs_dtype="u8")
    wide = PKG.LmazeVecEnv(N, variant="v3", layout=lay, seed=3)
    acts = torch.randint(-1, 5, (T, N), dtype=torch.int32, device="cuda")
    S = T // k if k else 0
    o8 = torch.empty((S, N, G, G), dtype=torch.uint8, device=DEV) if k else None
    o32 = torch.empty((S, N, G, G), dtype=torch.int32, device=DEV) if k else None
    narrow.rollout(acts, obs_t=o8, obs_every=k)
    wide.rollout(acts, obs_t=o32, obs_every=k)
    if k:
        assert torch.equal(o8, o32.to(torch.uint8))
    assert torch.equal(narrow.obs, wide.obs.to(torch.uint8))
    _same_state(narrow, wide)


# ---------------------------------------------------------------- 3. grid: every step against the reference fixtures
@pytest.mark.parametrize("name", golden_files("v0_") + golden_files("v3_"))
def test_grid_recording_matches_reference_fixture(name):
    """Each run of steps between the fixture's resets is one rollout(obs_every=1): every step's slot against planes[t]."""
    g = load_golden(name)
    v3 = name.startswith("v3")
    env = PKG.LmazeVecEnv(1, variant="v3" if v3 else "v0", layout=g["layout"], expansion=int(g["E"]))
    acts_all = np.asarray(g["actions"], dtype=np.int32)
    T, t = len(acts_all), 0
    while t < T:
        if g["reset_before"][t]:
            env.set_state(ball_xy=g["ball_before"][t:t + 1], step_count=np.zeros(1, np.int32),
                          reward=np.array([-0.0], np.float32), done=np.zeros(1, np.uint8),
                          goal_xy=g["goal_before"][t:t + 1] if v3 else None)
        end = t + 1
        while end < T and not g["reset_before"][end]:
            end += 1
        acts = torch.as_tensor(acts_all[t:end].reshape(-1, 1), device=DEV)
        obs_t = torch.empty((end - t, 1, env.grid, env.grid), dtype=torch.int32, device=DEV)
        env.rollout(acts, auto_reset=False, obs_t=obs_t, obs_every=1)
        got = compact_to_ref_bits(_np(obs_t)[:, 0], env.channel_mask)
        for j in range(end - t):
            assert (got[j] == np.asarray(g["planes"][t + j])).all(), (name, t + j)
        t = end


# ---------------------------------------------------------------- 4. foveal: recording rollout == T step launches
HI = {"v1": 6, "v2": 27, "v4": 27}          # action ids drawn from [-1, HI): out-of-range ids, i.e. skipped envs, included


def _foveal_pair(variant, n, seed):
    envs = [PKG.LmazeFovealVecEnv(n, variant=variant, device=DEV, seed=seed) for _ in range(3)]
    rs = np.random.RandomState(seed)
    lim = int(envs[0].params.step_limit)
    sc = np.where(rs.rand(n) < 0.3, lim - rs.randint(0, 4, n), rs.randint(0, 5, n)).astype(np.int32)
    for e in envs:
        e.set_state(step_count=sc)
    return envs


def _same_foveal(a, b, what=""):
    _same_state(a, b, what)
    assert (_bits(a.obs) == _bits(b.obs)).all(), (what, "obs")
    if a.obs_local is not None:
        assert (_bits(a.obs_local) == _bits(b.obs_local)).all(), (what, "obs_local")
    if a._has_visit:
        assert (_bits(a.visit) == _bits(b.visit)).all(), (what, "visit")


@pytest.mark.parametrize("n,T", [(1000, 9), (1 << 20, 4)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("variant,auto_reset", [("v1", False), ("v1", True), ("v2", False), ("v2", True), ("v4", False),
                                                ("v4", True)])
def test_foveal_recording_equals_step_launches(variant, auto_reset, k, n, T):
    rec, ref, plain = _foveal_pair(variant, n, 5)
    gen = torch.Generator(device="cuda").manual_seed(n + T + k)
    acts = torch.randint(-1, HI[variant], (T, n), dtype=torch.int32, device="cuda", generator=gen)
    obs_t = torch.full((T // k, n) + tuple(rec.obs.shape[1:]), -3.0, dtype=torch.float32, device=DEV)
    out = rec.rollout(acts, auto_reset=auto_reset, trajectory=True, obs_t=obs_t, obs_every=k)
    pout = plain.rollout(acts, auto_reset=auto_reset, trajectory=True)
    assert len(out) == len(pout)
    for t in range(T):
        ref.step(acts[t], auto_reset=auto_reset)
        if (t + 1) % k == 0:
            assert (_bits(obs_t[(t + 1) // k - 1]) == _bits(ref.obs)).all(), t
    _same_foveal(rec, ref, "steps")
    _same_foveal(rec, plain, "plain")
    for x, y in zip(out[3:], pout[3:]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.parametrize("n,T", [(1000, 9), (1 << 20, 4)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("variant", ["v5", "v6"])
def test_two_level_recording_equals_hier_steps(variant, k, n, T):
    rec, ref, plain = (PKG.LmazeFovealVecEnv(n, variant=variant, device=DEV, seed=6) for _ in range(3))
    for e in (rec, ref, plain):
        e.foveal_done.fill_(True)
    gen = torch.Generator(device="cuda").manual_seed(n + T + k)
    acts = torch.randint(-1, 5, (T, n), dtype=torch.int32, device="cuda", generator=gen)
    goals = torch.randint(-1, 26, (T, n), dtype=torch.int32, device="cuda", generator=gen)
    obs_t = torch.empty((T // k, n) + tuple(rec.obs.shape[1:]), dtype=torch.float32, device=DEV)
    loc_t = torch.empty((T // k, n) + tuple(rec.obs_local.shape[1:]), dtype=torch.float32, device=DEV)
    rec.rollout(acts, goals=goals, obs_t=obs_t, obs_local_t=loc_t, obs_every=k)
    plain.rollout(acts, goals=goals)
    for t in range(T):
        ref.hier_step(acts[t], goals[t])
        if (t + 1) % k == 0:
            assert (_bits(obs_t[(t + 1) // k - 1]) == _bits(ref.obs)).all(), t
            assert (_bits(loc_t[(t + 1) // k - 1]) == _bits(ref.obs_local)).all(), t
    _same_foveal(rec, ref, "steps")
    _same_foveal(rec, plain, "plain")


def test_plain_v5_host_path_records():
    n, T, k = 700, 7, 2
    rec, ref = (PKG.LmazeFovealVecEnv(n, variant="v5", device=DEV, seed=8) for _ in range(2))
    acts = torch.randint(-1, 5, (T, n), dtype=torch.int32, device="cuda")
    obs_t = torch.empty((T // k, n) + tuple(rec.obs.shape[1:]), dtype=torch.float32, device=DEV)
    loc_t = torch.empty((T // k, n) + tuple(rec.obs_local.shape[1:]), dtype=torch.float32, device=DEV)
    out = rec.rollout(acts, obs_t=obs_t, obs_local_t=loc_t, obs_every=k)
    assert len(out) == 3
    for t in range(T):
        ref.step(acts[t])
        if (t + 1) % k == 0:
            assert (_bits(obs_t[(t + 1) // k - 1]) == _bits(ref.obs)).all(), t
            assert (_bits(loc_t[(t + 1) // k - 1]) == _bits(ref.obs_local)).all(), t
    _same_foveal(rec, ref)


# ---------------------------------------------------------------- 5. foveal: every step against the reference fixtures
@pytest.mark.parametrize("name", golden_files("v2_") + golden_files("v4_"))
def test_foveal_recording_matches_reference_fixture(name):
    g = load_golden(name)
    env = PKG.LmazeFovealVecEnv(1, variant=name[:2], layouts=list(g["layouts"]), device=DEV)
    T, t = len(g["actions"]), 0
    while t < T:
        if g["reset_before"][t]:
            env.set_state(ball_xy=g["ball_before"][t:t + 1], goal_xy=g["goal_before"][t:t + 1],
                          layout_id=g["layout_id"][t:t + 1])
            env.reset(place=False)
        end = t + 1
        while end < T and not g["reset_before"][end]:
            end += 1
        acts = torch.as_tensor(np.asarray(g["actions"][t:end], dtype=np.int32).reshape(-1, 1), device=DEV)
        obs_t = torch.empty((end - t, 1) + tuple(env.obs.shape[1:]), dtype=torch.float32, device=DEV)
        env.rollout(acts, obs_t=obs_t, obs_every=1)
        for j in range(end - t):
            assert (_bits(_np(obs_t)[j, 0]) == _bits(g["planes"][t + j])).all(), (name, t + j)
        t = end


@pytest.mark.parametrize("name", golden_files("v5_") + golden_files("v6_"))
def test_v56_recording_matches_reference_fixture(name):
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
        obs_t = torch.empty((end - t, 1) + tuple(env.obs.shape[1:]), dtype=torch.float32, device=DEV)
        loc_t = torch.empty((end - t, 1) + tuple(env.obs_local.shape[1:]), dtype=torch.float32, device=DEV)
        env.rollout(acts, obs_t=obs_t, obs_local_t=loc_t, obs_every=1)
        for j in range(end - t):
            if not g["raised"][t + j]:
                assert (_bits(_np(obs_t)[j, 0]) == _bits(g["fov_planes"][t + j])).all(), (name, t + j)
                assert (_bits(_np(loc_t)[j, 0]) == _bits(g["loc_planes"][t + j])).all(), (name, t + j)
        t = end


# ---------------------------------------------------------------- 6. the Python surface
def test_python_surface_refusals():
    N, G = 64, 11
    env = _grid_env("shared", "v0", G, N)
    acts = torch.zeros((6, N), dtype=torch.int32, device=DEV)
    ok = torch.empty((2, N, G, G), dtype=torch.int32, device=DEV)
    bad = [dict(obs_t=torch.empty((3, N, G, G), dtype=torch.int32, device=DEV), obs_every=3),     # shape
           dict(obs_t=torch.empty((2, N, G, G), dtype=torch.float32, device=DEV), obs_every=3),   # dtype
           dict(obs_t=torch.empty((2, G, N, G), dtype=torch.int32, device=DEV).transpose(1, 2), obs_every=3),
           dict(obs_t=torch.empty((2, N, G, G), dtype=torch.int32), obs_every=3),                  # host tensor
           dict(obs_t=torch.empty(2 * N * G * G + 1, dtype=torch.int32, device=DEV)[1:].view(2, N, G, G), obs_every=3),
           dict(obs_t=ok, obs_every=0), dict(obs_t=None, obs_every=3), dict(obs_t=ok, obs_every=-1),
           dict(obs_t=ok, obs_every=3, device_epoch=True), dict(obs_t=ok)]
    for kw in bad:
        with pytest.raises(ValueError):
            env.rollout(acts, **kw)
    with pytest.raises(ValueError):
        env.capture_rollout(acts, obs_t=ok, obs_every=3)
    assert len(env.rollout(acts, obs_t=ok, obs_every=3)) == 3
    assert len(env.rollout(acts, trajectory=True, obs_t=ok, obs_every=3)) == 5
    # T = 0 and T < k: zero slots
    env.rollout(acts[:0], obs_t=ok[:0], obs_every=1)
    env.rollout(acts[:2], obs_t=ok[:0], obs_every=3)

    fov = PKG.LmazeFovealVecEnv(N, variant="v2", device=DEV)
    facts = torch.zeros((4, N), dtype=torch.int32, device=DEV)
    fok = torch.empty((4, N) + tuple(fov.obs.shape[1:]), dtype=torch.float32, device=DEV)
    for kw in [dict(obs_t=fok, obs_every=0),                                           # final-only: grid only
               dict(obs_t=fok, obs_every=1, obs_local_t=torch.empty((4, N, 4, 5, 5), device=DEV)),   # v5/v6 only
               dict(obs_t=fok[:, :, :1], obs_every=1), dict(obs_t=fok.double(), obs_every=1),
               dict(obs_t=fok, obs_every=1, device_epoch=True)]:
        with pytest.raises(ValueError):
            fov.rollout(facts, **kw)
    with pytest.raises(ValueError):
        fov.capture_rollout(facts, obs_t=fok, obs_every=1)
    assert len(fov.rollout(facts, obs_t=fok, obs_every=1)) == 3
    assert len(fov.rollout(facts, trajectory=True, obs_t=fok, obs_every=1)) == 5
    fov.rollout(facts[:0], obs_t=fok[:0], obs_every=1)
    fov.rollout(facts[:2], obs_t=fok[:0], obs_every=3)
