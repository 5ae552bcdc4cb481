"""GPU: the v5 / v6 visit map through renormalisation and deep decay, against the C oracle bit for bit -- every state field,
obs, obs_local and the materialised visit map.

The other v5 / v6 tests and reference recordings reset on globalDone under the reference's limits, so no clock of theirs
gets near LMAZE_VISIT_RENORM: the whole-map rewrite with a live "previous window" record, the record's rewrite after it,
workgroups that mix whole-map envs with window-pass envs, and cells below 2^-126 in a v5 / v6 window (the slow decode)
ran on no GPU.  The recipes (foveal_visit_range.py) reach all of it at 600 envs; what each test needs of its inputs is
asserted from the oracle's flags here, and with the oracle alone in test_foveal_visit_range_cpu.py.  The reference's own
walk through the same range is the recording v5_noreset_deepdecay_seed7, replayed by the fixture tests of
test_gpu_foveal.py, test_gpu_foveal_rollout.py and test_gpu_rollout_obs.py."""
import importlib
import os

import numpy as np
import pytest
import torch

import foveal_launch_matrix as M
import foveal_visit_range as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads():
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        O.set_threads(max(1, int(os.environ["OMP_NUM_THREADS"])))


def _np(t):
    return t.detach().cpu().numpy()


def _bytes(a):
    return np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a).view(np.uint8)


def _env(walk, variant="v5", hint=0, loaded=False, reset=True):
    """the env of a recipe: the oracle's layouts, seed and limits; every env waiting for its plannerStep"""
    env = PKG.LmazeFovealVecEnv(walk.n, variant=variant, layouts=list(walk.lay), device=DEV, seed=walk.seed,
                                env_base=walk.env_base, reset=reset)
    env.params.step_limit, env.params.foveal_step_limit = walk.p.step_limit, walk.p.foveal_step_limit
    env.params.launch_hint = hint
    if reset:
        env.foveal_done.fill_(True)
        walk.st.obs_local[...] = _np(env.obs_local)
    if loaded:
        env.load_visit(walk.st.visit)
    return env


def _same(env, st, tag):
    h = env.host_state()
    assert set(h) == set(R.STATE)
    for k in R.STATE:
        assert (_bytes(h[k]) == _bytes(getattr(st, k))).all(), (k, tag)
    for k in ("obs", "obs_local", "visit"):
        got, want = _bytes(getattr(env, k)), _bytes(getattr(st, k))
        if not (got == want).all():
            bad = np.flatnonzero((got.reshape(st.n, -1) != want.reshape(st.n, -1)).any(axis=1))
            raise AssertionError("%s %s: %d envs differ, first %d" % (k, tag, bad.size, bad[0]))


class _Clocks(object):
    """as test_v4_renormalisation_inside_rollout: the low byte of _visit_clock went down between two looks at an env that
    was not reset in between -- in how many blocks of 32?"""

    def __init__(self, env, walk):
        self.env, self.walk = env, walk
        self.last = _np(env._visit_clock) & 0xff
        self.wrapped = np.zeros(walk.n, bool)
        walk.mark()

    def look(self):
        now = _np(self.env._visit_clock) & 0xff
        self.wrapped |= (now < self.last) & self.walk.mark()
        self.last = now

    def blocks(self):
        return len(set(np.flatnonzero(self.wrapped) // 32))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- (a) hier_step, every step compared
@pytest.mark.parametrize("variant,G", [("v5", 18), ("v6", 18), ("v5", R.G_OFF)])
def test_hier_step_through_renormalisation_and_deep_decay(variant, G):
    walk, a, g = R.hier_case(variant, G)
    env = _env(walk, variant, loaded=G != 18)
    assert env.grid == G
    _same(env, walk.st, "start")
    clocks = _Clocks(env, walk)
    for t, at, gt, safe, epoch in R.hier_steps(walk, variant, a, g):
        if safe is not None:
            assert env._epoch == safe
            assert (_np(env.safe_foveal_goal()) == gt).all(), ("safe_foveal_goal", t)
        assert env._epoch == epoch
        env.hier_step(_dev(at), _dev(gt))
        _same(env, walk.st, (variant, G, t))
        clocks.look()
    c = walk.check_common()
    print("conditions %s G=%d: %s, clock wrapped in %d blocks" % (variant, G, c, clocks.blocks()))
    assert clocks.blocks() > 1


# ---------------------------------------------------------------- (b) plannerStep + step, never a reset, default limits
def test_planner_step_and_step_without_resets_under_the_default_limits():
    walk, a, g = R.noreset_case()
    env = _env(walk, loaded=True)
    assert (env.params.step_limit, env.params.foveal_step_limit) == (10, 50)
    clocks = _Clocks(env, walk)
    all_updated = True
    for t, m, gt, at in R.noreset_steps(walk, a, g):
        env.planner_step(_dev(gt), mask=_dev(m))
        env.step(_dev(at))
        _same(env, walk.st, ("noreset", t))
        clocks.look()
        if t >= R.T_NORESET - 100:
            all_updated &= bool(walk.st.foveal_done.all())
    c = R.check_noreset(walk, all_updated)
    print("conditions noreset: %s, clock wrapped in %d blocks" % (c, clocks.blocks()))
    assert clocks.blocks() > 1


# ---------------------------------------------------------------- (c) the one-launch forms
def test_one_launch_rollouts_through_renormalisation_and_deep_decay():
    walk, a, g = R.hier_case("v5", 18)
    env = _env(walk)
    a_d, g_d = _dev(a), _dev(g)
    clocks = _Clocks(env, walk)
    n = walk.n
    for call, sl, epoch, rows, slots, lslots in R.rollout_calls(walk, a, g):
        assert env._epoch == epoch
        obs_t = obs_local_t = None
        if slots is not None:
            obs_t = torch.full((sl.stop - sl.start, n, 7, 5, 5), float("nan"), dtype=torch.float32, device=DEV)
            obs_local_t = torch.full((sl.stop - sl.start, n, 4, 5, 5), float("nan"), dtype=torch.float32, device=DEV)
            out = env.rollout(a_d[sl], goals=g_d[sl], trajectory=True, obs_t=obs_t, obs_local_t=obs_local_t, obs_every=1)
        else:
            out = env.rollout(a_d[sl], goals=g_d[sl], trajectory=True)
        assert len(out) == 7
        for k, got in zip(("reward", "done", "foveal_reward", "foveal_done"), out[3:7]):
            got = got.contiguous()
            got = got.view(torch.uint8) if got.dtype == torch.bool else got
            assert (_bytes(got) == _bytes(rows[k])).all(), (k, call)
        _same(env, walk.st, ("rollout", call))
        if slots is not None:
            assert (_bytes(obs_t) == _bytes(slots)).all(), ("obs_t", call)
            assert (_bytes(obs_local_t) == _bytes(lslots)).all(), ("obs_local_t", call)
        clocks.look()
    c = walk.check_common()
    print("conditions rollouts: %s, clock wrapped in %d blocks" % (c, clocks.blocks()))
    assert call == 8 and clocks.blocks() > 1


# ---------------------------------------------------------------- (d) another launch hint
def _other_hint(params, n):
    """the first of LmazeFovealVecEnv.CANDIDATES with another envs-per-workgroup code than hint 0 that the launcher also
    runs with another number of envs per workgroup"""
    abi = PKG._abi
    p = abi.LmazeFovealParams.from_buffer_copy(params)
    p.launch_hint = 0
    epb0 = M.field(abi.describe_foveal_step(p, n, auto_reset=True), "envs_per_workgroup")
    for h in PKG.LmazeFovealVecEnv.CANDIDATES:
        p.launch_hint = h
        if (h >> 4) & 15 and M.field(abi.describe_foveal_step(p, n, auto_reset=True), "envs_per_workgroup") != epb0:
            return h
    raise AssertionError("no candidate with another workgroup size")


def test_launch_hint_does_not_change_the_far_range():
    walk, a, g = R.hier_case("v5", 18)
    ref = _env(walk)
    other = _env(walk, hint=_other_hint(ref.params, walk.n))
    assert other.params.launch_hint != 0 and ref.params.launch_hint == 0
    for t, at, gt, safe, epoch in R.hier_steps(walk, "v5", a, g):
        at, gt = _dev(at), _dev(gt)
        ref.hier_step(at, gt)
        other.hier_step(at, gt)
        if (t + 1) % 100 == 0:
            tag = ("hint 0x%x" % other.params.launch_hint, t)
            _same(ref, walk.st, ("hint 0", t))
            _same(other, walk.st, tag)
            assert torch.equal(ref._state, other._state) and torch.equal(ref._visit_clock, other._visit_clock), tag
            assert torch.equal(ref._visit_tiles.view(torch.int32), other._visit_tiles.view(torch.int32)), tag
    assert t + 1 == R.T
    walk.check_common()


# ---------------------------------------------------------------- (e) restore mid-run
def test_restored_state_reads_the_previous_window_from_decayed_tiles():
    """a fresh env takes every state field and the oracle's dense plane (load_visit: no "previous window" record), with last_xy
    pointed at windows that hold cells below 2^-126: plane 6 comes from the tiles through the slow decode"""
    walk, a, g, pointed = R.restore_case()
    env = _env(walk, reset=False)
    env.set_state(**{k: getattr(walk.st, k) for k in R.STATE})
    env.load_visit(walk.st.visit)
    env._epoch = 1 + R.T_RESTORE
    assert (_bytes(env.visit) == _bytes(walk.st.visit)).all()
    for t, at, gt, epoch in R.restore_steps(walk, a, g):
        assert env._epoch == epoch
        env.hier_step(_dev(at), _dev(gt))
        _same(env, walk.st, ("restored", t))
        if t == 0:
            shown = R.decayed(_np(env.obs)[:, 6])
            print("restore: %d envs pointed, %d decayed samples in plane 6 of %d envs" %
                  (len(pointed), int(shown.sum()), int(shown.reshape(walk.n, -1).any(axis=1).sum())))
            assert int(shown.sum()) >= 1
    assert t + 1 == R.T_AFTER
