"""GPU: the sampling closed-loop one-launch two-level rollout of v5/v6 (LmazeFovealVecEnv.rollout_hier_sample,
lmaze_v5_rollout_sample) against the C oracle's reset / plannerStep / step composed T times from the same state, with both keys,
the draw and both sums of compares restated in numpy (hier_sample_ref.py) -- never against the library's own step.  Bit for bit at
every step: key_t, actions_t, goals_t, goal_key_t, float32 bit patterns of both reward rows, both done rows and every recorded
slot of obs and obs_local; at the end every state tensor, obs, obs_local and the materialised visit map against the oracle's plane.

N = 333 (several workgroups at 32 envs, a partial last chunk, two chunks per workgroup under hint 0x120), T = 24 with both step
limits lowered to 4, env_base and epoch above 2^32, a fifth of the envs done and a fifth locally done on entry.  Tables: uniform,
peaked (zero-weight actions: equal thresholds) and raw words (unsorted, all-zero and all-ones rows).  The seeds were chosen on the
CPU with the oracle alone so that every case takes every path of the rule (test_hier_rollout_sample_cpu.py asserts it)."""
import importlib

import numpy as np
import pytest
import torch

import hier_sample_ref as R

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
ABI = importlib.import_module("gym-lmaze_amd._abi")
DEV = torch.device("cuda", 0)
HINTS = (0, 0x30, 0x40, 0x120)
PAD = 48                                            # sentinel bytes before and after the slots
IDS = dict(ids=R.shape_id)


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:                        # the same bits
        return torch.from_numpy(a.view(np.int32)).to(DEV)
    return torch.from_numpy(a).to(DEV)


def _env(shape, lays, start, start_visit, hint=0):
    env = PKG.LmazeFovealVecEnv(R.N, variant=shape.variant, layouts=lays, device=DEV, seed=R.SEED, env_base=R.ENV_BASE, reset=False)
    assert env.grid == shape.G
    env.params.step_limit, env.params.foveal_step_limit = R.STEP_LIMIT, R.FOVEAL_STEP_LIMIT   # through the env's params
    env.params.launch_hint = hint
    env.set_state(**start)
    env.load_visit(start_visit)
    env._epoch = R.EPOCH
    return env


def _guarded(shape):
    nbytes = 4 * int(np.prod(shape))
    buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    t = buf[PAD:PAD + nbytes].view(torch.float32).view(shape)
    assert t.data_ptr() % 16 == 0
    t.view(torch.uint8).fill_(0x5A)
    return buf, t


def _same(what, got, want):
    """bit for bit; the first differing row (step, or env) in the message"""
    got = got.contiguous()
    got = got.view(torch.uint8) if got.dtype == torch.bool else got
    want = _dev(want)
    assert got.shape == want.shape and got.element_size() == want.element_size(), (what, got.shape, want.shape)
    g, w = got.view(torch.uint8), want.view(torch.uint8)
    if torch.equal(g, w):
        return
    bad = (g.reshape(got.shape[0], -1) != w.reshape(got.shape[0], -1)).any(dim=1).nonzero()
    raise AssertionError("%s: %d of %d rows differ, first %d" % (what, bad.numel(), got.shape[0], int(bad[0])))


ROWS = ("reward", "done", "foveal_reward", "foveal_done", "action", "key", "goal", "goal_key")


def _rollout(env, ckey, controller_d, planner_d, every, T=R.T):
    """rollout_hier_sample with trajectory rows from sentinel buffers; ({name: rows}, obs_t, obs_local_t, their sentinel buffers)"""
    env.obs.view(torch.uint8).fill_(0xEE)
    env.obs_local.view(torch.uint8).fill_(0xEE)
    bufs = obs_t = obs_local_t = None
    if every:
        b0, obs_t = _guarded((T // every, R.N, env.channels, 5, 5))
        b1, obs_local_t = _guarded((T // every, R.N, 4, 5, 5))
        bufs = (b0, b1)
    given = {n: torch.full((T, R.N), -77, dtype=torch.int32, device=DEV) for n in ("actions_t", "key_t", "goals_t", "goal_key_t")}
    out = env.rollout_hier_sample(T, controller_thresholds=controller_d, planner_thresholds=planner_d, controller_key=ckey,
                                  trajectory=True, obs_t=obs_t, obs_local_t=obs_local_t, obs_every=every, **given)
    assert len(out) == 11 and out[0] is env.obs and all(a is b for a, b in zip(out[7:], given.values()))
    return dict(zip(ROWS, out[3:])), obs_t, obs_local_t, bufs


def _check(env, want, rows, obs_t, obs_local_t, bufs, every, tag):
    hs = env.host_state()
    for n in R.STATE:
        a, b = np.ascontiguousarray(hs[n]).view(np.uint8), np.ascontiguousarray(want.state[n]).view(np.uint8)
        assert a.shape == b.shape and (a == b).all(), (n, tag)
    _same("obs " + tag, env.obs, want.obs)
    _same("obs_local " + tag, env.obs_local, want.obs_local)
    _same("visit " + tag, env.visit, want.visit)
    assert set(rows) == set(want.rows), tag
    for n, w in want.rows.items():
        _same("%s rows %s" % (n, tag), rows[n], w)
    if every:
        _same("obs_t " + tag, obs_t, R.slots(want.obs_t, every))
        _same("obs_local_t " + tag, obs_local_t, R.slots(want.obs_local_t, every))
        for buf in bufs:
            assert (buf[:PAD] == 0xA5).all() and (buf[buf.numel() - PAD:] == 0xA5).all(), ("bytes beside the slots", tag)
    assert env._epoch == R.EPOCH + R.T, tag


@pytest.mark.parametrize("every", [None, 1, 5])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("ckey", R.CKEYS)
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_every_step_against_the_oracle(shape, ckey, kind, every):
    lays, lay, controller, planner, p, start, start_visit, want = R.case(shape, ckey, kind, R.SEEDS[shape])
    R.check_coverage(want.coverage, kind)                               # on the oracle's side
    env = _env(shape, lays, start, start_visit)
    L = lay.shape[0]
    assert (env.params.step_limit, env.params.foveal_step_limit, env.n_layouts) == (p.step_limit, p.foveal_step_limit, L)
    controller_d, planner_d = _dev(controller), _dev(planner)
    snap = env.snapshot()
    for h in HINTS:
        env.restore(snap)
        env.params.launch_hint = h
        line = ABI.describe_v5_rollout_sample(env.params, R.N, R.T, ckey, every or 0)
        assert " controller=%s planner=%s " % (R.controller_side(shape, L, ckey), shape.planner) in line, line
        assert line.startswith("foveal_hier_sample_kernel<v5, ") and (", obs_t>" in line) == bool(every), line
        rows, obs_t, obs_local_t, bufs = _rollout(env, ckey, controller_d, planner_d, every)
        torch.cuda.synchronize()
        _check(env, want, rows, obs_t, obs_local_t, bufs, every, "hint 0x%x: %s" % (h, line))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("ckey", R.CKEYS)
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_closed_loop_and_open_loop_over_its_rows_end_alike(shape, ckey, kind):
    """A cross-check only (the oracle run above is the proof): a twin env's rollout(actions_t, goals=goals_t with -1 -> 0) over
    the recorded rows (the goal of an env that does not plan is never read) -- state, visit map, both observations, the four
    reward / done rows and the epoch bit-identical."""
    lays, lay, controller, planner, p, start, start_visit, _ = R.case(shape, ckey, kind, R.SEEDS[shape])
    a, b = _env(shape, lays, start, start_visit), _env(shape, lays, start, start_visit)
    for env in (a, b):
        env.obs.view(torch.uint8).fill_(0xEE)
        env.obs_local.view(torch.uint8).fill_(0xEE)
    out = a.rollout_hier_sample(R.T, controller_thresholds=_dev(controller), planner_thresholds=_dev(planner), controller_key=ckey,
                                trajectory=True)
    actions_t, goals_t = out[7], out[9]
    assert int((goals_t == -1).sum()) > 0 and int(goals_t.max()) <= 24 and 0 <= int(actions_t.min()) and int(actions_t.max()) <= 3
    twin = b.rollout(actions_t, goals=goals_t.clamp(min=0), trajectory=True)
    torch.cuda.synchronize()
    assert torch.equal(a._state, b._state)
    assert torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32))
    assert torch.equal(a.obs_local.view(torch.int32), b.obs_local.view(torch.int32))
    assert torch.equal(a.visit.view(torch.int32), b.visit.view(torch.int32))
    assert len(twin) == 7
    for x, y in zip(out[3:7], twin[3:]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert a._epoch == R.EPOCH + R.T == b._epoch


@pytest.mark.parametrize("shape,ckey,kind", [(R.SHAPES[0], "offset", "peaked"), (R.SHAPES[1], "cell", "raw"), (R.SHAPES[2], "cell", "uniform"),
                                             (R.SHAPES[3], "offset", "raw")],
                         ids=lambda v: v if isinstance(v, str) else R.shape_id(v))
def test_launch_hint_never_changes_results(shape, ckey, kind):
    """every envs-per-workgroup code, chunk count and cap against hint 0, recording on: all outputs bit-identical"""
    lays, lay, controller, planner, p, start, start_visit, _ = R.case(shape, ckey, kind, R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    controller_d, planner_d = _dev(controller), _dev(planner)
    snap = env.snapshot()
    first, kernels = None, set()
    for h in (0, 0x10, 0x20, 0x30, 0x40, 0x50, 0x120, 0x230, 0x340, 0x25, 0x132, 0x48):
        env.restore(snap)
        env.params.launch_hint = h
        kernels.add(ABI.describe_v5_rollout_sample(env.params, R.N, R.T, ckey, 5).split(">")[0])
        rows, obs_t, obs_local_t, _ = _rollout(env, ckey, controller_d, planner_d, 5)
        torch.cuda.synchronize()
        got = [env._state.clone(), env.obs.clone().view(torch.int32), env.obs_local.clone().view(torch.int32),
               obs_t.clone().view(torch.int32), obs_local_t.clone().view(torch.int32), env.visit.view(torch.int32)]
        got += [rows[n].clone().view(torch.uint8) for n in sorted(rows)]
        if first is None:
            first = got
        assert all(torch.equal(x, y) for x, y in zip(got, first)), hex(h)
    assert len(kernels) == 3, kernels                                  # 32, 64 and 128 envs per workgroup, at any grid


@pytest.mark.parametrize("ckey", R.CKEYS)
@pytest.mark.parametrize("shape", R.SHAPES[1:], **IDS)
def test_state_and_controller_keys_are_the_next_rollouts_first_rows(shape, ckey):
    """After a rollout: controller_keys() is row 0 of the key_t the next rollout writes for the envs that enter it with neither
    flag set (they neither reset nor plan, and their goal rows are -1); state_keys() is row 0 of its goal_key_t for the envs that
    plan where they stand (locally done, not done) and, in cell mode, the planner part of everybody's controller key."""
    lays, lay, controller, planner, p, start, start_visit, _ = R.case(shape, ckey, "peaked", R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    tables = dict(controller_thresholds=_dev(controller), planner_thresholds=_dev(planner), controller_key=ckey)
    env.rollout_hier_sample(5, **tables)
    keys, ckeys = env.state_keys(), env.controller_keys(ckey)
    hs = env.host_state()
    want_c, _ = R.controller_keys(ckey, shape.G, lay.shape[0], hs["layout_id"], hs["ball_xy"], hs["fgoal_xy"])
    assert torch.equal(ckeys, _dev(want_c)) and torch.equal(keys, _dev(R.planner_keys(shape.G, lay.shape[0], hs["layout_id"], hs["ball_xy"])))
    gd, ld = env.done.bool().clone(), env.foveal_done.bool().clone()
    quiet, stands = ~gd & ~ld, ld & ~gd
    assert int(quiet.sum()) > 0 and int(stands.sum()) > 0 and int(gd.sum()) > 0
    out = env.rollout_hier_sample(3, trajectory=True, **tables)
    key0, goal0, goal_key0 = out[8][0], out[9][0], out[10][0]
    assert torch.equal(key0[quiet], ckeys[quiet])
    assert bool((goal0[quiet] == -1).all()) and bool((goal_key0[quiet] == -1).all())
    assert torch.equal(goal_key0[stands], keys[stands]) and bool((goal_key0[gd | ld] >= 0).all()) and bool((goal0[gd | ld] >= 0).all())
    if ckey == "cell":
        assert torch.equal(key0[~gd] // 100, keys[~gd])
    assert 0 <= int(ckeys.min()) and int(ckeys.max()) < controller.shape[0]


@pytest.mark.parametrize("shape,ckey", [(R.SHAPES[0], "offset"), (R.SHAPES[2], "cell")], ids=lambda v: v if isinstance(v, str) else R.shape_id(v))
def test_learner_rows(shape, ckey):
    """table_stats over the planner's rows and over the controller's equals np.add.at on the restatement's rows: the -1 entries
    of the planner's rows are skipped."""
    lays, lay, controller, planner, p, start, start_visit, want = R.case(shape, ckey, "peaked", R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    out = env.rollout_hier_sample(R.T, controller_thresholds=_dev(controller), planner_thresholds=_dev(planner), controller_key=ckey,
                                  trajectory=True)
    reward_t, foveal_reward_t, actions_t, key_t, goals_t, goal_key_t = out[3], out[5], out[7], out[8], out[9], out[10]
    for keys_d, ids_d, w_d, names, keys, A in ((goal_key_t, goals_t, reward_t, ("goal_key", "goal", "reward"), planner.shape[0], 25),
                                               (key_t, actions_t, foveal_reward_t, ("key", "action", "foveal_reward"), controller.shape[0], 4)):
        count, total = PKG.table_stats(keys_d, ids_d, w_d, keys=keys, actions=A)
        k, a, w = (want.rows[n].reshape(-1) for n in names)
        ok = (k >= 0) & (k < keys) & (a >= 0) & (a < A)
        assert ok.any() and ok.all() == (A == 4)                        # only the planner's rows have entries to skip
        want_count, want_total = np.zeros((keys, A), np.int64), np.zeros((keys, A), np.int64)
        np.add.at(want_count, (k[ok], a[ok]), 1)
        np.add.at(want_total, (k[ok], a[ok]), np.rint(w[ok].astype(np.float64) * 2.0 ** 24).astype(np.int64))
        assert torch.equal(count, _dev(want_count)) and torch.equal(total, _dev(want_total)), names
    assert int((goal_key_t == -1).sum()) > 0


def test_python_surface():
    """probs= / logits= / thresholds= give the same rows when they describe the same table (the softmax and the conversion run
    on the device in all three); the host's conversion of the same weights is the device's; T = 0 is a no-op that returns empty
    rows; v1/v2/v4, wrong table sizes, dtypes and devices raise (stream capture: the CPU suite)"""
    shape = R.SHAPES[2]
    lays, lay, controller, planner, p, start, start_visit, want = R.case(shape, "offset", "uniform", R.SEEDS[shape])
    gen = torch.Generator(device="cpu").manual_seed(4)
    cl = torch.randn(100, 4, generator=gen).to(DEV)
    pl = torch.randn(planner.shape[0], 25, generator=gen, dtype=torch.float64).to(DEV)
    cp, pp = torch.softmax(cl.double() / 0.3, -1), torch.softmax(pl.double() / 0.7, -1)
    ct, pt = ABI.sampling_thresholds(cp, actions=4), ABI.sampling_thresholds(pp, actions=25)
    assert ct.dtype == pt.dtype == torch.uint32 and tuple(ct.shape) == (100, 4) and tuple(pt.shape) == (planner.shape[0], 24)
    outs = []
    for kw in (dict(controller_logits=cl, planner_logits=pl, temperature=0.3, planner_temperature=0.7),
               dict(controller_probs=cp, planner_probs=pp),
               dict(controller_thresholds=ct, planner_thresholds=pt),
               dict(controller_thresholds=ct.view(torch.int32), planner_thresholds=pt.view(torch.int32)),   # int32: the same bits
               dict(controller_probs=cp, planner_logits=pl, planner_temperature=0.7),    # mixed; temperature is the controller's, unused
               dict(controller_logits=cl, temperature=0.3, planner_thresholds=pt)):
        env = _env(shape, lays, start, start_visit)
        outs.append(env.rollout_hier_sample(R.T, trajectory=True, **kw))
        assert env._epoch == R.EPOCH + R.T
    for other in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(outs[0][3:], other[3:]))
    assert int((outs[0][7] != 0).sum()) > 0 and int((outs[0][9] > 0).sum()) > 0
    # the uniform table: ones as weights are the restatement's thresholds, and its rows
    env = _env(shape, lays, start, start_visit)
    out = env.rollout_hier_sample(R.T, controller_probs=torch.ones(100, 4, device=DEV), planner_probs=torch.ones(planner.shape[0], 25, device=DEV),
                                  trajectory=True)
    for n, got in zip(ROWS, out[3:]):
        _same(n, got, want.rows[n])
    before = env._state.clone()
    controller_d, planner_d = _dev(controller), _dev(planner)
    out = env.rollout_hier_sample(0, controller_thresholds=controller_d, planner_thresholds=planner_d, trajectory=True)
    assert tuple(out[-1].shape) == (0, R.N) and torch.equal(env._state, before)
    ok = dict(controller_thresholds=controller_d, planner_thresholds=planner_d)
    for kw in (dict(ok, controller_thresholds=controller_d[:-1]), dict(ok, planner_thresholds=planner_d[:-1]),
               dict(ok, controller_thresholds=controller_d.to(torch.int64)), dict(ok, planner_thresholds=torch.from_numpy(planner.view(np.int32))),
               dict(ok, controller_key="cell"), dict(ok, obs_every=0), dict(ok, obs_t=torch.zeros(1, device=DEV)),
               dict(ok, obs_local_t=torch.zeros(1, device=DEV)), dict(ok, controller_thresholds=None, controller_probs=torch.ones(100, 5, device=DEV)),
               dict(ok, planner_thresholds=None, planner_probs=-torch.ones(planner.shape[0], 25, device=DEV)),
               dict(ok, goals_t=torch.zeros((R.T + 1, R.N), dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            env.rollout_hier_sample(R.T, **kw)
    assert torch.equal(env._state, before)
    flat = PKG.LmazeFovealVecEnv(8, variant="v2", device=DEV)
    with pytest.raises(ValueError):
        flat.rollout_hier_sample(4, **ok)
