"""GPU: the sampling closed-loop one-launch foveal rollout (LmazeFovealVecEnv.rollout_sample, lmaze_foveal_rollout_sample)
against the C oracle stepped T times from the same state, with the threshold conversion, the key, the draw and the sum of
compares restated in numpy (foveal_sample_ref.py) -- never against the library's own step.  Bit for bit at every step: key_t,
actions_t, float32 bit patterns of the reward rows, the done rows (both streams for v1), every recorded slot and the sentinel
bytes beside the slots; at the end every state tensor, obs, v4's materialised visit map against the oracle's plane and the
epoch.  No env-step is left out of a comparison.

N = 333 (several workgroups at 32 envs, a partial last chunk, two chunks per workgroup under hint 0x120), T = 24 with the
step limit lowered to 9, env_base and epoch above 2^32, a fifth of the envs done on entry.  Every case's coverage (fused
resets, goal rewards, moved windows, every action taken, none of zero probability) is asserted from the oracle's side before
anything is compared."""
import importlib

import numpy as np
import pytest
import torch

import foveal_sample_ref as R

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
ABI = importlib.import_module("gym-lmaze_amd._abi")
DEV = torch.device("cuda", 0)
HINTS = (0, 0x20, 0x30, 0x40, 0x120)
PAD = 48                                            # sentinel bytes before and after the slots


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).to(DEV).view(torch.uint32)
    return torch.from_numpy(a).to(DEV)


def _env(shape, lays, start, start_visit, hint=0, n=R.N, env_base=R.ENV_BASE, sl=slice(None)):
    env = PKG.LmazeFovealVecEnv(n, variant=shape.variant, layouts=lays, device=DEV, seed=R.SEED, env_base=env_base, reset=False)
    assert env.grid == shape.G
    env.params.step_limit = R.STEP_LIMIT                               # through the env's params
    env.params.launch_hint = hint
    env.set_state(**{k: v[sl] for k, v in start.items()})
    if env._has_visit:
        env.load_visit(start_visit[sl])
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


def _rollout(env, shape, auto_reset, every, **table):
    """rollout_sample with trajectory rows; ({name: rows}, obs_t, its sentinel buffer)"""
    env.obs.view(torch.uint8).fill_(0xEE)
    buf = obs_t = None
    if every:
        buf, obs_t = _guarded((R.T // every, env.num_envs, env.channels, 5, 5))
    out = env.rollout_sample(R.T, auto_reset=bool(auto_reset), trajectory=True, obs_t=obs_t, obs_every=every, **table)
    rows = {"reward": out[3], "done": out[4]}
    if shape.variant == "v1":
        assert len(out) == 9
        rows.update(foveal_reward=out[5], foveal_done=out[6])
    else:
        assert len(out) == 7
    rows.update(action=out[-2], key=out[-1])
    return rows, obs_t, buf


def _check(env, want, rows, obs_t, buf, tag):
    hs = env.host_state()
    for n in R.STATE:
        a, b = np.ascontiguousarray(hs[n]).view(np.uint8), np.ascontiguousarray(want.state[n]).view(np.uint8)
        assert a.shape == b.shape and (a == b).all(), (n, tag)
    _same("obs " + tag, env.obs, want.obs)
    if env._has_visit:
        _same("visit " + tag, env.visit, want.visit)
    assert set(rows) == set(want.rows), tag
    for n, w in want.rows.items():
        _same("%s rows %s" % (n, tag), rows[n], w)
    if want.slots is not None:
        _same("obs_t " + tag, obs_t, want.slots)
        assert (buf[:PAD] == 0xA5).all() and (buf[buf.numel() - PAD:] == 0xA5).all(), ("bytes beside the slots", tag)
    assert env._epoch == R.EPOCH + R.T, tag                            # whether or not auto_reset is set


def _line(env, shape, auto_reset, every):
    line = ABI.describe_foveal_rollout_sample(env.params, env.num_envs, R.T, bool(auto_reset), every or 0)
    assert " table=%s " % shape.table in line, line                    # which side of the rule the shape is on
    assert line.startswith("foveal_rollout_sample_kernel<v%s, " % shape.variant[1]), line
    assert (", obs_t>" in line) == bool(every) and ("fused-reset" in line) == bool(auto_reset), line
    return line


@pytest.mark.parametrize("every", [None, 1, 5])
@pytest.mark.parametrize("auto_reset", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_step_against_the_oracle(shape, auto_reset, every):
    """the rule matrix: every shape on its side of the table rule, plain and fused, recording or not, under five launch hints"""
    lays, lay, probs, table, p, start, start_visit, want = R.case(shape, auto_reset, every, R.SEEDS[shape])
    R.check_coverage(want.coverage, auto_reset, R.MIN_GOALS[shape])    # on the oracle's side
    env = _env(shape, lays, start, start_visit)
    assert (env.params.step_limit, env.n_layouts) == (p.step_limit, lay.shape[0])
    table_d = _dev(table)
    snap = env.snapshot()
    for h in HINTS:
        env.restore(snap)
        env.params.launch_hint = h
        line = _line(env, shape, auto_reset, every)
        rows, obs_t, buf = _rollout(env, shape, auto_reset, every, thresholds=table_d)
        torch.cuda.synchronize()
        _check(env, want, rows, obs_t, buf, "hint 0x%x: %s" % (h, line))


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3], R.SHAPES[4], R.SHAPES[7]], ids=R.shape_id)
def test_unsorted_raw_thresholds_follow_the_sum_of_compares(shape):
    """random uint32 words as thresholds=: one case per variant (v4 on both sides of the rule), fused reset, every 5th
    observation recorded.  Pins the sum of compares: a search would take other actions."""
    lays, lay, _, table, p, start, start_visit, want = R.case(shape, 1, 5, R.SEEDS[shape], True)
    R.check_coverage(want.coverage, 1, monotone=False)
    A = R.n_actions(shape.variant)
    c = table[want.rows["key"].reshape(-1), :A - 1]
    assert (np.diff(c.astype(np.int64), axis=1) < 0).any(axis=1).mean() > 0.5                 # the rows used are unsorted
    assert int(want.coverage["taken"].min()) > 0
    env = _env(shape, lays, start, start_visit)
    line = _line(env, shape, 1, 5)
    rows, obs_t, buf = _rollout(env, shape, 1, 5, thresholds=_dev(table))
    torch.cuda.synchronize()
    _check(env, want, rows, obs_t, buf, line)
    # int32 holds the same bits
    env2 = _env(shape, lays, start, start_visit)
    rows2, _, _ = _rollout(env2, shape, 1, 5, thresholds=_dev(table).view(torch.int32))
    assert all(torch.equal(rows[n].view(torch.uint8), rows2[n].view(torch.uint8)) for n in rows)


def _softmax64(x):
    x = x - x.max(axis=1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3], R.SHAPES[6]], ids=R.shape_id)
def test_conversions(shape):
    """probs= is thresholds=sampling_thresholds(probs, actions=A), word for word the numpy table; logits= with a temperature
    is the device's own sampling_thresholds(softmax(logits.double() / temperature)) exactly, and within one of a numpy
    softmax's table in every word (exp() is not the same to the last bit everywhere: test_gpu_rollout_sample.py)."""
    lays, lay, probs, table, p, start, start_visit, want = R.case(shape, 1, None, R.SEEDS[shape])
    A = R.n_actions(shape.variant)
    for dt in (torch.float64, torch.float32):
        pd = torch.from_numpy(probs).to(DEV).to(dt)
        td = ABI.sampling_thresholds(pd, actions=A)
        assert td.device == pd.device and td.dtype == torch.uint32 and tuple(td.shape) == table.shape
        assert (td.view(torch.int32).cpu().numpy().view(np.uint32) == R.thresholds(pd.cpu().numpy())).all()
    env = _env(shape, lays, start, start_visit)
    rows, obs_t, buf = _rollout(env, shape, 1, None, probs=torch.from_numpy(probs).to(DEV))
    torch.cuda.synchronize()
    _check(env, want, rows, obs_t, buf, "probs=")                      # the float64 weights give the case's own table
    # logits
    rs = np.random.RandomState(7)
    logits = (rs.randn(*probs.shape) * 3).astype(np.float32)
    temp = 0.7
    ld = torch.from_numpy(logits).to(DEV)
    mine = ABI.sampling_thresholds(torch.softmax(ld.double() / temp, -1), actions=A)
    ref = R.thresholds(_softmax64(logits.astype(np.float64) / temp))
    got = mine.view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.abs(got.astype(np.int64) - ref.astype(np.int64)).max() <= 1
    a, b = _env(shape, lays, start, start_visit), _env(shape, lays, start, start_visit)
    ra, _, _ = _rollout(a, shape, 1, None, logits=ld, temperature=temp)
    rb, _, _ = _rollout(b, shape, 1, None, thresholds=mine)
    torch.cuda.synchronize()
    assert torch.equal(a._state, b._state) and torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32))
    assert all(torch.equal(ra[n].view(torch.uint8), rb[n].view(torch.uint8)) for n in ra)
    # and against the oracle with the device's table
    lays, lay, _, _, p, start2, visit2, _ = R.case(shape, 1, None, R.SEEDS[shape])
    p2, st = R.P.start_state(shape, lay, R.SEEDS[shape])
    want2 = R.replay(shape, lay, got, p2, st, 1, None)
    _check(a, want2, ra, None, None, "logits=")


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[4], R.SHAPES[7]], ids=R.shape_id)
def test_two_half_batches_with_env_base_offsets_are_the_one_batch(shape):
    lays, lay, probs, table, p, start, start_visit, want = R.case(shape, 1, 1, R.SEEDS[shape])
    table_d = _dev(table)
    cut = 160
    got = {}
    for lo, hi in ((0, cut), (cut, R.N)):
        env = _env(shape, lays, start, start_visit, n=hi - lo, env_base=R.ENV_BASE + lo, sl=slice(lo, hi))
        rows, obs_t, buf = _rollout(env, shape, 1, 1, thresholds=table_d)
        torch.cuda.synchronize()
        hs = env.host_state()
        for n in R.STATE:
            assert (np.ascontiguousarray(hs[n]).view(np.uint8) == np.ascontiguousarray(want.state[n][lo:hi]).view(np.uint8)).all(), n
        _same("obs", env.obs, want.obs[lo:hi])
        if env._has_visit:
            _same("visit", env.visit, want.visit[lo:hi])
        for n, w in want.rows.items():
            _same(n, rows[n], w[:, lo:hi])
        _same("obs_t", obs_t, want.slots[:, lo:hi])
        assert (buf[:PAD] == 0xA5).all() and (buf[buf.numel() - PAD:] == 0xA5).all()
        got[lo] = env
    assert all(e._epoch == R.EPOCH + R.T for e in got.values())


def test_learner_rows():
    """rollout_sample -> gae -> table_stats(actions=25): the rows are what the learner kernels take; counts sum to T N and
    no (key, action) bin of zero probability is ever counted"""
    lm = PKG
    shape = R.SHAPES[4]                                                # v4, the shipped layouts
    lays, lay, probs, table, p, start, start_visit, want = R.case(shape, 1, None, R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    out = env.rollout_sample(R.T, probs=torch.from_numpy(probs).to(DEV), trajectory=True)
    reward_t, done_t, actions_t, key_t = out[3], out[4], out[5], out[6]
    S = table.shape[0]
    values = torch.zeros(S, dtype=torch.float32, device=DEV)
    adv, ret = lm.gae(reward_t, done_t, 0.9, 0.8, values=values, key_t=key_t, key_tail=env.state_keys())
    count, total = lm.table_stats(key_t, actions_t, adv, keys=S, actions=25)
    torch.cuda.synchronize()
    count = count.cpu().numpy().reshape(S, 25)
    assert int(count.sum()) == R.T * R.N
    w = R.widths(table, 25)
    assert (w == 0).any() and (count[w == 0] == 0).all()
    ref = np.zeros((S, 25), np.int64)
    np.add.at(ref, (want.rows["key"].reshape(-1), want.rows["action"].reshape(-1)), 1)
    assert (count == ref).all()
    assert tuple(adv.shape) == (R.T, R.N) and bool(torch.isfinite(adv).all()) and tuple(ret.shape) == (R.T, R.N)


def test_python_surface():
    """T = 0 is a no-op that returns empty rows; v5/v6 and bad arguments raise"""
    shape = R.SHAPES[3]
    lays, lay, probs, table, p, start, start_visit, want = R.case(shape, 1, None, R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    td, pd = _dev(table), torch.from_numpy(probs).to(DEV)
    before = env._state.clone()
    out = env.rollout_sample(0, thresholds=td, trajectory=True)
    assert tuple(out[-1].shape) == (0, R.N) and torch.equal(env._state, before) and env._epoch == R.EPOCH
    odd = torch.zeros(table.size + 1, dtype=torch.int32, device=DEV)[1:].view(table.shape)      # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 != 0
    for kw in (dict(), dict(probs=pd, thresholds=td), dict(probs=pd[:-1]), dict(probs=pd[:, :24]), dict(probs=pd.cpu()),
               dict(probs=pd.to(torch.int32)), dict(logits=pd, temperature=0.0), dict(logits=pd, temperature=-1.0),
               dict(thresholds=td[:-1]), dict(thresholds=td.view(torch.int32).to(torch.int64)), dict(thresholds=odd),
               dict(thresholds=torch.zeros((table.shape[0], 25), dtype=torch.int32, device=DEV)),
               dict(thresholds=td, obs_every=0), dict(thresholds=td, obs_t=torch.zeros(1, device=DEV)),
               dict(thresholds=td, actions_t=torch.zeros((R.T + 1, R.N), dtype=torch.int32, device=DEV)),
               dict(probs=-pd), dict(probs=torch.zeros_like(pd))):
        with pytest.raises(ValueError):
            env.rollout_sample(R.T, **kw)
    with pytest.raises(ValueError):
        env.rollout_sample(-1, thresholds=td)
    assert env._epoch == R.EPOCH and torch.equal(env._state, before)   # nothing was launched
    two = PKG.LmazeFovealVecEnv(8, variant="v5", device=DEV)
    with pytest.raises(ValueError):
        two.rollout_sample(4, probs=torch.ones(5 * 18 * 18, 25, device=DEV))
