"""GPU: the closed-loop one-launch foveal rollout (LmazeFovealVecEnv.rollout_policy, lmaze_foveal_rollout_policy) against the
C oracle stepped T times from the same state, with the table lookup and the draw restated in numpy (foveal_policy_ref.py) --
never against the library's own step.  Bit for bit at every step: key_t, actions_t, float32 bit patterns of the reward rows,
the done rows (both streams for v1) and every recorded slot; at the end every state tensor, obs and, v4, the materialised
visit map against the oracle's plane.  No env-step is left out of a comparison.

N = 333 (several workgroups at 32 envs, a partial last chunk, two chunks per workgroup under hint 0x120), T = 24 with the
step limit lowered to 9, env_base and epoch above 2^32, a fifth of the envs done on entry, step counts spread up to the
limit, a tenth of the table's ids outside the action range.  The seeds were chosen on the CPU with the oracle alone so
that every case takes every path of the rule its parameters allow (foveal_policy_ref.expected_paths)."""
import importlib

import numpy as np
import pytest
import torch

import foveal_policy_ref as R

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
ABI = importlib.import_module("gym-lmaze_amd._abi")
DEV = torch.device("cuda", 0)
HINTS = (0, 0x20, 0x30, 0x40, 0x120)
PAD = 48                                            # sentinel bytes before and after the slots


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _env(shape, lays, start, start_visit, hint=0):
    env = PKG.LmazeFovealVecEnv(R.N, variant=shape.variant, layouts=lays, device=DEV, seed=R.SEED, env_base=R.ENV_BASE, reset=False)
    assert env.grid == shape.G
    env.params.step_limit = R.STEP_LIMIT                               # through the env's params
    env.params.launch_hint = hint
    env.set_state(**start)
    if env._has_visit:
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


def _rollout(env, shape, table_d, eps, auto_reset, every):
    """rollout_policy with trajectory rows; ({name: rows}, obs_t, its sentinel buffer)"""
    env.obs.view(torch.uint8).fill_(0xEE)
    buf = obs_t = None
    if every:
        buf, obs_t = _guarded((R.T // every, R.N, env.channels, 5, 5))
    out = env.rollout_policy(R.T, policy=table_d, epsilon=eps, auto_reset=bool(auto_reset), trajectory=True, obs_t=obs_t,
                             obs_every=every)
    rows = {"reward": out[3], "done": out[4]}
    if shape.variant == "v1":
        assert len(out) == 9
        rows.update(foveal_reward=out[5], foveal_done=out[6])
    else:
        assert len(out) == 7
    rows.update(action=out[-2], key=out[-1])
    return rows, obs_t, buf


def _check(env, shape, want, rows, obs_t, buf, tag):
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


@pytest.mark.parametrize("every", [None, 1, 5])
@pytest.mark.parametrize("auto_reset", [0, 1])
@pytest.mark.parametrize("eps", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%s-G%d-%s" % (s.variant, s.G, s.table))
def test_every_step_against_the_oracle(shape, eps, auto_reset, every):
    lays, lay, table, p, start, start_visit, want = R.case(shape, eps, auto_reset, every, R.SEEDS[shape])
    for path in R.expected_paths(shape.variant, eps, auto_reset):      # on the oracle's side
        assert want.coverage[path] > 0, (path, want.coverage)
    env = _env(shape, lays, start, start_visit)
    assert (env.params.step_limit, env.n_layouts) == (p.step_limit, lay.shape[0])
    table_d = _dev(table)
    snap = env.snapshot()
    for h in HINTS:
        env.restore(snap)
        env.params.launch_hint = h
        line = ABI.describe_foveal_rollout_policy(env.params, R.N, R.T, bool(auto_reset), every or 0)
        assert " table=%s " % shape.table in line, line                # which side of the rule the shape is on
        assert line.startswith("foveal_rollout_policy_kernel<v%s, " % shape.variant[1]), line
        assert (", obs_t>" in line) == bool(every) and ("fused-reset" in line) == bool(auto_reset), line
        rows, obs_t, buf = _rollout(env, shape, table_d, eps, auto_reset, every)
        torch.cuda.synchronize()
        _check(env, shape, want, rows, obs_t, buf, "hint 0x%x: %s" % (h, line))


@pytest.mark.parametrize("auto_reset", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES[:3] + R.SHAPES[5:], ids=lambda s: "%s-G%d-%s" % (s.variant, s.G, s.table))
def test_greedy_closed_loop_and_open_loop_over_its_actions_end_alike(shape, auto_reset):
    """A cross-check only (the oracle run above is the proof): epsilon = 0, then a twin env's rollout(actions_t) over the
    recorded actions -- state, obs, visit map, rows and epoch bit-identical."""
    lays, lay, table, p, start, start_visit, _ = R.case(shape, 0.0, auto_reset, None, R.SEEDS[shape])
    a, b = _env(shape, lays, start, start_visit), _env(shape, lays, start, start_visit)
    for env in (a, b):
        env.obs.view(torch.uint8).fill_(0xEE)
    out = a.rollout_policy(R.T, policy=_dev(table), epsilon=0.0, auto_reset=bool(auto_reset), trajectory=True)
    twin = b.rollout(out[-2], auto_reset=bool(auto_reset), trajectory=True)
    torch.cuda.synchronize()
    assert torch.equal(a._state, b._state) and torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32))
    if a._has_visit:
        assert torch.equal(a.visit.view(torch.int32), b.visit.view(torch.int32))
    for x, y in zip(out[3:-2], twin[3:]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert a._epoch == R.EPOCH + R.T and b._epoch == R.EPOCH + (R.T if auto_reset else 0)


@pytest.mark.parametrize("shape", R.SHAPES[:2] + R.SHAPES[4:], ids=lambda s: "%s-G%d-%s" % (s.variant, s.G, s.table))
def test_launch_hint_never_changes_results(shape):
    """every envs-per-workgroup code, chunk count and cap against hint 0, recording on: all outputs bit-identical"""
    lays, lay, table, p, start, start_visit, _ = R.case(shape, 0.25, 1, 5, R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    table_d = _dev(table)
    snap = env.snapshot()
    first = None
    for h in (0, 0x10, 0x20, 0x30, 0x40, 0x50, 0x120, 0x230, 0x340, 0x25, 0x132, 0x48):
        env.restore(snap)
        env.params.launch_hint = h
        rows, obs_t, _ = _rollout(env, shape, table_d, 0.25, 1, 5)
        torch.cuda.synchronize()
        got = [env._state.clone(), env.obs.clone().view(torch.int32), obs_t.clone().view(torch.int32)]
        got += [rows[n].clone().view(torch.uint8) for n in sorted(rows)]
        if env._has_visit:
            got.append(env.visit.view(torch.int32))
        if first is None:
            first = got
        assert all(torch.equal(x, y) for x, y in zip(got, first)), hex(h)


@pytest.mark.parametrize("shape", R.SHAPES[:3], ids=lambda s: s.variant)
def test_state_keys_are_the_next_rollouts_first_key_row(shape):
    """no env done: state_keys() is row 0 of the key_t the next rollout writes -- and after it, the key_tail of gae()"""
    lays, lay, table, p, start, start_visit, _ = R.case(shape, 0.0, 1, None, R.SEEDS[shape])
    start = dict(start, done=np.zeros_like(start["done"]))
    if shape.variant != "v1":                                          # ids outside 0..L-1 are clamped, as the step clamps them
        lid = start["layout_id"].copy()
        lid[:4] = (-3, lay.shape[0], 99, -1)
        start["layout_id"] = lid
    env = _env(shape, lays, start, start_visit)
    keys = env.state_keys()
    assert keys.dtype == torch.int32 and tuple(keys.shape) == (R.N,)
    want = R.keys_of(shape.variant, shape.G, lay.shape[0], start["layout_id"], start["ball_xy"])
    assert torch.equal(keys, _dev(want))
    out = env.rollout_policy(3, policy=_dev(table), epsilon=0.5, auto_reset=True, trajectory=True)
    assert torch.equal(out[-1][0], keys)
    assert 0 <= int(keys.min()) and int(keys.max()) < lay.shape[0] * shape.G * shape.G


def test_python_surface():
    """q= is reduced by greedy_table; T = 0 is a no-op that returns empty rows; v5/v6 and bad arguments raise"""
    shape = R.SHAPES[1]
    lays, lay, table, p, start, start_visit, want = R.case(shape, 0.0, 1, None, R.SEEDS[shape])
    env = _env(shape, lays, start, start_visit)
    entries = lay.shape[0] * shape.G * shape.G
    good = table.astype(np.int64) % 25
    q = np.zeros((entries, 25), np.float32)
    q[np.arange(entries), good] = 1.0
    a = env.rollout_policy(R.T, q=_dev(q), trajectory=True)
    b = _env(shape, lays, start, start_visit).rollout_policy(R.T, policy=_dev(good.astype(np.uint8)), trajectory=True)
    assert torch.equal(a[-2], b[-2]) and torch.equal(a[-1], b[-1])
    before = env._state.clone()
    out = env.rollout_policy(0, policy=_dev(table), trajectory=True)
    assert tuple(out[-1].shape) == (0, R.N) and torch.equal(env._state, before)
    for kw in (dict(), dict(policy=_dev(table), q=_dev(q)), dict(policy=_dev(table[:-1])), dict(policy=_dev(table.astype(np.int32))),
               dict(policy=torch.from_numpy(table)), dict(policy=_dev(table), epsilon=1.5), dict(policy=_dev(table), obs_every=0),
               dict(policy=_dev(table), obs_t=torch.zeros(1, device=DEV)),
               dict(policy=_dev(table), actions_t=torch.zeros((R.T + 1, R.N), dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            env.rollout_policy(R.T, **kw)
    with pytest.raises(ValueError):
        env.rollout_policy(-1, policy=_dev(table))
    two = PKG.LmazeFovealVecEnv(8, variant="v5", device=DEV)
    with pytest.raises(ValueError):
        two.rollout_policy(4, policy=torch.zeros(5 * 18 * 18, dtype=torch.uint8, device=DEV))
