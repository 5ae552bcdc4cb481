"""GPU: every row of foveal_launch_matrix.ROWS -- every kernel instantiation, envs-per-workgroup size, chunk count, LDS
cap and store flavour a launch_hint (or the launcher's own default) can pick for the foveal variants -- against the C
oracle stepping the same envs, bit for bit: every field of the state, float32 bit patterns of obs and obs_local, the
materialised visit map against the oracle's dense plane, every per-step reward / done row of both streams, every
recorded slot of obs_t and obs_local_t, the sentinel bytes beside the slots, and the host epoch.

The oracle is the only reference: the state a group starts from is made on the host by the oracle itself (reset, foveal
goals, a few warm-up steps for a non-trivial visit map, then step counts near their limits and done flags injected) and
loaded into the env.  For the fused entries it runs reset(mask = done, place = 1, seed, epoch + t) then step, for v5 / v6
v5_hier_step.  Rows that differ only in their hint share one env (restored between hints) and one oracle run.

The streaming sizes (290 000 - 500 000 envs, T = 2) are compared whole, on the device, not on windows: measured on an
MI355X the slowest of those cases takes 0.4 s, the 238 groups together 13 s, and the describe sweep of the coverage
test 4 s."""
import importlib
import os
import zlib

import numpy as np
import pytest
import torch

import foveal_launch_matrix as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
DEV = torch.device("cuda", 0)
SEED, ENV_BASE, EPOCH0 = 21, 4099, (1 << 32) + 5
PAD = 48                                            # sentinel bytes before and after the slots
GROUPS = M.groups()
VID = {"v1": O.VARIANT_V1, "v2": O.VARIANT_V2, "v4": O.VARIANT_V4, "v5": O.VARIANT_V5, "v6": O.VARIANT_V6}
STATE = ("ball_xy", "goal_xy", "fgoal_xy", "layout_id", "step_count", "foveal_step_count", "reward", "foveal_reward", "done",
         "foveal_done", "ball1_xy", "fovea_xy", "last_xy", "foveal_goal")


def _id(key):
    entry, variant, G, L, N, T, k = key
    return "%s-%s-G%d-L%d-N%d-T%d%s" % (entry, variant, G, L, N, T, "" if k is None else "-k%d" % k)


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads():
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        O.set_threads(max(1, int(os.environ["OMP_NUM_THREADS"])))


def _oracle_step(key, p, lay, st, acts, goals, epoch):
    """one step of the row's entry point in the oracle"""
    entry, variant = key[0], key[1]
    two = variant in M.TWO_LEVEL
    resets = entry in (M.STEP_RESET, M.ROLLOUT, M.ROLLOUT_OBS)
    if two:
        if resets:
            O.v5_hier_step(p, lay, acts, goals, SEED, epoch, st, env_base=ENV_BASE)
        else:
            O.v5_step(p, lay, acts, st)
    else:
        if resets:
            O.foveal_reset(p, lay, st.done.copy(), 1, SEED, epoch, st, env_base=ENV_BASE)
        O.foveal_step(p, lay, acts, st)


def _group(key):
    """(env, oracle params, layouts, the oracle's state = the env's, actions, planner goals) of a group: episodes end inside
    the run, a tenth of the envs is done on entry, the visit map is not the fresh one"""
    entry, variant, G, L, N, T, k = key
    seed = zlib.crc32(repr(key).encode())
    rs = np.random.RandomState(seed)
    two = variant in M.TWO_LEVEL
    lays = M.layouts(G, L, seed)
    lay = np.ascontiguousarray(np.stack(lays))
    env = PKG.LmazeFovealVecEnv(N, variant=variant, layouts=lays, device=DEV, seed=SEED, env_base=ENV_BASE, reset=False)
    assert env.grid == G and env.n_layouts == L
    p = O.foveal_params(VID[variant], G, L)
    assert (p.step_limit, p.foveal_step_limit) == (env.params.step_limit, env.params.foveal_step_limit)
    st = O.FovealState(VID[variant], N, G)
    if two:
        O.v5_reset(p, lay, None, 1, SEED, EPOCH0 - 1, st, env_base=ENV_BASE)
        O.v5_planner_step(p, lay, rs.randint(0, 25, N).astype(np.int32), None, st)
    else:
        O.foveal_reset(p, lay, None, 1, SEED, EPOCH0 - 1, st, env_base=ENV_BASE)
        if variant == "v1":
            c = int(np.flatnonzero(lay[0].reshape(-1) == ord("X"))[0])  # v1's goal is the 'X' cell; no step or reset moves it
            st.goal_xy[...] = (c // G, c % G)
            O.v1_set_foveal_goal(p, lay, rs.randint(0, 5, (N, 2)).astype(np.int32), (rs.rand(N) < 0.7).astype(np.uint8), st)
    hi = 4 if variant == "v1" or two else 25
    for _ in range(3):                                              # warm-up: a visit map with history (v4, v5, v6)
        a = rs.randint(0, hi, N).astype(np.int32)
        if two:
            O.v5_step(p, lay, a, st)
        else:
            O.foveal_step(p, lay, a, st)
    near = rs.rand(N) < 0.4
    st.step_count[near] = p.step_limit - rs.randint(0, 3, int(near.sum()))
    if variant == "v1" or two:
        near = rs.rand(N) < 0.3
        st.foveal_step_count[near] = p.foveal_step_limit - rs.randint(0, 3, int(near.sum()))
    st.done[...] = rs.rand(N) < 0.1
    if two:
        st.foveal_done[...] = rs.rand(N) < 0.3
    env.set_state(**{name: getattr(st, name) for name in STATE})
    if env._has_visit:
        env.load_visit(st.visit)
    env._epoch = EPOCH0
    # actions with out-of-range ids.  An out-of-range v2 / v4 action skips the env, and a chunk with a skipped env renders
    # through the scalar path: such ids sit in a window of 24 envs that moves with t, so most chunks keep the vector path
    acts = rs.randint(0, hi, (T, N)).astype(np.int32)
    for t in range(T):
        s = (t * 977) % N
        w = acts[t, s:s + 24]
        bad = rs.rand(w.size) < 0.5
        w[bad] = rs.choice(np.array([-1, hi], np.int32), int(bad.sum()))
    if variant == "v1" or two:                                      # no skipping there: anywhere
        bad = rs.rand(T, N) < 0.05
        acts[bad] = rs.choice(np.array([-1, hi], np.int32), int(bad.sum()))
    goals = None
    if two:
        goals = rs.randint(0, 25, (T, N)).astype(np.int32)
        bad = rs.rand(T, N) < 0.05
        goals[bad] = rs.choice(np.array([-1, 25, 26], np.int32), int(bad.sum()))
    return env, p, lay, st, acts, goals


def _oracle(key, p, lay, st, acts, goals):
    """what T oracle steps from st leave, on the device: state (host), obs, obs_local, visit, the four row streams, the
    recorded slots, the epoch after.  Observations start as the sentinel the GPU side starts from: an env that is never
    stepped keeps it on both sides."""
    entry, variant, G, L, N, T, k = key
    st.obs.view(np.uint8)[...] = 0xEE
    st.obs_local.view(np.uint8)[...] = 0xEE
    rows = {n: [] for n in ("reward", "done", "foveal_reward", "foveal_done")}
    slots, lslots = [], []
    for t in range(T):
        _oracle_step(key, p, lay, st, acts[t], None if goals is None else goals[t], EPOCH0 + t)
        for n in rows:
            rows[n].append(getattr(st, n).copy())
        if k and (t + 1) % k == 0:
            slots.append(st.obs.copy())
            lslots.append(st.obs_local.copy())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    want = {n: dev(np.stack(v)) for n, v in rows.items()}
    want.update(obs=dev(st.obs), obs_local=dev(st.obs_local), visit=dev(st.visit))
    want["slots"] = dev(np.stack(slots)) if slots else None
    want["lslots"] = dev(np.stack(lslots)) if lslots else None
    resets = entry in (M.STEP_RESET, M.ROLLOUT, M.ROLLOUT_OBS)
    return want, EPOCH0 + (T if resets else 0)


def _guarded(shape):
    """a float32 tensor of this shape inside sentinel bytes, PAD before and PAD after; 16-byte aligned"""
    nbytes = 4 * int(np.prod(shape))
    buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    t = buf[PAD:PAD + nbytes].view(torch.float32).view(shape)
    assert t.data_ptr() % 16 == 0
    t.view(torch.uint8).fill_(0x5A)
    return buf, t


def _run(key, env, acts_d, goals_d):
    """the row's entry point under env.params.launch_hint: ({stream: rows}, obs_t, obs_local_t, their sentinel buffers)"""
    entry, variant, G, L, N, T, k = key
    two = variant in M.TWO_LEVEL
    resets = entry in (M.STEP_RESET, M.ROLLOUT, M.ROLLOUT_OBS)
    env.obs.view(torch.uint8).fill_(0xEE)
    if two:
        env.obs_local.view(torch.uint8).fill_(0xEE)
    if entry in (M.STEP, M.STEP_RESET):
        rows = {n: [] for n in ("reward", "done", "foveal_reward", "foveal_done")}
        for t in range(T):
            if two and resets:
                env.hier_step(acts_d[t], goals_d[t])
            else:
                env.step(acts_d[t], auto_reset=resets)
            for n in rows:
                rows[n].append(getattr(env, n).clone())
        return {n: torch.stack(v) for n, v in rows.items()}, None, None, ()
    bufs, obs_t, obs_local_t = (), None, None
    if k:
        b0, obs_t = _guarded((T // k, N, env.channels, 5, 5))
        bufs = (b0,)
        if two:
            b1, obs_local_t = _guarded((T // k, N, 4, 5, 5))
            bufs = (b0, b1)
    out = env.rollout(acts_d, goals=goals_d if two and resets else None, auto_reset=resets and not two, trajectory=True,
                      obs_t=obs_t, obs_local_t=obs_local_t, obs_every=k)
    rows = {"reward": out[3], "done": out[4]}
    if len(out) > 5:
        rows.update(foveal_reward=out[5], foveal_done=out[6])
    return rows, obs_t, obs_local_t, bufs


def _same(what, got, want):
    """bit for bit, on the device; the first differing env (or step) in the message"""
    got = got.contiguous()
    got = got.view(torch.uint8) if got.dtype == torch.bool else got
    assert got.shape == want.shape and got.element_size() == want.element_size(), (what, got.shape, want.shape)
    g, w = got.view(torch.uint8), want.view(torch.uint8)
    if torch.equal(g, w):
        return
    bad = (g.reshape(got.shape[0], -1) != w.reshape(got.shape[0], -1)).any(dim=1).nonzero()
    raise AssertionError("%s: %d of %d rows differ, first %d" % (what, bad.numel(), got.shape[0], int(bad[0])))


@pytest.mark.parametrize("key", sorted(GROUPS, key=str), ids=_id)
def test_every_foveal_launch_hint_matches_the_oracle(key):
    entry, variant, G, L, N, T, k = key
    two = variant in M.TWO_LEVEL
    env, p, lay, st, acts, goals = _group(key)
    acts_d = torch.from_numpy(acts).to(DEV)
    goals_d = torch.from_numpy(goals).to(DEV) if goals is not None else None
    snap = env.snapshot()
    want, epoch = _oracle(key, p, lay, st, acts, goals)
    for h in GROUPS[key]:
        env.restore(snap)
        env.params.launch_hint = h
        rows, obs_t, obs_local_t, bufs = _run(key, env, acts_d, goals_d)
        torch.cuda.synchronize()
        tag = "hint 0x%x: %s" % (h, M.describe(PKG._abi, *key, h))
        hs = env.host_state()
        assert set(hs) == set(STATE)
        for n in STATE:
            a, b = np.ascontiguousarray(hs[n]).view(np.uint8), np.ascontiguousarray(getattr(st, n)).view(np.uint8)
            assert a.shape == b.shape and (a == b).all(), (n, tag)
        _same("obs " + tag, env.obs, want["obs"])
        if two:
            _same("obs_local " + tag, env.obs_local, want["obs_local"])
        if env._has_visit:
            _same("visit " + tag, env.visit, want["visit"])
        streams = ("reward", "done", "foveal_reward", "foveal_done") if variant == "v1" or two else ("reward", "done")
        assert set(rows) >= set(streams), tag
        for n in streams:
            _same("%s rows %s" % (n, tag), rows[n], want[n])
        if k:
            _same("obs_t " + tag, obs_t, want["slots"])
            if two:
                _same("obs_local_t " + tag, obs_local_t, want["lslots"])
        for buf in bufs:
            assert (buf[:PAD] == 0xA5).all() and (buf[buf.numel() - PAD:] == 0xA5).all(), ("bytes beside the slots", tag)
        assert env._epoch == epoch, tag


def test_refused_recording_forms_record_through_step_launches():
    """v1 off G = 14 and v5 / v6 off G = 18: the C layer refuses the one-launch recording form by its arguments
    (LMAZE_E_GRID, nothing queued), the table still holds those shapes -- LmazeFovealVecEnv.rollout takes T launches"""
    abi = PKG._abi
    shapes = {(r.variant, r.G) for r in M.ROWS if r.entry in M.RECORDING and not M.one_launch(r.entry, r.variant, r.G)}
    assert {("v1", 13), ("v5", 13)} <= shapes
    for variant, G in (("v1", 13), ("v5", 13), ("v6", 33)):
        with pytest.raises(abi.LmazeError) as e:
            abi.describe_foveal_rollout(M.params(abi, variant, G, M.default_layouts(variant)), 1000, 8, True,
                                        variant in M.TWO_LEVEL, obs_every=3)
        assert e.value.code == M.E_GRID


def test_every_kernel_named_under_the_device_limit_has_a_row():
    """the CPU module's coverage assertion again, with the launcher asking this device for its LDS limit (the halving
    fallback lands elsewhere than under the 64 KiB it assumes without one), and every plan within 160 KiB.  The sweep
    describes 1.5 million launches: about four seconds of host time, nothing is queued."""
    abi = PKG._abi
    by_text = M.swept(abi)
    M.check_coverage(abi, by_text, 480)
    for text, calls in by_text.items():
        lds, epb, grid, chunks = (M.field(text, f) for f in ("lds", "envs_per_workgroup", "grid", "chunks"))
        assert lds <= M.LDS_PER_WORKGROUP, (calls[0], text)
        assert grid >= 1 and all(grid * epb * chunks >= c[4] for c in calls), (calls[0], text)
