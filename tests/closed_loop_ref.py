"""The closed-loop one-launch rollouts (include/lmaze.h lmaze_rollout_policy / lmaze_rollout_sample and their kin) restated
on the host, for the tests of every form: the Philox draw, the sampling rule, the LDS a launch needs, the envs the GPU
tests start from, and the replay of one rollout call against the C oracle stepped T times.  Importing it needs no GPU."""
import functools
import importlib
import re

import numpy as np
import torch

import oracle_lib as O
from helpers import bordered_random_layouts, f32_bits

M32 = np.uint64(0xFFFFFFFF)
TOP = 0xFFFFFFFF
ENV_BASE = (1 << 33) + 1000          # both words of the global env index and of the epoch enter the draws
EPOCH = (1 << 35) + 77
DEV = torch.device("cuda", 0)


def to_numpy(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------- the draws
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (Salmon et al., SC'11); checked against the oracle's and the
    Random123 vectors below."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def explore_draw(seed, ep, env_global):
    """The closed loop's draw of (env, epoch), four words: the reset draw's counter with the top bit of its last word
    flipped.  The epsilon-greedy forms explore on .x and take their uniform action from .y; the sampling forms compare .x."""
    e = np.asarray(env_global, dtype=np.uint64)
    ep = np.uint64(ep)
    return philox(e & M32, e >> np.uint64(32), ep & M32, ((ep >> np.uint64(32)) & M32) ^ np.uint64(0x80000000),
                  np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32))


def sample_action(rows, r):
    """(r >= c0) + (r >= c1) + (r >= c2), unsigned, whatever the row holds."""
    c = rows.astype(np.uint64)
    return ((r >= c[:, 0]).astype(np.int32) + (r >= c[:, 1]) + (r >= c[:, 2])).astype(np.int32)


# The two checks of philox() itself.  They are tests: a test module that draws with philox() imports them by name, which
# collects them there.
def test_numpy_philox_is_the_oracles():
    rs = np.random.RandomState(5)
    w = rs.randint(0, 1 << 32, (64, 6), dtype=np.uint64)
    w[0] = 0
    w[1] = (1 << 32) - 1
    got = np.stack(philox(w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[0, 4], w[0, 5]), axis=1)
    for i in range(64):
        assert [int(x) for x in got[i]] == O.philox4x32_10([int(x) for x in w[i, :4]], [int(w[0, 4]), int(w[0, 5])]), i


def test_numpy_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10."""
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((TOP, TOP, TOP, TOP), (TOP, TOP), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = philox(*([c] for c in ctr), *key)
        assert tuple(int(x[0]) for x in got) == want


# ------------------------------------------------------------- what a describe line must say
def fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


def shared_lds(G, epb):
    """rollout_shared_kernel's arrays, before a closed-loop form's table"""
    c = G * G
    return c * 4 + 2 * epb * 4 + ((c + 15) & ~15) + ((2 * c + 15) & ~15)


def u8_lds(G, epb):
    c = G * G
    pw = (2 * c + 16 + 3) >> 2
    return (4 * pw * 4 + 2 * (epb + 1) * 4 + ((c + 1) & ~1) * 2 + c + 15) & ~15


def perenv_lds(G, epb):
    return 2 * epb * 4 + ((epb * G * G + 15) & ~15)


def grid_params(abi, variant, G, mode, hint=0):
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, G, mode, 100, -1.0, -0.01, 100.0)
    p.launch_hint = hint
    return p


# ------------------------------------------------------------- the envs of the GPU tests
@functools.lru_cache(maxsize=None)
def layouts(kind, G, N):
    if kind == "per_env":
        if N > 8192:                                        # a streaming batch: 4 099 mazes, tiled
            return np.ascontiguousarray(np.resize(bordered_random_layouts(4099, G, 300 + G), (N, G, G)))
        return bordered_random_layouts(N, G, 300 + G)
    return bordered_random_layouts(1, G, 300 + G)[0]


def make_env(kind, variant, G, N, seed=21, step_limit=7, env_base=ENV_BASE, epoch=EPOCH, hint=0):
    """kind: "shared", "u8" (shared, narrow planes) or "per_env".  Returns (env, its layouts)."""
    pkg = importlib.import_module("gym-lmaze_amd")
    lay = layouts(kind, G, N)
    kw = dict(variant=variant, seed=seed, step_limit=step_limit, env_base=env_base)
    if kind == "per_env":
        env = pkg.LmazeVecEnv(N, per_env_layouts=lay, **kw)
    else:
        env = pkg.LmazeVecEnv(N, layout=lay, obs_dtype="u8" if kind == "u8" else "int32", **kw)
    env._epoch = epoch
    env.params.launch_hint = hint
    # a spread of episode phases: some envs already done, some about to run into the step limit
    rs = np.random.RandomState(G + N)
    env.set_state(step_count=rs.randint(0, step_limit, N).astype(np.int32), done=(rs.rand(N) < 0.2).astype(np.uint8),
                  reward=np.where(rs.rand(N) < 0.5, -0.01, -1.0).astype(np.float32))
    return env, lay


def bare_grid_env(monkeypatch, variant="v0", u8=False, G=5, N=8):
    """An LmazeVecEnv that never saw a device, with only what the closed-loop methods' Python refusals read: no tuner, the
    variant and plane flags, G, N and the host as its device.  obs is there for the recording request alone, the last
    refusal: a call that gets as far as "obs_every must be ..." has had its table accepted.  torch's capture query needs a
    device; it is answered here, "no"."""
    pkg = importlib.import_module("gym-lmaze_amd")
    env = object.__new__(pkg.LmazeVecEnv)
    env._tuner, env._u8, env._is_v3, env.grid, env.num_envs = None, u8, variant == "v3", G, N
    env.device = torch.device("cpu")
    env.obs = torch.zeros((N, G, G), dtype=torch.uint8 if u8 else torch.int32)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return env


# ------------------------------------------------------------- one call against the oracle
def replay(env, lay, kind, T, auto_reset, k, key, rollout, action, window=None):
    """One closed-loop rollout of env against the oracle stepped T times from the env's host_state().
    rollout(obs_t) makes the call (trajectory=True, obs_every=k) and returns what it returned; action(key, t, env_global)
    is the policy restated: the int32 action of every env from its key, at step t (epoch0 + t is the draw's epoch).
    window = (first env, count): the oracle replays that contiguous range of the batch only (streaming sizes).
    Every step's key, action, reward bits and done, every recorded slot, the final state byte for byte and the final
    planes are compared.  Returns the oracle's sequences ([T, count]: key, act, sc, reward, done, and ball, the pre-step
    ball after the reset), the call's rows as numpy, its outputs, the final state and the number of resets."""
    N, G, v3 = env.num_envs, env.grid, env.variant == "v3"
    lo, cnt = window if window else (0, N)
    sl = slice(lo, lo + cnt)
    st = {name: np.array(v[sl], copy=True) for name, v in env.host_state().items()}
    p = O.params(O.VARIANT_V3 if v3 else O.VARIANT_V0, G, O.LAYOUT_PER_ENV if kind == "per_env" else O.LAYOUT_SHARED,
                 env.step_limit, *env.rewards)
    lay_c = np.ascontiguousarray(lay[sl] if kind == "per_env" else lay)
    epoch0 = env._epoch
    S = T // k if k else 0
    obs_t = torch.full((S, N, G, G), 113, dtype=env.obs.dtype, device=DEV) if k else None
    env.obs.fill_(113)
    out = rollout(obs_t)
    assert len(out) == 7 and env._epoch == epoch0 + T
    reward_t, done_t, actions_t, key_t = (np.ascontiguousarray(to_numpy(x[:, sl])) for x in out[3:])
    slots = np.ascontiguousarray(to_numpy(obs_t[:, sl])) if k else None
    obs_ref = np.zeros((cnt, G, G), np.int32)
    seq = {name: np.zeros((T, cnt), dt) for name, dt in (("key", np.int32), ("act", np.int32), ("sc", np.int32),
                                                         ("reward", np.float32), ("done", np.uint8))}
    seq["ball"] = np.zeros((T, cnt, 2), np.int32)
    eg = np.arange(cnt, dtype=np.uint64) + np.uint64(env.env_base + lo)
    n_reset = 0
    for t in range(T):
        if auto_reset and st["done"].any():                # reset(mask = done) with the library's draw rule
            n_reset += int(st["done"].sum())
            O.reset(p, lay_c, st["done"].copy(), env.seed, epoch0 + t, st["ball_xy"], st["goal_xy"], st["step_count"],
                    st["reward"], st["done"], env_base=env.env_base + lo)
        key_ref = st["ball_xy"][:, 0] * G + st["ball_xy"][:, 1]
        if key == "goal":
            key_ref = (st["goal_xy"][:, 0] * G + st["goal_xy"][:, 1]) * G * G + key_ref
        act = action(key_ref, t, eg)
        seq["key"][t], seq["act"][t], seq["ball"][t] = key_ref, act, st["ball_xy"]
        if v3:
            O.step_v3(p, lay_c, act, st["ball_xy"], st["goal_xy"], st["step_count"], st["reward"], st["done"], obs_ref)
        else:
            O.step_v0(p, lay_c, act, st["ball_xy"], st["step_count"], st["reward"], st["done"], st["goal_count"], obs_ref)
        seq["sc"][t], seq["reward"][t], seq["done"][t] = st["step_count"], st["reward"], st["done"]
        assert (key_t[t] == key_ref).all(), ("key", t)
        assert (actions_t[t] == act).all(), ("action", t)
        assert (f32_bits(reward_t[t]) == f32_bits(st["reward"])).all(), ("reward", t)
        assert (done_t[t].view(np.uint8) == st["done"]).all(), ("done", t)
        if k and (t + 1) % k == 0:
            assert (slots[(t + 1) // k - 1] == obs_ref.astype(slots.dtype)).all(), ("slot", t)
    if T:
        h = env.host_state()
        for name in h:
            assert (np.ascontiguousarray(h[name][sl]).view(np.uint8) == np.ascontiguousarray(st[name]).view(np.uint8)).all(), name
        got = to_numpy(env.obs[sl])
        assert (got == obs_ref.astype(got.dtype)).all(), "final planes"
    if k and T % k:                                        # the steps past the last slot store no planes
        assert slots.shape[0] == T // k
    return dict(seq=seq, rows=(reward_t, done_t, actions_t, key_t), out=out, final=st, resets=n_reset, env=env)
