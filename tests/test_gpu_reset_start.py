"""GPU: LmazeVecEnv.reset(start=, thresholds=) / lmaze_reset_start against reset_start_ref.py, exact integers on ball_xy,
goal_xy, step_count, the reward's bits, done and the planes (the planes against observe() of the reference state): every row
mode on shared and per-env layouts, v0 and v3, kept and re-drawn goals, masks, env_base, two epochs; rows built from the
envs' own draws around every compare; the v3 goals tied to lmaze_reset's; sharding; the curriculum end to end on generated
mazes; occupancy(start=law) as the prediction; the describe lines."""
import importlib

import numpy as np
import pytest
import torch

import reset_start_ref as RS
from closed_loop_ref import ENV_BASE, EPOCH, fields
from helpers import bordered_random_layouts, f32_bits

pytestmark = pytest.mark.gpu

ONE = RS.ONE
SHAPES = [(G, N) for G in (5, 11, 12, 18, 64) for N in (1, 63, 65, 257, 1000) if G < 64 or N <= 65]
ROW_MODE = {"ball": 0, "env": 1, "goal": 2}


@pytest.fixture(scope="module")
def lm():
    assert torch.cuda.is_available()
    return importlib.import_module("gym-lmaze_amd")


def dev():
    return torch.device("cuda", 0)


def up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def words(t):
    return t.view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def as_u32(w):
    """int64 words -> the uint32 table on the device"""
    w = np.asarray(w, np.int64)
    return up(np.where(w >= ONE, w - (1 << 32), w).astype(np.int32)).view(torch.uint32)


def layouts_of(kind, G, N):
    return bordered_random_layouts(N, G, 500 + G) if kind == "per_env" else bordered_random_layouts(1, G, 500 + G)[0]


def make(lm, variant, kind, G, N, env_base=0, epoch=0, u8=False, seed=21, lay=None):
    lay = layouts_of(kind, G, N) if lay is None else lay
    kw = dict(variant=variant, seed=seed, env_base=env_base, device=dev())
    if kind == "per_env":
        env = lm.LmazeVecEnv(N, per_env_layouts=lay, **kw)
    else:
        env = lm.LmazeVecEnv(N, layout=lay, obs_dtype="u8" if u8 else "int32", **kw)
    env._epoch = epoch
    return env, lay


def load(env, seed):
    """a spread of counters, rewards and done flags, which a reset must zero where its mask says so and nowhere else"""
    rs = np.random.RandomState(seed)
    N = env.num_envs
    env.set_state(step_count=rs.randint(0, 90, N).astype(np.int32), done=(rs.rand(N) < 0.3).astype(np.uint8),
                  reward=rs.choice(np.array([-0.01, -1.0, 100.0], np.float32), N))


def random_table(lm, rows, S, seed):
    """uint32[rows, S] of random laws: mass on a random third of ALL cells (walls among them: a cell is not excluded), a row in
    eight without any mass"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.rand((rows, S), generator=g) * (torch.rand((rows, S), generator=g) < 0.34)
    w[3::8] = 0
    return lm.start_thresholds(w.to(dev()))


def masks(N, seed):
    return {"none": None, "zero": np.zeros(N, np.uint8), "half": (np.random.RandomState(seed).rand(N) < 0.5).astype(np.uint8) * 3}


def check_call(env, twin, lay, thr, key, keep_goal, mask, what, thr_words=None, **how):
    """One reset(thresholds= or start=) of env against the reference from env's own state; twin: an env of the same shape whose
    observe() renders the reference state.  Returns (k, u) of the reference."""
    N, G = env.num_envs, env.grid
    st = {name: np.array(v, copy=True) for name, v in env.host_state().items()}
    before = env.obs.clone()
    epoch0 = env._epoch
    obs = env.reset(mask=None if mask is None else up(mask), key=key, keep_goal=keep_goal, **(how or {"thresholds": thr}))
    assert obs is env.obs and env._epoch == epoch0 + 1
    k, u = RS.reset_start(env.variant, lay, words(thr) if thr_words is None else thr_words, ROW_MODE[key], keep_goal, env.seed,
                          epoch0, env.env_base, st, mask)
    got = env.host_state()
    for name in got:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(st[name])
        bad = (a.view(np.uint8) != b.view(np.uint8)).reshape(N, -1).any(1)
        assert not bad.any(), (what, name, int(bad.sum()), np.flatnonzero(bad)[:5].tolist(), a[bad][:3].tolist(), b[bad][:3].tolist())
    on = np.ones(N, bool) if mask is None else mask != 0
    assert (f32_bits(got["reward"])[on] == 0x80000000).all()                 # -0.0
    twin.set_state(ball_xy=st["ball_xy"], **({"goal_xy": st["goal_xy"]} if env.variant == "v3" else {}))
    twin.observe()
    assert (env.obs == twin.obs).all(), (what, "planes")
    assert (env.obs[up(~on)] == before[up(~on)]).all(), (what, "planes outside the mask")
    return k, u


@pytest.mark.parametrize("G,N", SHAPES)
def test_every_form_against_the_reference(lm, G, N):
    S = G * G
    n = 0
    for variant in ("v0", "v3"):
        for kind in ("shared", "per_env"):
            keys = ("ball", "env") + (("goal",) if variant == "v3" and kind == "shared" else ())
            for key in keys:
                n += 1
                base, epoch = ((ENV_BASE, EPOCH) if n % 2 else (0, 0))
                env, lay = make(lm, variant, kind, G, N, base, epoch)
                twin, _ = make(lm, variant, kind, G, N, base, epoch, lay=lay)
                load(env, n)
                thr = random_table(lm, {"ball": 1, "env": N, "goal": S}[key], S, 7 * n + G)
                tw = words(thr)
                m = masks(N, n + N)
                order = [("none", "half", "zero"), ("half", "zero", "none"), ("zero", "none", "half")][n % 3]
                for c, mk in enumerate(order):                               # three epochs: the masks in turn, both goal modes
                    keep = variant == "v3" and (n + c) % 2 == 1
                    goals = env.goal_xy.clone()
                    k, _ = check_call(env, twin, lay, thr, key, keep, m[mk], (variant, kind, key, keep, mk, G, N), thr_words=tw)
                    if variant == "v3" and not keep and mk == "none":        # the goals are lmaze_reset's own, bit for bit
                        other, _ = make(lm, variant, kind, G, N, base, env._epoch - 1, lay=lay)
                        other.reset()
                        assert (other.goal_xy == env.goal_xy).all()
                    if keep:
                        assert (env.goal_xy == goals).all()
                    if mk == "none" and key != "goal":
                        assert (k == S).any() == (key == "env" and N > 3)    # rows without mass: those balls stayed
    # start=: the law itself, through start_thresholds()
    env, lay = make(lm, "v0", "shared", G, N)
    twin, _ = make(lm, "v0", "shared", G, N, lay=lay)
    law = lm.reset_distribution(env.layout, "v0")
    k, _ = check_call(env, twin, lay, lm.start_thresholds(law), "ball", False, None, ("start=", G, N), start=law)
    assert (law.reshape(-1).cpu().numpy()[k] > 0).all()


def test_the_narrow_planes(lm):
    G, N = 11, 257
    for variant in ("v0", "v3"):
        env, lay = make(lm, variant, "shared", G, N, ENV_BASE, EPOCH, u8=True)
        twin, _ = make(lm, variant, "shared", G, N, ENV_BASE, EPOCH, u8=True, lay=lay)
        assert env.obs.dtype == torch.uint8
        load(env, 5)
        for key in ("ball", "env") + (("goal",) if variant == "v3" else ()):
            thr = random_table(lm, {"ball": 1, "env": N, "goal": G * G}[key], G * G, 90)
            for mk, mask in masks(N, 4).items():
                check_call(env, twin, lay, thr, key, variant == "v3" and mk == "half", mask, ("u8", variant, key, mk))


# ------------------------------------------------------------- rows built from the envs' own draws
@pytest.mark.parametrize("kind", ["shared", "per_env"])
def test_rows_around_every_compare(lm, kind):
    """key="env" rows made from each env's u_i, the expected k in brackets: row[j] == u_i [j + 1], row[j] == u_i + 1 [j], mass
    on the first and on the last interior cell alone, no mass [the ball stays, the counters are zeroed], 2^31 everywhere [cell
    0], and the ends of the draw's range forced through rows of 0, of 2^31 - 1 and of 2^31."""
    G, N = 11, 1000
    S = G * G
    env, lay = make(lm, "v0", kind, G, N, ENV_BASE, EPOCH)
    twin, _ = make(lm, "v0", kind, G, N, ENV_BASE, EPOCH, lay=lay)
    load(env, 8)
    u = RS.ball_draw(env.seed, EPOCH, np.arange(N, dtype=np.uint64) + np.uint64(ENV_BASE))
    rows = np.zeros((N, S), np.int64)
    want = np.zeros(N, np.int64)
    first, last = G + 1, (G - 2) * G + G - 2
    for i in range(N):
        j, form = (i // 8) % (S - 1), i % 8
        if form in (0, 1):                                                  # zeros below j, 2^31 above it
            rows[i, j] = u[i] + form
            rows[i, j + 1:] = ONE
            want[i] = j + 1 - form
        elif form in (2, 3):
            c = first if form == 2 else last
            rows[i, c:] = ONE
            want[i] = c
        elif form == 4:
            want[i] = S
        elif form == 5:
            rows[i] = ONE
        elif form == 6:                                                     # words of 2^31 - 1 count for the largest draw alone
            rows[i] = ONE - 1
            rows[i, -1] = ONE
            want[i] = S - 1 if u[i] == ONE - 1 else 0
        else:                                                               # words of 0 count for every draw, u = 0 too
            rows[i, j + 1:] = ONE
            want[i] = j + 1
    ball0 = env.ball_xy.clone()
    k, _ = check_call(env, twin, lay, as_u32(rows), "env", False, None, ("edges", kind))
    assert (k == want).all()
    got = env.ball_xy.cpu().numpy().astype(np.int64)
    moved = want < S
    assert (got[moved, 0] * G + got[moved, 1] == want[moved]).all()
    assert (env.ball_xy[up(~moved)] == ball0[up(~moved)]).all() and not env.step_count.any() and not env.done.any()
    # the one-row and the goal-row forms search: the same compares around env 0's draw
    for variant, key in (("v0", "ball"), ("v3", "ball"), ("v3", "goal")):
        if kind == "per_env" and key == "goal":
            continue
        env, lay = make(lm, variant, kind, G, 65, ENV_BASE, EPOCH)
        twin, _ = make(lm, variant, kind, G, 65, ENV_BASE, EPOCH, lay=lay)
        for c, (j, plus) in enumerate(((0, 0), (0, 1), (59, 0), (59, 1), (S - 2, 0), (S - 2, 1))):
            u0 = int(RS.ball_draw(env.seed, env._epoch, np.array([ENV_BASE], np.uint64))[0])
            row = np.zeros(S, np.int64)
            row[j] = u0 + plus
            row[j + 1:] = ONE
            table = np.tile(row, (S if key == "goal" else 1, 1))
            k, _ = check_call(env, twin, lay, as_u32(table), key, False, None, ("edges", kind, variant, key, j, plus))
            assert k[0] == j + 1 - plus
        for word, cell in ((0, S), (ONE, 0), (ONE - 1, None)):                # constant rows (the table is not validated)
            table = np.full((S if key == "goal" else 1, S), word, np.int64)
            k, u = check_call(env, twin, lay, as_u32(table), key, False, None, ("constant row", word), thresholds=as_u32(table),
                              validate=False)
            assert (k == (cell if cell is not None else np.where(u == ONE - 1, S, 0))).all()


# ------------------------------------------------------------- sharding
@pytest.mark.parametrize("variant,kind,key", [("v3", "shared", "ball"), ("v3", "shared", "goal"), ("v0", "per_env", "env"),
                                              ("v3", "per_env", "env")])
def test_two_shards_reproduce_one_batch(lm, variant, kind, key):
    G, N = 11, 514
    S, h = G * G, N // 2
    lay = layouts_of(kind, G, N)
    thr = random_table(lm, {"ball": 1, "env": N, "goal": S}[key], S, 33)
    whole, _ = make(lm, variant, kind, G, N, 0, EPOCH, lay=lay)
    whole.reset(thresholds=thr, key=key)
    parts = []
    for lo in (0, h):
        part, _ = make(lm, variant, kind, G, h, lo, EPOCH, lay=lay[lo:lo + h] if kind == "per_env" else lay)
        part.reset(thresholds=thr[lo:lo + h].contiguous() if key == "env" else thr, key=key)
        parts.append(part)
    for name in ("ball_xy", "goal_xy", "step_count", "reward", "done"):
        assert (torch.cat([getattr(p, name) for p in parts]) == getattr(whole, name)).all(), name
    assert (torch.cat([p.obs for p in parts]) == whole.obs).all()


# ------------------------------------------------------------- the curriculum, end to end
def first_done(done_t):
    """int64[N]: the 1-based step at which done_t[:, i] is first set, 0 if never"""
    d = done_t.cpu().numpy()
    return np.where(d.any(0), d.argmax(0) + 1, 0)


def test_the_curriculum_end_to_end(lm):
    """mazes -> solve -> score -> distance_band -> reset(start=, key="env") -> rollout_policy(auto_reset=False) -> reset(mask=done,
    start=next band): every env is done after exactly optimal[start cell] steps, inside its band.  No maze of this seed has an
    empty 3..6 band (test_reset_start_cpu.py: a connected maze holds every distance up to its largest, 10 at the least here), so
    the fallback is reached in the second stage, whose bounds are per maze and out of reach for every 16th."""
    N, G = 257, 11
    S = G * G
    lays = lm.layouts.mazes(N, G, dev(), seed=7)
    env = lm.LmazeVecEnv(N, variant="v0", per_env_layouts=lays, device=dev(), seed=5)
    solved = env.solve()
    scored = env.score(policy=solved.policy)
    opt = scored.optimal.cpu().numpy()
    support = lm.reset_distribution(lays, "v0").cpu().numpy() > 0
    env_i = np.arange(N)

    law = lm.distance_band(scored.optimal, 3, 6, lays, "v0")
    env.reset(start=law, key="env")
    cell = env.state_keys("ball").cpu().numpy()
    assert (law.cpu().numpy()[env_i, cell] > 0).all()
    out = env.rollout_policy(6, q=solved.q, key="env", epsilon=0, auto_reset=False, trajectory=True)
    steps = first_done(out[4])
    assert (steps > 0).all(), "an env is left undone"
    assert (steps == opt[env_i, cell]).all() and (steps >= 3).all() and (steps <= 6).all()

    lo = torch.full((N,), 5, dtype=torch.int32, device=dev())
    hi = torch.full((N,), 9, dtype=torch.int32, device=dev())
    lo[::16] = hi[::16] = 1000                                               # no cell is that far: reset()'s own law
    fallback = np.zeros(N, bool)
    fallback[::16] = True
    law2 = lm.distance_band(scored.optimal, lo, hi, lays, "v0")
    assert (law2[up(fallback)] == lm.reset_distribution(lays, "v0")[up(fallback)]).all()
    env.reset(mask=out[4].any(0), start=law2, key="env")          # every env that was done at some step: all of them
    assert not env.done.any() and not env.step_count.any()
    cell = env.state_keys("ball").cpu().numpy()
    d0 = opt[env_i, cell]
    assert support[env_i, cell].all() and (d0 >= 1).all()
    assert ((d0 >= 5) & (d0 <= 9))[~fallback].all()
    T = int(d0.max())
    assert T <= 60
    out = env.rollout_policy(T, q=solved.q, key="env", epsilon=0, auto_reset=False, trajectory=True)
    steps = first_done(out[4])
    assert (steps > 0).all(), "an env is left undone"
    assert (steps == d0).all()


# ------------------------------------------------------------- occupancy(start=law) predicts what the envs do
def test_occupancy_takes_the_law_and_the_envs_follow_it(lm):
    G, N = 11, 4096
    S = G * G
    env, lay = make(lm, "v0", "shared", G, N, ENV_BASE, EPOCH)
    solved = env.solve()
    scored = env.score(policy=solved.policy)
    law = lm.distance_band(scored.optimal.reshape(1, S), 2, 5, env.layout, "v0")
    assert int((law > 0).sum()) >= 2
    d = env.occupancy(policy=solved.policy, start=law, sweeps=1).d
    assert (d.reshape(-1).view(torch.int32) == law.reshape(-1).view(torch.int32)).all()
    env.reset(start=law)
    thr = words(lm.start_thresholds(law))[0]
    k = RS.count_below(thr, RS.ball_draw(env.seed, EPOCH, np.arange(N, dtype=np.uint64) + np.uint64(ENV_BASE)))
    hist = np.bincount(env.state_keys("ball").cpu().numpy(), minlength=S)
    assert (hist == np.bincount(k, minlength=S)).all() and (hist[RS.row_law(thr) == 0] == 0).all()


# ------------------------------------------------------------- what would be queued
def test_describe_names_the_kernel_of_every_rows_form(lm):
    abi = lm._abi
    G, N = 11, 1000
    row, spawn = (G * G * 4 + 15) & ~15, (G * G * 2 + 15) & ~15

    def line(variant, mode, key):
        p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, G, mode, 100, -1.0, -0.01, 100.0)
        return abi.describe_reset_start(p, N, key)

    for variant, mode, key, name, lds, grid in (
            ("v0", 0, "ball", "reset_start_kernel<v0, rows=one, table=lds>", row, 4),
            ("v3", 0, "ball", "reset_start_kernel<v3, rows=one, table=lds>", row + spawn, 4),
            ("v3", 0, "goal", "reset_start_kernel<v3, rows=goal, table=global>", spawn, 4),
            ("v0", 0, "env", "reset_start_kernel<v0, rows=env, table=global>", 0, 250),
            ("v3", 1, "env", "reset_start_kernel<v3, rows=env, table=global>", 0, 250),
            ("v0", 1, "ball", "reset_start_kernel<v0, rows=one, table=global>", 0, 250)):
        text = line(variant, mode, key)
        f = fields(text)
        assert text.startswith(name + " "), text
        assert f["lds"] == lds and f["grid"] == grid and f["block"] == 256, text
        assert f["envs_per_workgroup"] == (256 if grid == 4 else 4), text
    p = abi.make_params(abi.VARIANT_V3, 64, 0, 100, -1.0, -0.01, 100.0)
    assert fields(abi.describe_reset_start(p, 65, "ball"))["lds"] == 16384 + 8192
    assert abi.describe_reset_start(p, 0, "goal") == ""
