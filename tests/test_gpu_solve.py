"""GPU: lmaze_solve against solve_ref.py (the model extracted from the C oracle, the float32 Jacobi sweep in numpy), bit for
bit on q, v, policy, sweeps_run and delta -- floats compared as uint32, every problem of every case -- on both kernel forms
(a wave per problem up to 16x16, a workgroup per problem above), with problem counts ragged against the packing, pockets
that never reach the goal (solves more than a thousand sweeps long beside solves of a dozen, in one launch) and sticky pairs;
and the loop closed through the existing kernels: the solved table, run by rollout_policy, reaches done from every cell in
exactly the BFS distance."""
import functools
import importlib

import numpy as np
import pytest
import torch

import helpers as H
import solve_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("q", "v", "policy", "sweeps_run", "delta")


@pytest.fixture(scope="module")
def lm():
    assert torch.cuda.is_available()
    return importlib.import_module("gym-lmaze_amd")


def dev():
    return torch.device("cuda", 0)


def same(got, ref, what=""):
    """Every output of got (SolvedTables, any leading shape) equals ref (solve_ref.Solved) bit for bit; prints the figures."""
    for f in FIELDS:
        g, r = getattr(got, f), np.asarray(getattr(ref, f))
        if g is None:
            continue
        g = g.cpu().numpy().reshape(r.shape)
        assert g.dtype == r.dtype, (what, f, g.dtype, r.dtype)
        gb, rb = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == np.float32 else (g, r)
        bad = int((gb != rb).sum())
        if f in ("sweeps_run", "delta"):
            print(what, f, "min", g.min(), "max", g.max())
        assert bad == 0, (what, f, bad, np.argwhere(gb != rb)[:5].tolist())


def shipped(lm, variant):
    lay = lm.layouts.to_codes(lm.VARIANTS[variant]["layout"])
    gx, gy = np.argwhere(lay == ord("X"))[0]
    return lay, (int(gx), int(gy))


@functools.lru_cache(maxsize=None)
def random_case(variant, N, G):
    lays = H.bordered_random_layouts(N, G, 7)
    goals = H.random_free_cells(lays, 3) if variant == "v3" else None
    return lays, goals


@functools.lru_cache(maxsize=None)
def _random_ref(variant, N, G, gamma, sweeps, reward_bytes):
    lays, goals = random_case(variant, N, G)
    return R.solve_many(variant, lays, goals, gamma, sweeps, tuple(float(r) for r in np.frombuffer(reward_bytes, np.float32)))


def random_ref(variant, N, G, gamma, sweeps, rewards=R.DEFAULT_REWARDS):
    """The reference of one random case, computed once (keyed by the rewards' bits: -0.0 == 0.0 would share an entry)."""
    return _random_ref(variant, N, G, gamma, sweeps, np.asarray(rewards, np.float32).tobytes())


def on_gpu(lays, goals):
    return torch.from_numpy(lays).to(dev()), None if goals is None else torch.from_numpy(goals).to(dev())


# ------------------------------------------------------------- shared layouts
@pytest.mark.parametrize("sweeps,expect", [(5, 5), (64, 18)])
def test_v0_shipped_layout_cut_off_and_early_stop(lm, sweeps, expect):
    lay, _ = shipped(lm, "v0")
    env = lm.LmazeVecEnv(3, variant="v0", device=dev())
    got = env.solve(gamma=0.99, sweeps=sweeps)
    assert tuple(got.q.shape) == (144, 4) and tuple(got.v.shape) == (144,) and got.policy.dtype == torch.uint8
    ref = R.solve(R.extract_model("v0", lay), 0.99, sweeps)
    same(got, ref, "v0 12x12 sweeps=%d" % sweeps)
    assert int(got.sweeps_run) == expect
    assert (float(got.delta) > 0.0) == (sweeps == 5)
    assert "solve_kernel<v0, wave, 4>" in lm._abi.describe_solve(env.params, 1)


def test_v3_every_goal_cell_long_solve_and_mixed_exit(lm):
    """All 324 problems of 324 cells (more cells than a workgroup has threads): goals nothing can reach run V down to
    -0.01 / (1 - gamma) over 1256 sweeps beside problems that settle within twenty, in one launch."""
    lay, _ = shipped(lm, "v3")
    G = 18
    env = lm.LmazeVecEnv(2, variant="v3", device=dev())
    got = env.solve(gamma=0.99, sweeps=1400, key="goal")
    assert tuple(got.q.shape) == (G ** 4, 4) and tuple(got.v.shape) == (G ** 4,) and tuple(got.policy.shape) == (G ** 4,)
    assert tuple(got.sweeps_run.shape) == (G * G,)
    goals = np.stack([np.arange(G * G) // G, np.arange(G * G) % G], 1).astype(np.int32)
    ref = R.solve_many("v3", lay, goals, 0.99, 1400)
    same(got, ref, "v3 18x18 every goal")
    run = got.sweeps_run.cpu().numpy()
    assert run.max() == 1256 and run.min() <= 14 and (run < 1400).all()
    assert "solve_kernel<v3, workgroup, 2>" in lm._abi.describe_solve(env.params, G * G)


# ------------------------------------------------------------- per-env layouts
@pytest.mark.parametrize("N,G", [(257, 5), (257, 8), (257, 11), (33, 32), (3, 64), (1, 11)])
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_per_env_random_mazes(lm, variant, N, G):
    lays, goals = random_case(variant, N, G)
    ref = random_ref(variant, N, G, 0.99, 1400)
    lay_d, goal_d = on_gpu(lays, goals)
    got = lm.solve_tables(lay_d, variant=variant, goals=goal_d, gamma=0.99, sweeps=1400)
    assert tuple(got.q.shape) == (N, G * G, 4)
    same(got, ref, "%s %d x %dx%d" % (variant, N, G, G))
    if N > 1:
        assert ref.sweeps_run.max() > 1000                             # a pocket: cells that cannot reach the goal
        if variant == "v0":
            assert np.isneginf(ref.q).any()                            # sticky pairs
    if N >= 33 and G <= 11:
        assert ref.sweeps_run.min() < 20                               # ... beside solves that settle at once


@pytest.mark.parametrize("N,G,form", [(9, 16, "wave, 4"), (9, 17, "workgroup, 2"), (5, 22, "workgroup, 2"), (5, 23, "workgroup, 4"),
                                      (5, 33, "workgroup, 8"), (5, 40, "workgroup, 8"), (3, 45, "workgroup, 8"), (3, 46, "workgroup, 16")])
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_every_kernel_form_at_the_edges_of_the_form_table(lm, variant, N, G, form):
    """Either side of every change of form (G = 16/17, 22/23, 32/33, 45/46), and the form "workgroup, 8 cells per lane"
    (G = 33..45), which no other case launches."""
    lays, goals = random_case(variant, N, G)
    ref = random_ref(variant, N, G, 0.99, 1400)
    lay_d, goal_d = on_gpu(lays, goals)
    got = lm.solve_tables(lay_d, variant=variant, goals=goal_d, gamma=0.99, sweeps=1400)
    assert tuple(got.q.shape) == (N, G * G, 4)
    same(got, ref, "%s %d x %dx%d" % (variant, N, G, G))
    p = lm._abi.make_params(lm._abi.VARIANT_V3 if variant == "v3" else lm._abi.VARIANT_V0, G, lm._abi.LAYOUT_PER_ENV, 100, *R.DEFAULT_REWARDS)
    assert "solve_kernel<%s, %s>" % (variant, form) in lm._abi.describe_solve(p, N)


def test_v3_goals_off_the_grid_and_on_wall_cells(lm):
    """"A goal off the grid is never hit" (include/lmaze.h), nor is one on a corner of the border: no terminal pair, V runs
    down to reward_move / (1 - gamma) over more than a thousand sweeps (-1 where a state can move, never above).  A goal on
    any other wall cell is compared as it is too -- the look-ahead pays for it from two cells away -- and the solve equals
    the reference there as everywhere."""
    N, G = 257, 8
    lays, goals = random_case("v3", N, G)
    goals, off = R.unreachable_goals(lays, goals)
    goals, walled = R.walled_goals(lays, goals, 5)
    ref = R.solve_many("v3", lays, goals, 0.99, 1400)
    lay_d, goal_d = on_gpu(lays, np.ascontiguousarray(goals))
    got = lm.solve_tables(lay_d, variant="v3", goals=goal_d, gamma=0.99, sweeps=1400)
    same(got, ref, "v3 goals off the grid and on walls")
    free = lays.reshape(N, -1) != ord("W")
    v = got.v.cpu().numpy()
    assert len(off) == 65 and (got.sweeps_run.cpu().numpy()[off] > 1000).all()
    assert (v[off][free[off]] <= np.float32(-0.99)).all()
    assert not np.isin(np.float32(100.0), got.q.cpu().numpy()[off])
    assert (got.q.cpu().numpy()[walled] == np.float32(100.0)).any()


@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_warm_start(lm, variant):
    lays, goals = random_case(variant, 257, 11)
    lay_d, goal_d = on_gpu(lays, goals)
    kw = dict(variant=variant, gamma=0.99)
    if variant == "v3":
        kw["goals"] = goal_d
    first = lm.solve_tables(lay_d, sweeps=7, **kw)
    second = lm.solve_tables(lay_d, sweeps=7, v_init=first.v, **kw)
    whole = lm.solve_tables(lay_d, sweeps=14, **kw)
    ref = random_ref(variant, 257, 11, 0.99, 14)
    same(whole, ref, "14 sweeps")
    for f in ("q", "v", "policy"):
        assert torch.equal(getattr(second, f).view(torch.uint8), getattr(whole, f).view(torch.uint8)), f
    unsettled = whole.sweeps_run > 8                                   # a problem still moving at the hand-over: the legs add up
    assert bool(unsettled.any()) and torch.equal((first.sweeps_run + second.sweeps_run)[unsettled], whole.sweeps_run[unsettled])
    ref2 = R.solve_many(variant, lays, goals, 0.99, 7, v_init=first.v.cpu().numpy())
    same(second, ref2, "7 more sweeps")


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("gamma", [0.0, 1.0])
def test_gamma_zero_and_one(lm, variant, gamma):
    """gamma = 1 and a pocket: every sweep lowers the pocket's values by reward_move, the solve never settles."""
    sweeps = 60
    lays, goals = random_case(variant, 257, 8)
    ref = random_ref(variant, 257, 8, gamma, sweeps)
    kw = dict(goals=on_gpu(lays, goals)[1]) if variant == "v3" else {}
    got = lm.solve_tables(on_gpu(lays, None)[0], variant=variant, gamma=gamma, sweeps=sweeps, **kw)
    same(got, ref, "%s gamma=%g" % (variant, gamma))
    run = got.sweeps_run.cpu().numpy()
    if gamma == 1.0:
        assert (run == sweeps).any() and (run < sweeps).any()
    else:
        assert (run == 2).all()                                        # the rewards themselves, then one unchanged sweep


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("rewards", [(100.0, -0.01, 100.0), (-1.0, 0.0, 0.0), (-1.0, -0.0, 0.0), (-0.0, 0.0, -0.0)])
def test_reward_edge_cases(lm, variant, rewards):
    """reward_wall == reward_goal makes a bump terminal; reward_move == reward_goal == 0 makes every move terminal and brings
    both zeros into the maximum, where a strict '>' keeps the first."""
    lays, goals = random_case(variant, 257, 8)
    ref = random_ref(variant, 257, 8, 0.99, 1400, rewards)
    kw = dict(goals=on_gpu(lays, goals)[1]) if variant == "v3" else {}
    got = lm.solve_tables(on_gpu(lays, None)[0], variant=variant, gamma=0.99, sweeps=1400, rewards=rewards, **kw)
    same(got, ref, "%s rewards=%r" % (variant, rewards))


@pytest.mark.parametrize("G", [11, 32])
@pytest.mark.parametrize("outputs", [("policy",), ("v",)])
def test_output_subsets(lm, outputs, G):
    N = 257 if G == 11 else 33
    lays, _ = random_case("v0", N, G)
    ref = random_ref("v0", N, G, 0.99, 1400)
    got = lm.solve_tables(on_gpu(lays, None)[0], variant="v0", gamma=0.99, sweeps=1400, outputs=outputs)
    for f in FIELDS:
        assert (getattr(got, f) is not None) == (f in outputs), f
    same(got, ref, "only %s" % (outputs,))


@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_env_solve_is_solve_tables_on_its_tensors(lm, variant):
    lays, _ = random_case(variant, 33, 32)
    env = lm.LmazeVecEnv(33, variant=variant, per_env_layouts=lays, device=dev(), seed=5)
    got = env.solve(gamma=0.99, sweeps=1400)
    want = lm.solve_tables(env.layout, variant=variant, goals=env.goal_xy if variant == "v3" else None, gamma=0.99, sweeps=1400)
    assert tuple(got.q.shape) == (33, 1024, 4)
    for f in FIELDS:
        assert torch.equal(getattr(got, f).view(torch.uint8), getattr(want, f).view(torch.uint8)), f
    ref = R.solve_many(variant, lays, env.goal_xy.cpu().numpy() if variant == "v3" else None, 0.99, 1400)
    same(got, ref, "env.solve %s" % variant)


def test_u8_env_and_refusals(lm):
    env = lm.LmazeVecEnv(4, variant="v0", device=dev(), obs_dtype="u8")
    plain = lm.LmazeVecEnv(4, variant="v0", device=dev())
    assert torch.equal(env.solve(sweeps=64).q.view(torch.int32), plain.solve(sweeps=64).q.view(torch.int32))
    with pytest.raises(ValueError, match="key must be 'ball' or 'goal'"):
        env.solve(key="cell")
    with pytest.raises(ValueError, match="key='goal' needs the v3 variant"):
        env.solve(key="goal")
    v3 = lm.LmazeVecEnv(4, variant="v3", device=dev())
    with pytest.raises(ValueError, match="needs goal="):
        v3.solve()
    with pytest.raises(ValueError):
        lm.solve_tables(plain.layout, variant="v0", sweeps=0)
    with pytest.raises(ValueError):
        lm.solve_tables(plain.layout, variant="v0", outputs=("delta",))
    with pytest.raises(ValueError):
        lm.solve_tables(plain.layout, variant="v3")
    open_border = plain.layout.clone()
    open_border[0, 3] = ord("B")
    with pytest.raises(ValueError, match="border"):
        lm.solve_tables(open_border, variant="v0")


# ------------------------------------------------------------- the loop closes through the existing kernels
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_solved_table_reaches_done_in_the_bfs_distance(lm, variant):
    """One env on every non-wall cell of the shipped layout (v3: the goal at 'X'), run by rollout_policy on the solved q
    with no exploration and no reset: every env's first done row is steps_to_done - 1 and carries reward_goal.  No env is
    left out: test_solve_cpu.py asserts that no non-wall cell is cut off."""
    lay, goal = shipped(lm, variant)
    G = lay.shape[0]
    model = R.extract_model(variant, lay, goal if variant == "v3" else None)
    dist = R.steps_to_done(model)
    cells = np.flatnonzero(~model.wall)
    assert np.isfinite(dist[cells]).all()
    n, T = len(cells), int(dist[cells].max())
    env = lm.LmazeVecEnv(n, variant=variant, device=dev(), seed=1)
    state = dict(ball_xy=np.stack([cells // G, cells % G], 1).astype(np.int32))
    if variant == "v3":
        state["goal_xy"] = np.tile(np.asarray(goal, np.int32), (n, 1))
    env.set_state(**state)
    solved = env.solve(gamma=0.99, sweeps=4096, goal=goal if variant == "v3" else None)
    assert int(solved.sweeps_run) < 100
    out = env.rollout_policy(T, q=solved.q, epsilon=0.0, auto_reset=False, trajectory=True)
    reward_t, done_t = out[3].cpu().numpy(), out[4].cpu().numpy().astype(bool)
    assert done_t.any(0).all()
    first = done_t.argmax(0)
    assert (first == dist[cells] - 1).all(), np.flatnonzero(first != dist[cells] - 1)[:8]
    assert (reward_t[first, np.arange(n)].view(np.uint32) == np.float32(env.rewards[2]).view(np.uint32)).all()
    assert T > 10
