"""GPU: lmaze_evaluate against evaluate_ref.py (the model extracted from the C oracle, the header's weight rule in numpy
integers, the float32 Jacobi sweep), every bit of q, v, sweeps_run and delta: every cells-per-lane instantiation of both kernel
forms, both variants, ragged problem counts, all three policy inputs; the cut-off and the tolerance stop; the shared-layout
problems of LmazeVecEnv.evaluate(); and the loop closed against solve() and score() on generated mazes."""
import functools
import importlib

import numpy as np
import pytest
import torch

import evaluate_ref as E
import helpers as H
import solve_ref as SR

pytestmark = pytest.mark.gpu

REWARDS = (-1.0, -0.01, 100.0)
# (problems, grid side): wave form 1 / 2 / 4 cells per lane, workgroup form 2 / 4 / 8 / 16; counts ragged against four problems
# per workgroup; one problem alone
SIZES = ((257, 5), (257, 11), (130, 16), (33, 18), (33, 32), (5, 40), (3, 64), (1, 11))
SWEEPS = 1400


@pytest.fixture(scope="module")
def lm():
    assert torch.cuda.is_available()
    return importlib.import_module("gym-lmaze_amd")


def dev():
    return torch.device("cuda", 0)


def up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def same(got, ref, what):
    """Every bit of got (EvaluatedTables, or a tuple in its order) equals ref (evaluate_ref.Evaluated, or another EvaluatedTables)"""
    for f, g, r in zip(("q", "v", "sweeps_run", "delta"), got, ref):
        if g is None:
            continue
        g, r = g.cpu().numpy(), (r.cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r))
        assert g.shape == r.shape and g.dtype == r.dtype, (what, f, g.shape, r.shape, g.dtype)
        gb, rb = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == np.float32 else (g, r)
        bad = gb != rb
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), g[bad][:5].tolist(), r[bad][:5].tolist())


@functools.lru_cache(maxsize=None)
def case(variant, N, G):
    """The mazes of one size, their goals (v3) and their models, built once"""
    lays = H.bordered_random_layouts(N, G, 7)
    goals = H.random_free_cells(lays, 5) if variant == "v3" else None
    return lays, goals, SR.models_of(variant, lays, goals, REWARDS)


def random_thresholds(rs, shape, wild=0.2):
    """uint32[..., 4]: sorted rows, a share of them left unsorted (non-monotone), word 3 noise"""
    c = rs.randint(0, 1 << 32, size=shape + (4,), dtype=np.uint64).astype(np.uint32)
    ordered = np.sort(c[..., :3], axis=-1)
    keep = rs.rand(*shape) < wild
    c[..., :3] = np.where(keep[..., None], c[..., :3], ordered)
    return c


def tables_for(P, S, seed):
    """The five tables of a case with the discount each is evaluated at: the epsilon-greedy ones settle within a few hundred
    sweeps at 0.9, the thresholds run for more than a thousand at 0.99"""
    rs = np.random.RandomState(seed)
    pol = rs.randint(0, 4, (P, S)).astype(np.uint8)
    pol[rs.rand(P, S) < 0.05] = rs.choice(np.array([4, 77, 255], np.uint8))
    q = rs.choice(np.array([-2.0, -0.0, 0.0, 0.25, 0.25, 1.0, np.nan, np.inf], np.float32), (P, S, 4)).astype(np.float32)
    q[:, ::5, 0] = np.nan
    q[:, 1::7] = 0.5
    return (("bytes e=0", 0.9, dict(policy=pol, epsilon_u32=0)),
            ("bytes e=2^28+3", 0.9, dict(policy=pol, epsilon_u32=(1 << 28) + 3)),
            ("bytes e=2^32-1", 0.9, dict(policy=pol, epsilon_u32=(1 << 32) - 1)),
            ("q", 0.9, dict(q=q, epsilon_u32=(1 << 28) + 3)),
            ("thresholds", 0.99, dict(thresholds=random_thresholds(rs, (P, S)))))


def call(lm, variant, lays, goals, gamma, sweeps=SWEEPS, tol=0.0, v_init=None, **table):
    """evaluate_tables with a table in the reference's terms (epsilon_u32 as the integer)"""
    e = table.pop("epsilon_u32", 0)
    return lm.evaluate_tables(up(lays), variant=variant, goals=up(goals), gamma=gamma, sweeps=sweeps, tol=tol, rewards=REWARDS,
                              v_init=up(v_init), epsilon=e / 4294967296.0, validate=False, **{k: up(v) for k, v in table.items()})


# ------------------------------------------------------------- per-env random mazes
@pytest.mark.parametrize("N,G", SIZES)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_per_env_random_mazes(lm, variant, N, G):
    S = G * G
    lays, goals, models = case(variant, N, G)
    wall = np.stack([m.wall for m in models])
    sticky = np.stack([m.sticky for m in models])
    early = cut = renorm = 0
    for kind, gamma, table in tables_for(N, S, 100 + G):
        assert lm._abi.epsilon_u32(table.get("epsilon_u32", 0) / 4294967296.0) == table.get("epsilon_u32", 0)
        v0 = np.random.RandomState(G).randn(N, S).astype(np.float32) if kind == "q" else None     # walls too
        ref = E.evaluate_many(variant, lays, goals, gamma, SWEEPS, rewards=REWARDS, v_init=v0, models=models, **table)
        got = call(lm, variant, lays, goals, gamma, v_init=v0, **table)
        assert tuple(got.q.shape) == (N, S, 4) and tuple(got.v.shape) == (N, S) and tuple(got.sweeps_run.shape) == (N,)
        same(got, ref, "%s N=%d G=%d %s" % (variant, N, G, kind))
        early += int((ref.sweeps_run < SWEEPS).sum())
        cut += int((ref.sweeps_run == SWEEPS).sum())
        renorm += int(E.renormalised(E.weights(**table), sticky, wall).sum())
    print(variant, N, G, "stopped early", early, "cut off", cut, "renormalised states", renorm)
    # the reference itself shows what the case is for: problems that stop on their own, and (v0) mass on sticky pairs
    assert early > 0
    if variant == "v0":
        assert sticky.any() and renorm > 0
    form, cpl = {5: ("wave", 1), 11: ("wave", 2), 16: ("wave", 4), 18: ("workgroup", 2), 32: ("workgroup", 4), 40: ("workgroup", 8),
                 64: ("workgroup", 16)}[G]
    p = lm._abi.make_params(lm.VARIANTS[variant]["id"], G, lm._abi.LAYOUT_PER_ENV, 100, *REWARDS)
    assert ("evaluate_kernel<%s, %s, %d>" % (variant, form, cpl)) in lm._abi.describe_evaluate(p, N)


# ------------------------------------------------------------- the other two stops
@pytest.mark.parametrize("G", [11, 18])
def test_cut_off_and_tolerance(lm, G):
    N = 33
    lays, goals, models = case("v0", N, G)
    table = tables_for(N, G * G, 100 + G)[1][2]
    ref = E.evaluate_many("v0", lays, None, 0.99, 5, rewards=REWARDS, models=models, **table)
    assert (ref.sweeps_run == 5).all() and (ref.delta > 0).all()           # cut off
    same(call(lm, "v0", lays, None, 0.99, sweeps=5, **table), ref, "cut off G=%d" % G)
    # a tolerance between two consecutive deltas of problem 0: it stops exactly at the later of the two sweeps
    deltas = []
    E.evaluate(models[0], 0.99, 60, deltas=deltas, **{k: (t if k == "epsilon_u32" else t[0]) for k, t in table.items()})
    k = next(i for i in range(10, 60) if 0 < deltas[i] < min(deltas[:i]))   # sweep k + 1 is the first to go this low
    tol = float(np.float32((np.float64(deltas[k - 1]) + np.float64(deltas[k])) / 2))
    assert deltas[k - 1] > np.float32(tol) >= deltas[k] and min(deltas[:k]) > np.float32(tol)
    ref = E.evaluate_many("v0", lays, None, 0.99, SWEEPS, tol=tol, rewards=REWARDS, models=models, **table)
    assert ref.sweeps_run[0] == k + 1 and (ref.sweeps_run < SWEEPS).all() and len(set(ref.sweeps_run.tolist())) > 1
    assert (ref.delta.view(np.uint32) <= np.float32(tol).view(np.uint32)).all()
    same(call(lm, "v0", lays, None, 0.99, tol=tol, **table), ref, "tol G=%d" % G)
    # a tolerance that is no tolerance: negative, NaN
    ref = E.evaluate_many("v0", lays, None, 0.9, SWEEPS, rewards=REWARDS, models=models, **table)
    for t in (-1.0, float("nan")):
        same(call(lm, "v0", lays, None, 0.9, tol=t, **table), ref, "tol=%r G=%d" % (t, G))


# ------------------------------------------------------------- venv.evaluate() on shared layouts
def test_env_evaluate_shared_ball(lm):
    env = lm.LmazeVecEnv(3, variant="v0", device=dev())
    G = env.grid
    S = G * G
    lay = lm.layouts.to_codes(lm.VARIANTS["v0"]["layout"])
    solved = env.solve()
    got = env.evaluate(policy=solved.policy, epsilon=0.1)
    assert tuple(got.q.shape) == (S, 4) and tuple(got.v.shape) == (S,) and got.sweeps_run.dim() == 0 and got.delta.dim() == 0
    e = lm._abi.epsilon_u32(0.1)
    ref = E.evaluate_many("v0", lay, None, 0.99, 4096, rewards=REWARDS, policy=solved.policy.cpu().numpy()[None], epsilon_u32=e)
    same([x[None] for x in got], ref, "shared ball")
    same([x[None] for x in env.evaluate(q=solved.q, epsilon=0.1)], ref, "shared ball q")
    warm = env.evaluate(q=solved.q, epsilon=0.1, v_init=got.v)             # [G*G] as it was returned
    assert int(warm.sweeps_run) == 1 and torch.equal(warm.v.view(torch.int32), got.v.view(torch.int32))
    v3 = lm.LmazeVecEnv(2, variant="v3", device=dev())
    with pytest.raises(ValueError, match="goal="):
        v3.evaluate(policy=torch.zeros(18 * 18, dtype=torch.uint8, device=dev()))
    lay3 = lm.layouts.to_codes(lm.VARIANTS["v3"]["layout"])
    gx, gy = (int(c) for c in np.argwhere(lay3 == ord("B"))[5])
    s3 = v3.solve(goal=(gx, gy))
    one = v3.evaluate(policy=s3.policy, epsilon=0.25, goal=(gx, gy), gamma=0.9)
    ref = E.evaluate_many("v3", lay3, np.array([[gx, gy]], np.int32), 0.9, 4096, rewards=REWARDS, policy=s3.policy.cpu().numpy()[None],
                          epsilon_u32=1 << 30)
    same([x[None] for x in one], ref, "shared ball v3")


def test_env_evaluate_key_goal(lm):
    """v3, the shipped 18 x 18 layout, all 324 goal cells, the policy solve(key="goal") plans for each, at epsilon = 0.1"""
    env = lm.LmazeVecEnv(2, variant="v3", device=dev())
    G = env.grid
    S = G * G
    lay = lm.layouts.to_codes(lm.VARIANTS["v3"]["layout"])
    solved = env.solve(gamma=0.9, sweeps=1400, key="goal")
    got = env.evaluate(policy=solved.policy, epsilon=0.1, key="goal", gamma=0.9, sweeps=SWEEPS)
    assert tuple(got.q.shape) == (G ** 4, 4) and tuple(got.v.shape) == (G ** 4,) and tuple(got.sweeps_run.shape) == (S,)
    assert tuple(got.delta.shape) == (S,)
    cells = np.arange(S)
    goals = np.stack([cells // G, cells % G], 1).astype(np.int32)
    ref = E.evaluate_many("v3", lay, goals, 0.9, SWEEPS, rewards=REWARDS, policy=solved.policy.cpu().numpy().reshape(S, S),
                          epsilon_u32=lm._abi.epsilon_u32(0.1))
    assert (ref.sweeps_run < SWEEPS).all() and len(set(ref.sweeps_run.tolist())) > 3
    same((got.q.reshape(S, S, 4), got.v.reshape(S, S), got.sweeps_run, got.delta), ref, "key=goal")


@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_env_evaluate_key_env_and_per_env(lm, variant):
    """key="env" on a shared layout: a population of N random tables on the one maze (v3: env i's current goal); per-env
    layouts: env i's maze"""
    N, G = 9, 11
    S = G * G
    lays = H.bordered_random_layouts(N, G, 31)
    rs = np.random.RandomState(4)
    pol = rs.randint(0, 4, (N, S)).astype(np.uint8)
    thr = random_thresholds(rs, (N, S))
    shared = lm.LmazeVecEnv(N, variant, layout=lays[0], device=dev(), seed=4)
    shared.reset()
    goals = shared.goal_xy.cpu().numpy() if variant == "v3" else None
    got = shared.evaluate(policy=up(pol), epsilon=0.5, key="env", gamma=0.9)
    assert tuple(got.q.shape) == (N, S, 4) and tuple(got.v.shape) == (N, S) and tuple(got.sweeps_run.shape) == (N,)
    same(got, E.evaluate_many(variant, lays[0], goals if goals is not None else [None] * N, 0.9, 4096, rewards=REWARDS, policy=pol,
                              epsilon_u32=1 << 31), "shared key=env")
    env = lm.LmazeVecEnv(N, variant, per_env_layouts=lays, device=dev(), seed=4)
    env.reset()
    goals = env.goal_xy.cpu().numpy() if variant == "v3" else None
    got = env.evaluate(thresholds=up(thr), gamma=0.9)
    same(got, E.evaluate_many(variant, lays, goals, 0.9, 4096, rewards=REWARDS, thresholds=thr), "per-env thresholds")
    same(env.evaluate(thresholds=up(thr).view(torch.int32).reshape(N * S, 4), gamma=0.9, key="env"), got, "flat int32 thresholds")


# ------------------------------------------------------------- the loop closed on generated mazes
@pytest.fixture(scope="module")
def generated(lm):
    return lm.layouts.mazes(64, 11, dev(), seed=7)


def test_planner_policy_is_worth_v_star(lm, generated):
    env = lm.LmazeVecEnv(64, "v0", per_env_layouts=generated, device=dev(), seed=3)
    solved = env.solve()
    assert bool((solved.sweeps_run < 4096).all())
    got = env.evaluate(policy=solved.policy, epsilon=0, v_init=solved.v)
    assert bool((got.sweeps_run == 1).all()) and bool((got.delta == 0).all())
    assert torch.equal(got.v.view(torch.int32), solved.v.view(torch.int32))
    assert torch.equal(got.q.view(torch.int32), solved.q.view(torch.int32))           # nothing is excluded here: no 'S'
    cold = env.evaluate(q=solved.q)                                                    # from zero, the table as q rows
    assert torch.equal(cold.v.view(torch.int32), solved.v.view(torch.int32))
    # the critic of the policy that explores lies below V*, and gae() takes it
    crit = env.evaluate(q=solved.q, epsilon=0.1)
    free = generated.flatten(1) != ord("W")
    assert bool((crit.v[free] < solved.v[free]).all())
    env.reset()
    out = env.rollout_policy(16, q=solved.q, epsilon=0.1, key="env", trajectory=True)
    reward_t, done_t, key_t = out[3], out[4], out[6]
    values = crit.v.reshape(-1)
    tail = env.state_keys("env")
    adv, tgt = lm.gae(reward_t, done_t, 0.99, 0.95, values=values, key_t=key_t, key_tail=tail)
    adv_b, tgt_b = lm.gae(reward_t, done_t, 0.99, 0.95, value_t=values[key_t.long()].contiguous(), tail=values[tail.long()].contiguous())
    assert torch.equal(adv.view(torch.int32), adv_b.view(torch.int32)) and torch.equal(tgt.view(torch.int32), tgt_b.view(torch.int32))


def test_values_are_walk_lengths(lm, generated):
    """Rewards (-2, -1, 0), gamma = 1, epsilon = 0: v = -(steps - 1) exactly wherever the table's walk arrives"""
    env = lm.LmazeVecEnv(64, "v0", per_env_layouts=generated, device=dev(), seed=3, rewards=(-2.0, -1.0, 0.0))
    pol = env.solve(gamma=0.99).policy
    steps = env.score(policy=pol).steps
    assert int(steps.max()) > 10
    got = env.evaluate(policy=pol, epsilon=0, gamma=1.0, sweeps=int(steps.max()) + 1)
    there = steps >= 1
    assert bool(there.any()) and bool((got.v[there] == -(steps[there] - 1).to(torch.float32)).all())
    assert bool((got.sweeps_run <= steps.max(dim=1).values + 1).all())
    # a random table: the walks that arrive still count their steps; the others are not looked at
    rnd = torch.randint(0, 4, pol.shape, dtype=torch.uint8, device=dev(), generator=torch.Generator(dev()).manual_seed(1))
    steps = env.score(policy=rnd).steps
    got = env.evaluate(policy=rnd, epsilon=0, gamma=1.0, sweeps=121)
    there = steps >= 1
    assert bool(there.any()) and bool((~there).any()) and bool((got.v[there] == -(steps[there] - 1).to(torch.float32)).all())


def test_probs_are_their_thresholds(lm, generated):
    env = lm.LmazeVecEnv(64, "v0", per_env_layouts=generated, device=dev(), seed=3)
    gen = torch.Generator(dev()).manual_seed(5)
    probs = torch.rand((64, 121, 4), device=dev(), generator=gen)
    probs[:, ::3] = torch.tensor([0.0, 1.0, 0.0, 0.0], device=dev())                  # one-hot rows
    thr = lm._abi.sampling_thresholds(probs.reshape(-1, 4)).view(64, 121, 4)
    a = env.evaluate(probs=probs, gamma=0.9)
    b = env.evaluate(thresholds=thr, gamma=0.9)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    logits = torch.randn((64, 121, 4), device=dev(), generator=gen)
    c = env.evaluate(logits=logits, temperature=0.5, gamma=0.9)
    d = env.evaluate(probs=torch.softmax(logits.double() / 0.5, -1), gamma=0.9)
    for x, y in zip(c, d):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ref = E.evaluate_many("v0", generated[:8].cpu().numpy(), None, 0.9, 4096, rewards=REWARDS, thresholds=thr[:8].cpu().numpy())
    same([x[:8] for x in a], ref, "probs")


# ------------------------------------------------------------- argument checks
def test_argument_checks(lm, generated):
    lay = generated[:4]
    S = 121
    pol = torch.zeros((4, S), dtype=torch.uint8, device=dev())
    q = torch.zeros((4, S, 4), device=dev())
    thr = torch.zeros((4, S, 4), dtype=torch.int32, device=dev())
    off16 = torch.zeros(4 * S * 4 + 4, dtype=torch.int32, device=dev())[1:-3].reshape(4, S, 4)     # contiguous, 4 bytes off
    assert off16.is_contiguous() and off16.data_ptr() % 16 == 4
    ok = lm.evaluate_tables(lay, policy=pol, outputs=("v",))
    assert ok.q is None and ok.sweeps_run is None and tuple(ok.v.shape) == (4, S)
    bad = [dict(), dict(policy=pol, q=q), dict(policy=pol, thresholds=thr), dict(probs=q, logits=q), dict(q=q, probs=q, thresholds=thr),
           dict(thresholds=thr, epsilon=0.1), dict(probs=q + 1, epsilon=0.5), dict(logits=q, epsilon=1.0),
           dict(logits=q, temperature=0.0), dict(policy=pol, epsilon=1.5), dict(policy=pol, epsilon=-0.1),
           dict(policy=pol[:3]), dict(policy=pol.reshape(-1)), dict(policy=pol.to(torch.int32)), dict(policy=pol.cpu()),
           dict(q=q[:, :, :3]), dict(q=q.double()), dict(q=q.cpu()), dict(q=q.transpose(0, 1)), dict(thresholds=thr.float()),
           dict(thresholds=thr[:, :100]), dict(thresholds=thr.cpu()), dict(thresholds=off16),
           dict(probs=q.reshape(-1, 4) + 1), dict(policy=pol, sweeps=0), dict(policy=pol, sweeps=2.5), dict(policy=pol, outputs=("delta",)),
           dict(policy=pol, outputs=("v", "policy")), dict(policy=pol, v_init=torch.zeros(4, S)), dict(policy=pol, v_init=q[:, :, 0]),
           dict(policy=pol, goals=torch.zeros((4, 2), dtype=torch.int32, device=dev())), dict(policy=pol, variant="v1"),
           dict(policy=pol, rewards=(1.0, 2.0))]
    for kw in bad:
        with pytest.raises(ValueError):
            lm.evaluate_tables(lay, **kw)
    with pytest.raises(ValueError):
        lm.evaluate_tables(lay.cpu(), policy=pol)
    with pytest.raises(ValueError):
        lm.evaluate_tables(lay, variant="v3", policy=pol)                              # v3 needs goals
    env = lm.LmazeVecEnv(4, "v0", per_env_layouts=lay, device=dev())
    for kw in (dict(), dict(policy=pol, q=q), dict(thresholds=thr, epsilon=0.2), dict(policy=pol, key="goal"), dict(policy=pol, key="cell"),
               dict(policy=pol[:2]), dict(policy=pol, goal=(1, 1)), dict(q=q[:, :, :2])):
        with pytest.raises(ValueError):
            env.evaluate(**kw)
    shared = lm.LmazeVecEnv(4, "v0", device=dev())
    with pytest.raises(ValueError, match="v3"):
        shared.evaluate(policy=torch.zeros(144, dtype=torch.uint8, device=dev()), key="goal")
    v3 = lm.LmazeVecEnv(4, "v3", per_env_layouts=lay, device=dev())
    with pytest.raises(ValueError):
        v3.evaluate(policy=pol, key="goal")                                            # per-env layouts keep their own goals
