"""GPU: lmaze_score against score_ref.py (the model extracted from the C oracle, a BFS, a plain vectorised walk), every integer
of optimal, steps and summary, at every plan step of both kernel forms, both variants, shared and per-env layouts, with the
planner's tables, random tables (cycles everywhere), bytes above 3 and q rows with ties, NaN and infinities; corridors deep
enough for the last doubling round and hundreds of sweeps; guard words, omitted outputs, ragged problem counts; and the
pipeline closed: generated mazes, solved, scored -- every free cell arrives in the fewest steps."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import helpers as H
import maze_ref as M
import qlearn_ref as Q
import score_ref as SC
import solve_ref as SR

pytestmark = pytest.mark.gpu

PLAN_STEPS = (3, 5, 8, 9, 11, 12, 16, 17, 23, 32, 33, 46, 64)
P7 = 7                                 # problems unless stated: the wave form's last workgroup is ragged


@pytest.fixture(scope="module")
def lm():
    assert torch.cuda.is_available()
    return importlib.import_module("gym-lmaze_amd")


def dev():
    return torch.device("cuda", 0)


def up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def same(got, ref, what):
    """Every integer of got (ScoredTables) equals ref (score_ref.Scored); an output neither has is skipped"""
    for f in ("optimal", "steps", "summary"):
        g, r = getattr(got, f), getattr(ref, f)
        if g is None:
            continue
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and r is not None and g.shape == r.shape, (what, f, g.shape)
        bad = g != r
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), g[bad][:5].tolist(), r[bad][:5].tolist())


def nasty_q(P, S, seed):
    """float32[P,S,4]: few distinct values, so ties are everywhere; NaN in word 0 and elsewhere, both infinities, -0.0"""
    rs = np.random.RandomState(seed)
    vals = np.array([-2.0, -0.0, 0.0, 0.25, 0.25, 1.0, np.nan, np.inf, -np.inf], np.float32)
    q = rs.choice(vals, (P, S, 4)).astype(np.float32)
    q[:, ::5, 0] = np.nan
    q[:, 1::7] = 0.5                                                       # a row of four equal words: action 0
    return q


def tables_for(lm, variant, lays, goals, P, S, seed):
    """The four kinds of table of one case: the planner's policy, random bytes, random bytes with some above 3, q rows"""
    rs = np.random.RandomState(seed)
    solved = lm.solve_tables(up(lays), variant=variant, goals=up(goals), gamma=0.99, outputs=("policy",), validate=False).policy
    solved = solved.cpu().numpy()
    if solved.shape[0] != P:                                               # v0 on one shared maze: one problem solved
        solved = np.repeat(solved, P, axis=0)
    rand = rs.randint(0, 4, (P, S)).astype(np.uint8)
    wild = rand.copy()
    wild[rs.rand(P, S) < 0.08] = 255
    wild[rs.rand(P, S) < 0.04] = 4
    return (("solved", dict(policy=solved)), ("random", dict(policy=rand)), ("above3", dict(policy=wild)),
            ("q", dict(q=nasty_q(P, S, seed + 1))))


def run_case(lm, variant, lays, goals, P, what, seed=5, kinds=None):
    """score_tables on every kind of table of the case against score_many; returns the summaries by kind"""
    G = lays.shape[-1]
    S = G * G
    out = {}
    for kind, tab in tables_for(lm, variant, lays, goals, P, S, seed):
        if kinds is not None and kind not in kinds:
            continue
        ref = SC.score_many(variant, lays, goals, problems=P, **tab)
        got = lm.score_tables(up(lays), variant=variant, goals=up(goals), validate=False, **{k: up(v) for k, v in tab.items()})
        assert tuple(got.optimal.shape) == (P, S) and tuple(got.steps.shape) == (P, S) and tuple(got.summary.shape) == (P, 4)
        same(got, ref, "%s %s %s" % (what, variant, kind))
        out[kind] = ref.summary
    return out


def mazes_np(G, P, seed, loops_u32):
    """P mazes of side G on the host: the generator's own specification (maze_ref: the bytes layouts.mazes() writes) from
    G = 5 on; at G = 3 the one layout there is"""
    if G == 3:                                                             # one free cell: every action bumps
        lay = np.full((P, 3, 3), ord("W"), np.uint8)
        lay[:, 1, 1] = ord("B")
        return lay
    return M.generate(G, P, seed, 0, loops_u32)[0]


# ------------------------------------------------------------- every plan step
@pytest.mark.parametrize("G", PLAN_STEPS)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_per_env_every_plan_step(lm, variant, G):
    lays = mazes_np(G, P7, 20 + G, (1 << 30) if G % 2 else 0)              # loops 0.25 at odd G, perfect mazes at even G
    goals = H.random_free_cells(lays, 3) if variant == "v3" else None
    sums = run_case(lm, variant, lays, goals, P7, "per-env G=%d" % G)
    free = (lays != ord("W")).reshape(P7, -1).sum(1)
    if G >= 5 and variant == "v0":                                         # connected, no 'S': the planner arrives from everywhere
        assert (sums["solved"] == np.stack([free, free, free, 0 * free], 1)).all()
    if G >= 8 and variant == "v0":
        assert (sums["random"][:, 1] < sums["random"][:, 0]).all()         # random tables lose walks to cycles
    form = "wave" if G * G <= 256 else "workgroup"
    p = lm._abi.make_params(lm.VARIANTS[variant]["id"], G, lm._abi.LAYOUT_PER_ENV, 100, -1.0, -0.01, 100.0)
    assert ("score_kernel<%s, %s," % (variant, form)) in lm._abi.describe_score(p, P7)


@pytest.mark.parametrize("G", PLAN_STEPS)
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_shared_every_plan_step(lm, variant, G):
    """One maze, seven tables (v0: a population on the one maze; v3: a goal per problem)"""
    lay = mazes_np(G, 1, 40 + G, 0 if G % 2 else (1 << 30))[0]
    goals = None
    if variant == "v3":
        goals = H.random_free_cells(np.repeat(lay[None], P7, axis=0), 9)
    run_case(lm, variant, lay, goals, P7, "shared G=%d" % G)


# ------------------------------------------------------------- layouts
@pytest.mark.parametrize("G", [11, 23])
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_disconnected_sticky_and_odd_goals(lm, variant, G):
    """random_walled's mazes (pockets: -1 regions) and bordered random ones with an 'S' cell (v0's excluded pairs); v3 with
    goals nothing can pay for and goals on wall cells"""
    P = 12
    walled = lm.layouts.random_walled(P, G, dev(), seed=7 + G).cpu().numpy()
    sticky = H.bordered_random_layouts(P, G, 3 + G)
    for name, lays in (("random_walled", walled), ("with S", sticky)):
        goals = None
        if variant == "v3":
            goals = H.random_free_cells(lays, 5)
            goals, _ = SR.unreachable_goals(lays, goals)
            goals, _ = SR.walled_goals(lays, goals, 8)
        sums = run_case(lm, variant, lays, goals, P, "%s G=%d" % (name, G))
        free = (lays != ord("W")).reshape(P, -1).sum(1)
        assert (sums["solved"][:, 0] < free).any()                         # cells that cannot reach done
        if variant == "v3":
            assert (sums["solved"][::4, 0] == 0).all()                     # the unreachable goals: nothing arrives anywhere
    if variant == "v0":
        m = [SR.extract_model("v0", lay) for lay in sticky]
        assert any(x.sticky.any() for x in m)


# ------------------------------------------------------------- depth
@functools.lru_cache(maxsize=None)
def corridor(G):
    lay, path = SC.serpentine(G)
    model = SR.extract_model("v0", lay)
    return lay, path, model, SC.optimal(model)


@pytest.mark.parametrize("G", [17, 64])
def test_serpentine_corridor(lm, G):
    """One path through every free cell, 'X' at its end: distances beyond S / 4 (hundreds of sweeps at G = 64) and walks
    that need the last doubling rounds; the corridor's policy, and the same with one cell reversed, at seven places"""
    S = G * G
    lay, path, model, opt = corridor(G)
    assert opt.max() > S // 4 and opt.max() == len(path) - 1
    assert SC.doubling(model, SC.actions_of(policy=SC.corridor_policy(G, path)))[1] >= SC.log2_ceil(opt.max())
    pol = np.repeat(SC.corridor_policy(G, path)[None], P7, axis=0)
    for p in range(1, P7):
        x, y = path[(len(path) * p) // P7]
        pol[p, x * G + y] ^= 1
    ref = SC.score_many("v0", lay, policy=pol)
    assert ref.steps[0].max() == opt.max() and (ref.summary[1:, 1] < ref.summary[0, 1]).all()
    got = lm.score_tables(up(lay), policy=up(pol))
    same(got, ref, "serpentine G=%d" % G)
    q = np.zeros((P7, S, 4), np.float32)
    q[np.arange(P7)[:, None], np.arange(S)[None], pol] = 1.0               # the same tables as q rows
    same(lm.score_tables(up(lay), q=up(q)), ref, "serpentine q G=%d" % G)


# ------------------------------------------------------------- memory and outputs
@functools.lru_cache(maxsize=None)
def guard_case(G):
    P = 259
    lays = H.bordered_random_layouts(12, G, 77)[np.arange(P) % 12]         # twelve mazes, a table of its own for each problem
    pol = np.random.RandomState(G).randint(0, 4, (P, G * G)).astype(np.uint8)
    return lays, pol, SC.score_many("v0", lays, policy=pol)


@pytest.mark.parametrize("G", [8, 17])
@pytest.mark.parametrize("problems", [1, 4, 5, 259])
def test_guard_words_and_omitted_outputs(lm, G, problems):
    """Through the C entry: each output between guard words that stay as they were; each nullable output omitted in turn;
    distances only, with no table"""
    S, GUARD, MARK = G * G, 64, -0x5A5A5A5B
    lays, pol, ref = guard_case(G)
    lay_d, pol_d = up(lays[:problems]), up(pol[:problems])
    abi = lm._abi
    p = abi.make_params(abi.VARIANT_V0, G, abi.LAYOUT_PER_ENV, 100, -1.0, -0.01, 100.0)
    sizes = {"optimal": problems * S, "steps": problems * S, "summary": problems * 4}
    cases = [dict(), dict(skip="optimal"), dict(skip="steps"), dict(skip="summary"), dict(skip="steps", table=False)]
    for case in cases:
        bufs = {k: torch.full((n + 2 * GUARD,), MARK, dtype=torch.int32, device=dev()) for k, n in sizes.items() if k != case.get("skip")}
        ptr = {k: (bufs[k].data_ptr() + 4 * GUARD if k in bufs else None) for k in sizes}
        table = case.get("table", True)
        rc = abi.lib.lmaze_score(C.byref(p), lay_d.data_ptr(), None, problems, pol_d.data_ptr() if table else None, None,
                                 ptr["optimal"], ptr["steps"], ptr["summary"], torch.cuda.current_stream().cuda_stream)
        assert rc == 0, case
        torch.cuda.synchronize()
        for k, b in bufs.items():
            b = b.cpu().numpy()
            assert (b[:GUARD] == MARK).all() and (b[-GUARD:] == MARK).all(), (case, k)
            want = getattr(ref, k)[:problems].reshape(-1).copy()
            if k == "summary" and not table:
                want.reshape(-1, 4)[:, 1:] = 0
            assert (b[GUARD:-GUARD] == want).all(), (case, k)
    only = lm.score_tables(lay_d, outputs=("optimal",))
    assert only.steps is None and only.summary is None and (only.optimal.cpu().numpy() == ref.optimal[:problems]).all()
    with pytest.raises(ValueError, match="above 3"):
        lm.score_tables(lay_d, policy=up(np.full((problems, S), 4, np.uint8)))
    with pytest.raises(ValueError, match="needs a table"):
        lm.score_tables(lay_d)


# ------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("G", [11, 12])
@pytest.mark.parametrize("loops", [0.0, 0.25])
def test_generated_solved_scored(lm, G, loops):
    """256 generated mazes, solve(gamma=0.99), score(policy=solved.policy): every free cell of every maze arrives, in the
    fewest steps; the first 24 mazes against the reference integer by integer (the host's generator gives the same mazes)"""
    N = 256
    lay = lm.layouts.mazes(N, G, dev(), seed=11, loops=loops)
    env = lm.LmazeVecEnv(N, "v0", per_env_layouts=lay, device=dev(), seed=3)
    solved = env.solve(gamma=0.99)
    got = env.score(policy=solved.policy)
    assert tuple(got.optimal.shape) == (N, G * G) and tuple(got.steps.shape) == (N, G * G) and tuple(got.summary.shape) == (N, 4)
    free = (lay != ord("W")).flatten(1).sum(1).to(torch.int32)
    s = got.summary
    assert bool((s[:, 0] == free).all() & (s[:, 1] == free).all() & (s[:, 2] == free).all() & (s[:, 3] == 0).all())
    assert bool((got.steps == got.optimal).all())
    host = lay[:24].cpu().numpy()
    ref = SC.score_many("v0", host, policy=solved.policy[:24].cpu().numpy())
    assert (ref.summary == np.stack([free[:24].cpu().numpy()] * 3 + [np.zeros(24, np.int32)], 1)).all()     # the CPU says so too
    same(lm.ScoredTables(got.optimal[:24], got.steps[:24], got.summary[:24]), ref, "pipeline G=%d" % G)
    same(env.score(q=solved.q), lm.ScoredTables(*[x.cpu().numpy() for x in got]), "pipeline q G=%d" % G)


def test_learned_table_counts_are_greedy_shares(lm):
    """The learner's table of qlearn_ref.learn_case(), uploaded: the sums of shortest and reachable are greedy_share's"""
    case = Q.learn_case()
    got = lm.score_tables(up(case["lay"]), q=up(case["q"]))
    s = got.summary.cpu().numpy().astype(np.int64)
    print("shortest", s[:, 2].sum(), "reachable", s[:, 0].sum(), "arrived", s[:, 1].sum(), "excess", s[:, 3].sum())
    assert (int(s[:, 2].sum()), int(s[:, 0].sum())) == (case["good"], case["total"])
    same(got, SC.score_many("v0", case["lay"], q=case["q"]), "learn_case")


# ------------------------------------------------------------- venv.score()
def test_env_score_shared_ball(lm):
    env = lm.LmazeVecEnv(3, variant="v0", device=dev())
    G = env.grid
    lay = lm.layouts.to_codes(lm.VARIANTS["v0"]["layout"])
    solved = env.solve()
    got = env.score(policy=solved.policy)
    assert tuple(got.optimal.shape) == (G * G,) and tuple(got.steps.shape) == (G * G,) and tuple(got.summary.shape) == (4,)
    ref = SC.score_many("v0", lay, policy=solved.policy.cpu().numpy()[None])
    same(lm.ScoredTables(got.optimal[None], got.steps[None], got.summary[None]), ref, "shared ball")
    none = env.score()
    assert none.steps is None and (none.optimal.cpu().numpy() == ref.optimal[0]).all()
    assert none.summary.tolist() == [int(ref.summary[0, 0]), 0, 0, 0]
    same(lm.ScoredTables(*[x[None] for x in env.score(q=solved.q)]), ref, "shared ball q")
    v3 = lm.LmazeVecEnv(2, variant="v3", device=dev())
    with pytest.raises(ValueError, match="goal="):
        v3.score()
    lay3 = lm.layouts.to_codes(lm.VARIANTS["v3"]["layout"])
    gx, gy = (int(c) for c in np.argwhere(lay3 == ord("B"))[5])
    one = v3.score(goal=(gx, gy))
    assert (one.optimal.cpu().numpy() == SC.score_many("v3", lay3, np.array([[gx, gy]], np.int32)).optimal[0]).all()


def test_env_score_key_goal(lm):
    """v3, the shipped 18x18 layout, every goal cell: solve(key="goal")'s policy arrives in the fewest steps wherever done can
    be reached; every 9th problem against the reference integer by integer"""
    env = lm.LmazeVecEnv(2, variant="v3", device=dev())
    G = env.grid
    S = G * G
    lay = lm.layouts.to_codes(lm.VARIANTS["v3"]["layout"])
    solved = env.solve(gamma=0.99, sweeps=1400, key="goal")
    got = env.score(policy=solved.policy, key="goal")
    assert tuple(got.optimal.shape) == (G ** 4,) and tuple(got.steps.shape) == (G ** 4,) and tuple(got.summary.shape) == (S, 4)
    s = got.summary.cpu().numpy()
    assert (s[:, 0] == s[:, 1]).all() and (s[:, 1] == s[:, 2]).all() and (s[:, 3] == 0).all() and s[:, 0].max() > 0
    assert (s[:, 0] == 0).any()                                            # goals nothing can pay for
    who = np.arange(0, S, 9)
    goals = np.stack([who // G, who % G], 1).astype(np.int32)
    pol = solved.policy.cpu().numpy().reshape(S, S)[who]
    ref = SC.score_many("v3", lay, goals, policy=pol)
    part = lm.ScoredTables(got.optimal.reshape(S, S)[who], got.steps.reshape(S, S)[who], got.summary[who])
    same(part, ref, "key=goal")
    with pytest.raises(ValueError):
        lm.LmazeVecEnv(2, variant="v0", device=dev()).score(key="goal")


@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_env_score_per_env_and_key_env(lm, variant):
    """Per-env layouts: env i's maze and (v3) its current goal; key="env" on a shared layout: N tables on the one maze"""
    N, G = 9, 11
    S = G * G
    lays = M.generate(G, N, 5, 0, 1 << 30)[0]
    env = lm.LmazeVecEnv(N, variant, per_env_layouts=lays, device=dev(), seed=4)
    env.reset()
    goals = env.goal_xy.cpu().numpy() if variant == "v3" else None
    solved = env.solve()
    got = env.score(q=solved.q)
    assert tuple(got.optimal.shape) == (N, S) and tuple(got.steps.shape) == (N, S) and tuple(got.summary.shape) == (N, 4)
    same(got, SC.score_many(variant, lays, goals, q=solved.q.cpu().numpy()), "per-env env.score")
    with pytest.raises(ValueError):
        env.score(policy=solved.policy, q=solved.q)
    if variant == "v3":
        with pytest.raises(ValueError):
            env.score(key="goal")
    shared = lm.LmazeVecEnv(N, variant, layout=lays[0], device=dev(), seed=4)
    shared.reset()
    goals = shared.goal_xy.cpu().numpy() if variant == "v3" else None
    pol = np.random.RandomState(3).randint(0, 4, (N, S)).astype(np.uint8)
    got = shared.score(policy=up(pol), key="env")
    assert tuple(got.optimal.shape) == (N, S) and tuple(got.summary.shape) == (N, 4)
    same(got, SC.score_many(variant, lays[0], goals, policy=pol), "shared key=env")
