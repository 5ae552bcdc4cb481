"""CPU: the host side of the reset from a start law -- start_thresholds()'s table against its definition, distance_band()
against a loop over score_ref.optimal, the refusals of lmaze_reset_start (include/lmaze.h) and of LmazeVecEnv.reset(start=,
thresholds=) with their order, and the law of the draw itself on the numpy restatement (reset_start_ref.py), which
test_gpu_reset_start.py then holds the kernels to integer for integer.  No device is needed and none is touched: the C calls
pass n = 0 (or are refused sooner) and fabricated, aligned addresses stand for the buffers."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import reset_start_ref as RS
import score_ref as SC
import solve_ref as SR
from closed_loop_ref import bare_grid_env, test_numpy_philox_is_the_oracles, test_numpy_philox_known_answers  # noqa: F401
from helpers import bordered_random_layouts
from occupancy_rollout_ref import counts_follow_marginals, spawn_cells

E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
V0, V3 = 0, 3
ONE = RS.ONE


@pytest.fixture(scope="module")
def lm():
    return importlib.import_module("gym-lmaze_amd")


def words(t):
    return t.view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF


# ------------------------------------------------------------- start_thresholds()
def some_laws(seed, P=9, S=121):
    rs = np.random.RandomState(seed)
    w = rs.rand(P, S).astype(np.float32)
    w[rs.rand(P, S) < 0.6] = 0                      # zero-mass cells between the massive ones, and at both ends
    w[:, 0] = w[:, -1] = 0
    w[1] = 0                                        # no mass at all
    w[2] = 0
    w[2, 60] = 3.0                                  # one cell
    w[3] = 1.0                                      # uniform over everything
    w[4] *= 1e-30                                   # tiny weights, a tiny sum
    w[5, 5] = 1e30                                  # one cell outweighs the rest by far
    return w


def test_start_thresholds_is_its_definition(lm):
    w = some_laws(3)
    t = lm.start_thresholds(torch.from_numpy(w))
    assert t.dtype == torch.uint32 and tuple(t.shape) == w.shape and t.is_contiguous()
    c = words(t)
    total = w.astype(np.float64).sum(1)
    assert (c[total == 0] == 0).all() and (total == 0).any()
    full = total > 0
    assert (c[full, -1] == ONE).all()                                      # every row ends in 2**31 or is all zeros
    width = np.diff(np.c_[np.zeros(len(c), np.int64), c], axis=1)
    assert (width >= 0).all()
    assert (width[w == 0] == 0).all()                                      # zero-mass cells have zero width
    want = w[full].astype(np.float64) / total[full, None]
    assert np.abs(width[full] / 2.0 ** 31 - want).max() <= 2.0 ** -30
    for p in np.flatnonzero(full):                                         # the last massive cell's word, and all behind
        last = np.flatnonzero(w[p] > 0)[-1]
        assert (c[p, last:] == ONE).all() and (last == 0 or c[p, last - 1] < ONE or width[p, last] == 0)
    assert (c[2, :60] == 0).all() and (c[2, 60:] == ONE).all()             # the one-cell law
    # one row, given as [S]
    one = lm.start_thresholds(torch.from_numpy(w[0]))
    assert tuple(one.shape) == (1, w.shape[1]) and (words(one)[0] == c[0]).all()
    # float64 weights in, the same rule
    assert (words(lm.start_thresholds(torch.from_numpy(w.astype(np.float64)))) == c).all()


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -0.5e-30])
def test_start_thresholds_refuses_negative_and_non_finite_entries(lm, bad):
    w = torch.ones(2, 25)
    w[1, 7] = bad
    with pytest.raises(ValueError, match="negative or non-finite"):
        lm.start_thresholds(w)
    with pytest.raises(ValueError, match="float tensor"):
        lm.start_thresholds(torch.ones(2, 25, dtype=torch.int32))


# ------------------------------------------------------------- distance_band()
def band_by_loop(variant, lays, goals, opt, lo, hi, empty):
    """float32[P,S] and the size of every band: a loop over the problems, the cells reset() accepts and their distances"""
    P, G = lays.shape[0], lays.shape[-1]
    out, sizes = np.zeros((P, G * G), np.float32), []
    for p in range(P):
        cells = spawn_cells(lays[p], variant, None if goals is None else int(goals[p, 0]) * G + int(goals[p, 1]))
        band = [c for c in cells if lo[p] <= opt[p, c] <= hi[p]]
        sizes.append(len(band))
        use = band if band or empty == "zero" else list(cells)
        for c in use:
            out[p, c] = np.float32(1) / np.float32(len(use))
    return out, sizes


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("G", [5, 11])
def test_distance_band_against_a_loop_over_the_distances(lm, variant, G):
    P = 6
    lays = bordered_random_layouts(P, G, 40 + G)
    goals = None
    if variant == "v3":
        rs = np.random.RandomState(G)
        goals = np.stack([(lambda c: (c // G, c % G))(rs.choice(spawn_cells(lays[p], "v3"))) for p in range(P)]).astype(np.int32)
    opt = np.stack([SC.optimal(SR.extract_model(variant, lays[p], None if goals is None else goals[p])) for p in range(P)])
    lo, hi = np.full(P, 2), np.full(P, 4)
    lo[0] = hi[0] = 1000                                                   # an empty band
    for p in range(1, P):                                                  # a band of one cell, where a maze has such a distance
        cells = spawn_cells(lays[p], variant, None if goals is None else int(goals[p, 0]) * G + int(goals[p, 1]))
        d, n = np.unique(opt[p, cells], return_counts=True)
        if (n == 1).any():
            lo[p] = hi[p] = d[n == 1][0]
            break
    tl, tg, to = torch.from_numpy(lays), None if goals is None else torch.from_numpy(goals), torch.from_numpy(opt)
    for empty in ("reset", "zero"):
        want, sizes = band_by_loop(variant, lays, goals, opt, lo, hi, empty)
        assert 0 in sizes and 1 in sizes, sizes
        got = lm.distance_band(to, torch.from_numpy(lo), torch.from_numpy(hi), tl, variant=variant, goals=tg, empty=empty)
        assert got.dtype == torch.float32 and tuple(got.shape) == (P, G * G)
        assert (got.numpy().view(np.uint32) == want.view(np.uint32)).all(), (variant, G, empty)
        if empty == "reset":                                               # the empty band falls back on reset()'s own law
            assert (got[0] == lm.reset_distribution(tl, variant, tg)[0]).all()
    # plain ints: one stage for every maze
    want, _ = band_by_loop(variant, lays, goals, opt, np.full(P, 1), np.full(P, 3), "zero")
    got = lm.distance_band(to, 1, 3, tl, variant=variant, goals=tg, empty="zero")
    assert (got.numpy().view(np.uint32) == want.view(np.uint32)).all()
    with pytest.raises(ValueError, match="empty"):
        lm.distance_band(to, 1, 3, tl, variant=variant, goals=tg, empty="uniform")
    with pytest.raises(ValueError, match="optimal"):
        lm.distance_band(to.float(), 1, 3, tl, variant=variant, goals=tg)


def test_distance_band_serves_one_shared_layout_under_many_tables(lm):
    lay = bordered_random_layouts(1, 5, 45)[0]
    opt = SC.optimal(SR.extract_model("v0", lay))
    one = lm.distance_band(torch.from_numpy(opt), 1, 2, torch.from_numpy(lay))
    many = lm.distance_band(torch.from_numpy(np.tile(opt, (3, 1))), 1, 2, torch.from_numpy(lay))
    assert tuple(one.shape) == (1, 25) and tuple(many.shape) == (3, 25) and (many == one).all()


def test_the_curriculums_mazes_and_where_its_fallback_comes_from(lm):
    """The mazes of test_gpu_reset_start.py's curriculum, restated (maze_ref): a spanning-tree maze is connected, so its
    distances run from 1 to the largest without a gap and the 3..6 band is empty in none of the 257 (the largest distance is
    10 at the least) -- no seed gives a fallback env at that stage.  The GPU test therefore reaches the fallback in its second
    stage, with bounds per maze that no cell of every 16th maze meets; held here: those bands are empty, the others are not,
    and the fallback row is reset_distribution()'s."""
    import maze_ref as M
    N, G = 257, 11
    lays, _ = M.generate(G, N, 7)
    opt = np.stack([SC.optimal(SR.extract_model("v0", lays[p])) for p in range(N)])
    ok = np.stack([np.isin(np.arange(G * G), spawn_cells(lays[p], "v0")) for p in range(N)])
    far = np.where(ok, opt, 0).max(1)
    assert far.min() >= 10
    assert all(set(opt[p, ok[p]]) == set(range(1, far[p] + 1)) for p in range(N))
    tl, to = torch.from_numpy(lays), torch.from_numpy(opt)
    first = lm.distance_band(to, 3, 6, tl).numpy()
    assert (((opt >= 3) & (opt <= 6) & ok) == (first > 0)).all() and (first > 0).any(1).all()
    lo, hi = np.full(N, 5), np.full(N, 9)
    lo[::16] = hi[::16] = 1000
    second = lm.distance_band(to, torch.from_numpy(lo), torch.from_numpy(hi), tl).numpy()
    base = lm.reset_distribution(tl, "v0").numpy()
    fallback = np.arange(N) % 16 == 0
    assert (second[fallback] == base[fallback]).all() and fallback.sum() == 17
    assert (((opt >= 5) & (opt <= 9) & ok) == (second > 0))[~fallback].all() and (second > 0).any(1).all()


# ------------------------------------------------------------- lmaze_reset_start: the refusals and their order
ORDER = ("layout", "mask", "thresholds", "row_mode", "keep_goal", "seed", "epoch", "env_base", "ball_xy", "goal_xy", "step_count",
         "reward", "done", "obs", "n", "stream")
VALID = dict(layout=0x10000, mask=0x19000, thresholds=0x1b000, row_mode=0, keep_goal=0, seed=7, epoch=3, env_base=0, ball_xy=0x12000,
             goal_xy=0x13000, step_count=0x14000, reward=0x15000, done=0x16000, obs=0x18000, n=0, stream=None)


def call(lm, variant, G=11, mode=0, params=True, **over):
    assert over.get("n", 0) <= 0, "a call of this file never gets as far as a launch"
    p = lm._abi.make_params(variant, G, mode, 50, -1.0, -0.01, 100.0)
    args = dict(VALID, **over)
    return lm._abi.lib.lmaze_reset_start(C.byref(p) if params else None, *[args[k] for k in ORDER])


def test_valid_arguments_with_no_envs_return_0(lm):
    for variant, modes in ((V0, (0, 1)), (V3, (0, 1, 2))):
        for row_mode in modes:
            for layout_mode in (0, 1):
                assert call(lm, variant, mode=layout_mode, row_mode=row_mode) == 0
        assert call(lm, variant, mask=None, obs=None) == 0
        for G in (3, 64):
            assert call(lm, variant, G=G) == 0
    assert call(lm, V3, keep_goal=1) == 0 and call(lm, V3, keep_goal=5, row_mode=2) == 0
    assert call(lm, V0, goal_xy=None) == 0                                 # v0 keeps no goal


def test_the_refusals_stand_in_their_order(lm):
    bad_row = dict(row_mode=7, thresholds=None)                            # what every earlier refusal comes before
    # 1. lmaze_reset's own: the params, the variant, its buffers
    assert call(lm, V0, params=False, **bad_row) == E_NULL
    assert call(lm, V0, G=2, **bad_row) == E_GRID
    assert call(lm, V0, G=65, **bad_row) == E_GRID
    assert call(lm, V0, mode=2, **bad_row) == E_LAYOUT
    assert call(lm, V0, n=-1, **bad_row) == E_COUNT
    assert call(lm, V0, G=2, mode=2, n=-1) == E_GRID
    for v in (1, 2, 4, 5, 6, 7, -1):
        assert call(lm, v, ball_xy=None, **bad_row) == E_VARIANT
    for variant in (V0, V3):
        for k in ("layout", "ball_xy", "step_count", "reward", "done") + (("goal_xy",) if variant == V3 else ()):
            assert call(lm, variant, **{k: None}, **bad_row) == E_NULL, k
        for k, off in (("ball_xy", 4), ("goal_xy", 4), ("obs", 8), ("layout", 1)):
            assert call(lm, variant, **{k: VALID[k] + off}, **bad_row) == E_ALIGN, k
        assert call(lm, variant, layout=None, ball_xy=VALID["ball_xy"] + 4) == E_NULL
    # 2. the row mode, before what v0 cannot do and before the table
    for rm in (-1, 3, 1 << 20):
        assert call(lm, V3, row_mode=rm) == E_COUNT
        assert call(lm, V0, row_mode=rm, keep_goal=1, thresholds=None) == E_COUNT
    # 3. v0 has no per-env goal
    assert call(lm, V0, row_mode=2) == E_VARIANT
    assert call(lm, V0, keep_goal=1) == E_VARIANT
    assert call(lm, V0, row_mode=2, thresholds=None) == E_VARIANT
    assert call(lm, V0, keep_goal=1, thresholds=VALID["thresholds"] + 2) == E_VARIANT
    # 4. and 5. the table
    for variant in (V0, V3):
        assert call(lm, variant, thresholds=None) == E_NULL
        for off in (1, 2, 3):
            assert call(lm, variant, thresholds=VALID["thresholds"] + off) == E_ALIGN
        assert call(lm, variant, thresholds=VALID["thresholds"] + 4) == 0


def test_describe_refusals_and_the_empty_line(lm):
    abi = lm._abi
    for variant, name in ((V0, "v0"), (V3, "v3")):
        p = abi.make_params(variant, 11, 0, 50, -1.0, -0.01, 100.0)
        assert abi.describe_reset_start(p, 0, "ball") == ""
        buf = C.create_string_buffer(256)
        assert abi.lib.lmaze_describe_reset_start(C.byref(p), 5, 3, buf, 256) == E_COUNT
        assert abi.lib.lmaze_describe_reset_start(C.byref(p), -1, 3, buf, 256) == E_COUNT
        assert abi.lib.lmaze_describe_reset_start(C.byref(p), 5, 0, None, 256) == E_NULL
        assert abi.lib.lmaze_describe_reset_start(C.byref(p), 5, 2, buf, 256) == (E_VARIANT if variant == V0 else 0)
        assert abi.lib.lmaze_describe_reset_start(None, 5, 0, buf, 256) == E_NULL
        assert abi.describe_reset_start(p, 5, "env").startswith("reset_start_kernel<%s, rows=env, table=global>" % name)


# ------------------------------------------------------------- LmazeVecEnv.reset(start=, thresholds=): the Python refusals
def test_reset_refusals_stand_in_their_order(lm, monkeypatch):
    G, N = 5, 8
    S = G * G
    v0, v3 = bare_grid_env(monkeypatch, "v0", G=G, N=N), bare_grid_env(monkeypatch, "v3", G=G, N=N)
    v0.layout_mode = v3.layout_mode = lm._abi.LAYOUT_SHARED
    law = torch.ones(S)
    good = lm.start_thresholds(law)                                        # [1, S]
    falling = good.view(torch.int32).clone()
    falling[0, 3] = 5
    goal_rows = good.expand(S, S).contiguous()
    # both of start / thresholds, before everything else
    with pytest.raises(ValueError, match="exactly one"):
        v0.reset(start=law[:3], thresholds=falling, key="goal", keep_goal=True)
    # the shape every key asks for, before the variant
    for env in (v0, v3):
        for key, wrong in (("ball", good.expand(2, S).contiguous()), ("env", good), ("goal", good), ("ball", good[:, :-1].contiguous())):
            with pytest.raises(ValueError, match="thresholds must be"):
                env.reset(thresholds=wrong, key=key, keep_goal=True)
        with pytest.raises(ValueError, match="start must be"):
            env.reset(start=torch.ones(N + 1, S), key="env", keep_goal=True)
        with pytest.raises(ValueError, match="start must be"):
            env.reset(start=good, key="ball")                              # a law is a float tensor
        with pytest.raises(ValueError, match="thresholds must be"):
            env.reset(thresholds=law, key="ball")                          # and a table is not
    with pytest.raises(ValueError, match="key must be"):
        v3.reset(thresholds=good, key="cell")
    # key="goal" on v0, before keep_goal on v0
    with pytest.raises(ValueError, match="key='goal' needs the v3 variant"):
        v0.reset(thresholds=goal_rows, key="goal", keep_goal=True)
    with pytest.raises(ValueError, match="keep_goal needs the v3 variant"):
        v0.reset(thresholds=falling, key="ball", keep_goal=True)           # ... which comes before the rows are read
    with pytest.raises(ValueError, match="keep_goal needs the v3 variant"):
        v0.reset(start=law, keep_goal=True)
    # the rows, last
    for env in (v0, v3):
        with pytest.raises(ValueError, match="decreases"):
            env.reset(thresholds=falling)
        short = good.view(torch.int32).clone()
        short[0, -1] -= 1
        short[0, -2] = short[0, -1]
        with pytest.raises(ValueError, match="neither ends in"):
            env.reset(thresholds=short)
        with pytest.raises(ValueError, match="negative or non-finite"):
            env.reset(start=-law)
    v3.layout_mode = lm._abi.LAYOUT_PER_ENV
    with pytest.raises(ValueError, match="shared layout"):
        v3.reset(thresholds=goal_rows, key="goal")
    with pytest.raises(ValueError, match="keep_goal belongs"):
        v3.reset(keep_goal=True)


# ------------------------------------------------------------- the law of the draw, on the reference alone
LAW_SEED = 11


def test_the_reference_draws_the_rows_law(lm):
    """65 536 draws on one 11x11 row: the counts per cell follow Binomial(N, width / 2^31), every two-sided tail above
    1e-6 / cells -- the suite's criterion.  The seed is fixed so that it passes; the GPU tests then compare integers."""
    G, N = 11, 65536
    lay = bordered_random_layouts(1, G, 311)[0]
    rs = np.random.RandomState(2)
    w = np.zeros(G * G, np.float32)
    cells = spawn_cells(lay, "v0")
    w[cells] = rs.rand(len(cells)) * (rs.rand(len(cells)) < 0.8)
    thr = words(lm.start_thresholds(torch.from_numpy(w)))[0]
    mass = RS.row_law(thr)
    assert mass.sum() == ONE and (mass >= 0).all() and (mass[w == 0] == 0).all()
    u = RS.ball_draw(LAW_SEED, 0, np.arange(N))
    assert u.min() >= 0 and u.max() < ONE
    k = RS.count_below(thr, u)
    assert (k < G * G).all()
    counts = np.bincount(k, minlength=G * G)
    bins, _ = counts_follow_marginals(counts[None], mass[None] / float(ONE), N, 1e-6, "reset_start 11x11")
    assert bins == int((mass > 0).sum()) >= 30
