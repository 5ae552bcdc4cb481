"""CPU: the reference and the case table of loaded_state.py (no GPU).  The padded oracle equals the plain one bit for bit
on ordinary on-grid state; every per-env case of the table meets, in its reference run, the situations it is there for
(conditions on the table's seeds and sizes, not measurements); the placement rule holds on the fixed mazes; and every
kernel the launchers' describe sweep names for the table's shapes is run by one of its rows."""
import importlib
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

import helpers as H
import launch_matrix as M
import loaded_state as LS
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = LS.groups()
PER_ENV_CASES = [k for k in GROUPS if k[2] == LS.PER_ENV]


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


# ------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("G", [5, 11, 16])
@pytest.mark.parametrize("layout", [M.SHARED, M.PER_ENV])
@pytest.mark.parametrize("variant", ["v0", "v3"])
def test_padded_reference_is_the_plain_oracle_on_grid(variant, layout, G):
    """3 steps with resets from on-grid state on ordinary mazes: the state, every reward / done row, every step's planes."""
    N, T = 257, 3
    lays = H.bordered_random_layouts(N, G, 40 + G)
    lay = lays if layout == M.PER_ENV else np.ascontiguousarray(lays[0])
    rs = np.random.RandomState(G)
    st = dict(ball_xy=H.random_free_cells(np.broadcast_to(lay, (N, G, G)), 5, forbid=(ord("W"),)), goal_xy=H.random_free_cells(lays, 6),
              step_count=rs.randint(0, 4, N).astype(np.int32), reward=rs.choice(np.array([-1.0, -0.01, 100.0, -0.0], np.float32), N),
              done=(rs.rand(N) < 0.4).astype(np.uint8), goal_count=rs.randint(0, 5, N).astype(np.int32))
    acts = rs.randint(-1, 6, (T, N)).astype(np.int32)
    key = (LS.ROLLOUT_OBS, variant, LS.PER_ENV if layout == M.PER_ENV else LS.shared(0), G, N, T, 1)
    got = LS.run_reference(key, lay, st, acts, None, 7)
    # the plain oracle, as test_gpu_launch_matrix.py drives it
    p = O.params(O.VARIANT_V3 if variant == "v3" else O.VARIANT_V0, G, O.LAYOUT_PER_ENV if layout == M.PER_ENV else O.LAYOUT_SHARED,
                 LS.STEP_LIMIT, -1.0, -0.01, 100.0)
    w = {n: v.copy() for n, v in st.items()}
    obs = np.zeros((N, G, G), np.int32)
    for t in range(T):
        O.reset(p, lay, w["done"].copy(), LS.SEED, 7 + t, w["ball_xy"], w["goal_xy"] if variant == "v3" else None, w["step_count"],
                w["reward"], w["done"], None, env_base=LS.ENV_BASE)
        if variant == "v3":
            O.step_v3(p, lay, acts[t], w["ball_xy"], w["goal_xy"], w["step_count"], w["reward"], w["done"], obs)
        else:
            O.step_v0(p, lay, acts[t], w["ball_xy"], w["step_count"], w["reward"], w["done"], w["goal_count"], obs)
        assert got["slots"][t].tobytes() == obs.tobytes(), t
        assert got["rows"][0][t].tobytes() == w["reward"].tobytes() and got["rows"][1][t].tobytes() == w["done"].tobytes(), t
    for n in w:
        assert got["state"][n].tobytes() == w[n].tobytes(), n
    assert got["epoch"] == 7 + T
    fired = got["coverage"]
    assert fired["spawn3+"] > 0 and fired["ball_clamped"] == fired["target_clamped"] == fired["spawn0"] == 0


def test_padded_reset_places_as_the_plain_one_on_sparse_mazes():
    """O.reset on plain and on padded mazes places identically, whatever the spawn count; the padded step returns every
    ball on the grid from start coordinates in -3..G+2."""
    G, N = 5, 4000
    for variant in ("v0", "v3"):
        lay = LS.sparse_layouts(N, G, variant, 11)
        rs = np.random.RandomState(3)
        st = dict(ball_xy=rs.randint(1, G - 1, (N, 2)).astype(np.int32), goal_xy=rs.randint(-3, G + 3, (N, 2)).astype(np.int32),
                  step_count=np.zeros(N, np.int32), reward=np.zeros(N, np.float32), done=np.ones(N, np.uint8),
                  goal_count=np.zeros(N, np.int32))
        ref = LS.Reference(variant, LS.PER_ENV, G, N, lay)
        padded = {n: v.copy() for n, v in st.items()}
        ref.reset(padded, None, 9)
        p = O.params(O.VARIANT_V3 if variant == "v3" else O.VARIANT_V0, G, O.LAYOUT_PER_ENV, LS.STEP_LIMIT)
        O.reset(p, lay, None, LS.SEED, 9, st["ball_xy"], st["goal_xy"] if variant == "v3" else None, st["step_count"],
                st["reward"], st["done"], None, env_base=LS.ENV_BASE)
        for n in st:
            assert padded[n].tobytes() == st[n].tobytes(), (variant, n)
        c = LS.spawn_counts(lay, variant)
        assert min((c == 0).sum(), (c == 1).sum(), (c == 2).sum(), (c >= 3).sum()) > 400
        padded["ball_xy"][:] = rs.randint(-3, G + 3, (N, 2))
        ref.step(padded, rs.randint(-1, 6, N).astype(np.int32))
        assert ((padded["ball_xy"] >= 0) & (padded["ball_xy"] <= G - 1)).all()


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("G", [3, 4, 9, 12, 21, 62])
def test_fixed_mazes(abi, variant, G):
    """the fixed mazes validate, and have the spawn counts they are named for (abi: the package imports its built library)"""
    L = importlib.import_module("gym-lmaze_amd.layouts")
    counts = []
    for k in range(LS.N_FIXED):
        lay = LS.fixed_maze(k, G, variant, 5)
        L.validate(lay, need_goal_marker=variant == "v0")
        counts.append(int(LS.spawn_counts(lay, variant)))
    assert counts[0] == 0 and counts[4] == (1 if variant == "v3" else 0)
    if G >= 5:
        assert counts[1] == counts[2] == 1 and counts[3] == counts[6] == 2 and counts[7] >= 3
        assert counts[5] == {9: 2, 12: 3, 21: 7, 62: 60}[G]      # the 64-cell stretches that hold an interior cell, by hand
        five = LS.fixed_maze(5, G, "v3")
        assert five[G - 2, G - 2] != ord("W")                    # the last interior cell: the last ballot, the last register


# ------------------------------------------------------------- what the table's cases meet
@pytest.mark.parametrize("key", PER_ENV_CASES, ids=LS.case_id)
def test_every_per_env_case_meets_what_it_is_there_for(abi, key):
    """At least 8 envs (1 in the N = 13 cases) in every situation the case's entry point and grid admit
    (loaded_state.required_coverage): a reset that fired on 0, 1, 2 and >= 3 spawn cells, a reset that left the ball, a ball
    and a target clamped, a move off a wall cell, a v3 goal off the grid and one placed alone, a v0 sticky pair with every
    special reward pattern."""
    entry, variant, layout, G, N, T, k = key
    lay = LS.case_layouts(key)
    importlib.import_module("gym-lmaze_amd.layouts").validate(lay, need_goal_marker=variant == "v0")
    st, acts, mask = LS.loaded_state(key, lay)
    act = LS.closed_loop_actions(key, LS.closed_loop_table(key)) if entry in LS.CLOSED else None
    out = LS.run_reference(key, lay, LS.host_state_of(key, lay, st), acts, mask, 1, act)
    cov = out["coverage"]
    floor = 8 if N > LS.N_SMALL else 1
    print(LS.case_id(key), dict(cov))
    short = {n: cov[n] for n in LS.required_coverage(key) if cov[n] < floor}
    assert not short, (short, "wanted %d" % floor)
    if not LS.interior_only(G) and entry not in LS.RESETS_ONLY:
        b = st["ball_xy"]
        assert ((b < 0) | (b > G - 1)).any() and ((b >= 0) & (b <= G - 1)).all(1).any()
    assert set(np.unique(st["done"])) == {0, 1, 2, 255} or N <= LS.N_SMALL


def test_the_table_is_small_and_complete():
    per_family = defaultdict(set)
    for r in LS.ROWS:
        assert r.N * r.G * r.G * 4 <= 16 << 20 and r.T <= LS.T_STEPS, r
        fam = "reset" if r.entry in LS.RESETS_ONLY else "observe" if r.entry in LS.OBSERVES else "step" if r.entry in LS.STEPS else \
            "closed" if r.entry in LS.CLOSED else "rollout"
        per_family[fam].add(r.N)
    for fam, ns in per_family.items():
        assert {LS.N_SMALL, LS.N_TINY} <= ns, fam
    assert len(GROUPS) < 900


# ------------------------------------------------------------- the kernels the table runs
def _restricted_sweep(abi):
    """launch_matrix.sweep() at the table's own (variant, layout, G): the step calls at those of its step rows, the rollout
    calls at those of its rollout rows (int32 and u8 apart) and under the hints those rows use.  Batches up to 1000 envs:
    the streaming ("nt") forms and the 65 536-env wave grouping are another store policy, not another transition, and are
    launch_matrix's to run."""
    steps = {(r.variant, LS.PER_ENV if r.layout == LS.PER_ENV else M.SHARED, r.G) for r in LS.ROWS if r.entry in (LS.STEP, LS.STEP_RESET)}
    rolls = defaultdict(set)
    for r in LS.ROWS:
        if r.entry in LS.ROLLOUTS:
            rolls[(r.variant, LS.PER_ENV if r.layout == LS.PER_ENV else M.SHARED, r.G, r.entry in LS.U8)].add(r.hint)
    grids = sorted({g for _, _, g in steps} | {k[2] for k in rolls})
    for call, text in M.sweep(abi, grids=grids, ns=(1, 1000)):
        if not text:
            continue
        if call[0] == "step":
            _, variant, layout, G, n, h, ar, with_obs = call
            if (variant, layout, G) in steps:
                yield call, text
        else:
            _, variant, layout, G, n, h, T, ar, with_obs, k = call
            if h in rolls.get((variant, layout, G, with_obs == "u8"), ()) and (T > 1 or with_obs != "u8"):
                yield call, text


def test_every_kernel_the_restricted_sweep_names_has_a_row(abi):
    where = defaultdict(list)
    for call, text in _restricted_sweep(abi):
        where[M.kernel_key(text)].append(call)
    covered = {M.kernel_key(LS.describe(abi, *r)) for r in LS.ROWS if LS.describe(abi, *r)}
    missing = sorted(set(where) - covered)
    assert not missing, "kernels no row of loaded_state.ROWS runs (one call that picks each): " + "; ".join(
        "%s <- %s" % (k, where[k][0]) for k in missing)
    assert len(where) >= 40, len(where)
    closed = {M.kernel_key(LS.describe(abi, *r)).split(" epb")[0] for r in LS.ROWS if r.entry in LS.CLOSED}
    assert {"rollout_shared_kernel<policy=ball, obs_t>", "rollout_perenv_kernel<policy=ball, obs_t>",
            "rollout_shared_kernel<policy=goal, obs_t>", "rollout_perenv_kernel<policy=goal, obs_t>",
            "rollout_shared_kernel<sample=ball, table=lds, obs_t>", "rollout_perenv_kernel<sample=ball, table=lds, obs_t>",
            "rollout_shared_kernel<sample=goal, table=global, obs_t>", "rollout_perenv_kernel<sample=goal, table=global, obs_t>"} <= closed, closed
