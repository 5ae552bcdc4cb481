"""GPU: lmaze_generate against maze_ref.py (the specification restated in numpy: Philox draws, Kruskal, byte assembly), byte
for byte on the layouts and the goals -- both kernel forms (a wave per maze up to G = 33, a workgroup per maze above), every
rooms-per-lane form, maze counts ragged against the packing, maze offsets of every alignment with guard bytes around the
output, shards against the one-batch result -- and the pipeline the mazes are for: generate -> per-env layouts -> solve ->
rollout_policy(key="env"), every env reaching its goal."""
import importlib

import numpy as np
import pytest
import torch

import maze_ref as M

pytestmark = pytest.mark.gpu

SEEDS = (7, (0x9E3779B9 << 32) | 0x7F4A7C15)
BASES = (0, (1 << 33) + 5)
GUARD = 64


@pytest.fixture(scope="module")
def lm():
    assert torch.cuda.is_available()
    return importlib.import_module("gym-lmaze_amd")


def dev():
    return torch.device("cuda", 0)


def same(lay, goals, G, n, seed, base, loops_u32, what):
    want_lay, want_goal = M.generate(G, n, seed, base, loops_u32)
    got = lay.cpu().numpy()
    assert got.shape == want_lay.shape and got.dtype == np.uint8
    bad = int((got != want_lay).sum())
    if bad:
        p = int(np.argwhere(got != want_lay)[0][0])
        print(what, "maze", p, "got\n", "\n".join(r.tobytes().decode("latin1") for r in got[p]), "\nwant\n",
              "\n".join(r.tobytes().decode("latin1") for r in want_lay[p]))
    assert bad == 0, (what, bad, np.argwhere(got != want_lay)[:5].tolist())
    if goals is not None:
        g = goals.cpu().numpy()
        assert g.dtype == np.int32 and (g == want_goal).all(), (what, g.tolist(), want_goal.tolist())


@pytest.mark.parametrize("G", [5, 6, 8, 11, 12, 16, 32, 33, 34, 35, 63, 64])
def test_parity_sweep(lm, G):
    """7 mazes: the wave form's second workgroup is ragged.  No loops, a quarter of the walls, every wall; both words of the
    seed and of the maze index enter the draws."""
    abi = lm._abi
    for loops in (0.0, 0.25, None):
        loops_u32 = 0xFFFFFFFF if loops is None else abi.epsilon_u32(loops)
        for seed in SEEDS:
            for base in BASES:
                lay, goals = lm.layouts.mazes(7, G, dev(), seed=seed, loops=1.0 if loops is None else loops, maze_base=base,
                                              return_goals=True)
                same(lay, goals, G, 7, seed, base, loops_u32, "G=%d loops=%r seed=%#x base=%d" % (G, loops, seed, base))


@pytest.mark.parametrize("G", [17, 18, 19, 24, 25, 46, 47])
def test_every_other_form_and_threshold(lm, G):
    """The steps of the launch plan the sweep above does not land on: R = 8 (64 rooms on 64 lanes: no lane has a turn to
    spare for the goal's draw), two rooms per lane in the wave form (R = 9 .. 11) and its edges, the workgroup form's last
    size with two rooms per lane (R = 22) and first with four (R = 23)."""
    want = {17: "wave, 1", 18: "wave, 1", 19: "wave, 2", 24: "wave, 2", 25: "wave, 4", 46: "workgroup, 2", 47: "workgroup, 4"}[G]
    assert lm._abi.describe_generate(G, 5).startswith("generate_kernel<%s>" % want)
    for loops, base in ((0.0, BASES[1]), (0.25, 0)):
        lay, goals = lm.layouts.mazes(5, G, dev(), seed=SEEDS[1], loops=loops, maze_base=base, return_goals=True)
        same(lay, goals, G, 5, SEEDS[1], base, lm._abi.epsilon_u32(loops), "G=%d loops=%r base=%d" % (G, loops, base))


@pytest.mark.parametrize("G", [11, 35])
@pytest.mark.parametrize("n", [1, 4, 5, 259])
def test_counts_and_bounds(lm, G, n):
    """Into the middle of a buffer of 0xEE: the 64 bytes on either side stay as they were.  G*G is odd at both sizes, so the
    mazes start at every offset mod 4; goal_xy is not asked for."""
    S = G * G
    buf = torch.full((GUARD + n * S + GUARD,), 0xEE, dtype=torch.uint8, device=dev())
    out = buf[GUARD:GUARD + n * S].view(n, G, G)
    got = lm.layouts.mazes(n, G, dev(), seed=SEEDS[1], loops=0.25, maze_base=3, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xEE).all() and (host[-GUARD:] == 0xEE).all()
    assert not (host[GUARD:-GUARD] == 0xEE).any()
    same(out, None, G, n, SEEDS[1], 3, lm._abi.epsilon_u32(0.25), "guards G=%d n=%d" % (G, n))


def test_no_maze_is_no_launch(lm):
    lay, goals = lm.layouts.mazes(0, 11, dev(), return_goals=True)
    assert tuple(lay.shape) == (0, 11, 11) and tuple(goals.shape) == (0, 2)


@pytest.mark.parametrize("G", [11, 35])
def test_shards_hold_the_slices_of_one_batch(lm, G):
    whole = lm.layouts.mazes(10, G, dev(), seed=5, loops=0.25)
    parts = torch.cat([lm.layouts.mazes(4, G, dev(), seed=5, loops=0.25, maze_base=0),
                       lm.layouts.mazes(6, G, dev(), seed=5, loops=0.25, maze_base=4)])
    assert torch.equal(whole, parts)
    same(whole, None, G, 10, 5, 0, lm._abi.epsilon_u32(0.25), "shards G=%d" % G)


@pytest.mark.parametrize("G", [11, 12])
@pytest.mark.parametrize("loops", [0.0, 0.25])
def test_pipeline_generate_solve_act(lm, G, loops):
    """256 mazes -> LmazeVecEnv(per_env_layouts=) -> reset -> solve -> rollout_policy(key="env"): every env is done within 64
    steps (the longest path between two of the 25 rooms of a perfect maze is 24 edges, 48 moves), paid reward_goal bit for
    bit on its first done row, and every solve settles below the sweep cap."""
    N, T = 256, 64
    lay, goals = lm.layouts.mazes(N, G, dev(), seed=11, loops=loops, return_goals=True)
    env = lm.LmazeVecEnv(N, "v0", per_env_layouts=lay, device=dev(), seed=3)
    env.reset()
    solved = env.solve(gamma=0.99)
    sweeps = solved.sweeps_run.cpu().numpy()
    print("G", G, "loops", loops, "sweeps_run max", sweeps.max())
    assert (sweeps < 4096).all()
    out = env.rollout_policy(T, q=solved.q, key="env", epsilon=0, auto_reset=False, trajectory=True)
    reward_t, done_t = out[3].cpu().numpy(), out[4].cpu().numpy().astype(bool)
    assert done_t.any(0).all(), np.flatnonzero(~done_t.any(0))[:8]
    first = done_t.argmax(0)
    print("first done row: max", first.max())
    assert first.max() < 48
    assert (reward_t[first, np.arange(N)].view(np.uint32) == np.float32(env.rewards[2]).view(np.uint32)).all()
    # the goals handed back are the layouts' 'X' cells, what solve_tables(goals=) takes for v3
    g = goals.long()
    assert (lay[torch.arange(N, device=dev()), g[:, 0], g[:, 1]] == ord("X")).all()
