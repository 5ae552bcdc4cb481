"""CPU: lmaze_generate / lmaze_describe_generate without a GPU -- the specification restated in numpy against itself
(maze_ref.py: Kruskal is the definition, a round-synchronous Boruvka must find the same tree inside the loop bounds the kernel
fixes), the properties the header promises of every maze, every documented refusal in its order of precedence (answered
before any device call), the launch the describe call names for every grid size, and what the kernels need."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import maze_ref as M
from closed_loop_ref import test_numpy_philox_is_the_oracles, test_numpy_philox_known_answers  # noqa: F401  (collected here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_COUNT, E_ALIGN = -1, -2, -5, -6
MAX_ENVS = 1 << 30
SEED = (0xC0FFEE << 32) | 0x1234567


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


# ------------------------------------------------------------- the reference itself
def test_edge_table_is_the_headers():
    """R, the rooms' cells, which edges exist and where their wall cells lie, at an odd and an even G."""
    assert [M.rooms_per_side(G) for G in (5, 6, 11, 12, 33, 34, 64)] == [2, 2, 5, 5, 16, 16, 31]
    for G in (5, 6, 11, 12):
        R = M.rooms_per_side(G)
        e = M.edge_table(G)
        assert len(e) == 2 * R * (R - 1) and len(set(e[:, 0].tolist())) == len(e) and e[:, 0].max() < 2 * R * R
        for k, u, v, wx, wy in e.tolist():
            i, j = divmod(k >> 1, R)
            assert u == k >> 1 and v == (u + 1 if k & 1 else u + R)
            assert (wx, wy) == ((1 + 2 * i, 2 + 2 * j) if k & 1 else (2 + 2 * i, 1 + 2 * j))
            assert (j + 1 < R) if k & 1 else (i + 1 < R)


@pytest.mark.parametrize("G", M.GRIDS)
def test_kruskal_is_boruvka_within_the_loop_bounds(G):
    """21 mazes of every G (210 in all): the two trees are the same edge for edge; the Boruvka rounds and the pointer-jump
    passes of a round stay within ceil(log2(R*R)), the trip count the kernel fixes; R*R - 1 edges are opened."""
    RR = M.rooms_per_side(G) ** 2
    bound = M.log2_ceil(RR)
    assert (1 << bound) >= RR > (1 << (bound - 1))
    worst_rounds = worst_passes = 0
    for m in list(range(19)) + [(1 << 33) + 5, (1 << 40) + 7]:
        keys, _ = M.edge_keys(G, M.draws(G, SEED, m))
        assert len(set(keys.tolist())) == len(keys)                        # distinct: the tree is unique
        want = M.kruskal(G, keys)
        got, rounds, passes = M.boruvka(G, keys)
        assert (got == want).all(), (G, m)
        assert int(want.sum()) == RR - 1
        worst_rounds, worst_passes = max(worst_rounds, rounds), max(worst_passes, passes)
    print("G", G, "rooms", RR, "bound", bound, "rounds", worst_rounds, "passes", worst_passes)
    assert 1 <= worst_rounds <= bound and worst_passes <= bound


@pytest.mark.parametrize("G", M.GRIDS)
@pytest.mark.parametrize("loops_u32", [0, 1 << 30, 0xFFFFFFFF])
def test_every_maze_keeps_the_promises(G, loops_u32):
    R = M.rooms_per_side(G)
    L = importlib.import_module("gym-lmaze_amd.layouts")
    lays, goals = M.generate(G, 5, SEED, 3, loops_u32)
    L.validate(lays)
    assert np.isin(lays, [M.W, M.B, M.X]).all()                            # no 'S'
    e = M.edge_table(G)
    for p in range(5):
        lay = lays[p]
        assert M.connected(lay), (G, p)
        assert int((lay == M.X).sum()) == 1
        gx, gy = goals[p]
        assert lay[gx, gy] == M.X and gx % 2 == 1 and gy % 2 == 1 and gx < 2 * R and gy < 2 * R
        rooms = lay[1:2 * R:2, 1:2 * R:2]
        assert int((rooms != M.W).sum()) == R * R
        opened = int((lay[e[:, 3], e[:, 4]] == M.B).sum())
        assert int((lay != M.W).sum()) == R * R + opened                    # nothing but rooms and edge cells is free
        if loops_u32 == 0:
            assert opened == R * R - 1
        elif loops_u32 == 0xFFFFFFFF:
            assert opened >= len(e) - 1                                     # a draw of 2^32 - 1 alone stays shut
        else:
            assert R * R - 1 <= opened <= len(e)
        if G % 2 == 0:
            assert (lay[G - 2, :] == M.W).all() and (lay[:, G - 2] == M.W).all()
    # the loops only add to the tree, and maze_base + p is the maze
    perfect, _ = M.generate(G, 5, SEED, 3, 0)
    assert ((perfect != M.W) <= (lays != M.W)).all()
    assert (M.generate(G, 2, SEED, 6, loops_u32)[0] == lays[3:5]).all()


def test_the_specification_is_not_degenerate():
    """2 000 mazes at G = 11: every room is the goal of some maze, every edge is in some tree, and no two mazes are alike."""
    G = 11
    R = M.rooms_per_side(G)
    e = M.edge_table(G)
    lays, goals = M.generate(G, 2000, 7)
    rooms = set(((goals[:, 0] - 1) // 2 * R + (goals[:, 1] - 1) // 2).tolist())
    assert rooms == set(range(R * R))
    in_tree = (lays[:, e[:, 3], e[:, 4]] == M.B)
    assert in_tree.any(0).all() and (in_tree.sum(1) == R * R - 1).all()
    assert len({lay.tobytes() for lay in lays}) == 2000
    share = in_tree.mean(0)
    print("edge shares: min %.3f max %.3f" % (share.min(), share.max()))


# ------------------------------------------------------------- refusals
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_generate", "lmaze_describe_generate"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    L = importlib.import_module("gym-lmaze_amd.layouts")
    assert callable(L.mazes) and callable(L.random_walled) and callable(abi.describe_generate)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("R = (G - 1) / 2", "counter (m_lo, m_hi, r, 0x40000000)", "(weight(k) & 0xFFFFF800) | k", "minimum spanning tree",
                   "Kruskal in ascending key order is the definition", "loop draw < loops_u32", "(uint64(goal draw) R R) >> 32",
                   "There is no 'S'", "no reference counterpart (the reference only has literal layouts)",
                   "epoch_hi ^ 0x80000000", "ceil(log2(R R))"):
        assert phrase in flat, phrase


def test_generate_refusals_in_order(abi):
    f = abi.lib.lmaze_generate

    def call(grid=11, mazes=3, seed=7, base=0, loops=0, lay=64, goal=64):
        return f(grid, mazes, seed, base, loops, lay, goal, None)
    # 1. layouts
    assert call(lay=None) == E_NULL
    assert call(lay=None, grid=4, mazes=-1, goal=4) == E_NULL
    # 2. the grid
    for g in (4, 3, 0, -1, 65):
        assert call(grid=g) == E_GRID
        assert call(grid=g, mazes=-1, base=-1, lay=8, goal=4) == E_GRID
    # 3. the counts
    assert call(mazes=-1) == E_COUNT and call(mazes=MAX_ENVS + 1) == E_COUNT
    assert call(base=-1) == E_COUNT and call(base=-1, mazes=0) == E_COUNT
    assert call(base=(1 << 63) - 1, mazes=1) == E_COUNT and call(base=(1 << 63) - 3, mazes=3) == E_COUNT
    assert call(base=(1 << 63) - 1, mazes=0) == 0 and call(base=(1 << 63) - 4, mazes=0, lay=16) == 0
    assert call(mazes=-1, lay=8, goal=4) == E_COUNT                        # before the alignment
    # 4. alignment
    for kw in (dict(lay=8), dict(lay=65), dict(lay=48 + 4), dict(goal=4), dict(goal=66)):
        assert call(**kw) == E_ALIGN, kw
        assert call(mazes=0, **kw) == E_ALIGN, kw                          # before "nothing to do"
    # 5. nothing to do: nothing is written, whatever the addresses
    for kw in (dict(), dict(goal=None), dict(grid=5), dict(grid=64), dict(loops=0xFFFFFFFF), dict(seed=(1 << 64) - 1)):
        assert call(mazes=0, **kw) == 0, kw
    # a grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration (9), from grid_ok, before any launch
    assert call(grid=34, mazes=1 << 24) == 9
    assert call(grid=33, mazes=1 << 26) == 9


def test_describe_generate_refusals(abi):
    d = abi.lib.lmaze_describe_generate
    buf = C.create_string_buffer(256)
    assert d(11, 1, None, 256) == E_NULL and d(11, 1, buf, 0) == E_NULL and d(4, -1, None, 256) == E_NULL
    assert d(4, 1, buf, 256) == E_GRID and d(65, -1, buf, 256) == E_GRID
    assert d(11, -1, buf, 256) == E_COUNT and d(11, MAX_ENVS + 1, buf, 256) == E_COUNT
    buf.value = b"stale"
    assert d(11, 0, buf, 256) == 0 and buf.value == b""
    assert abi.describe_generate(11, 0) == ""
    assert d(11, 5, buf, 11) == 0 and buf.value == b"generate_k"            # truncated to len, always terminated
    with pytest.raises(abi.LmazeError):
        abi.describe_generate(4, 1)


# ------------------------------------------------------------- what a describe line must say
def plan_lds(G, mazes_per_workgroup):
    """The LDS of a workgroup as lmaze_generate.hip lays it out: per maze 2 R*R keys, three words and a cell index per room
    and the G*G bytes with room for their shift, every array rounded up to 16 bytes; the workgroup form's eight vote words."""
    RR = M.rooms_per_side(G) ** 2

    def up(b):
        return (b + 15) & ~15
    per_maze = up(8 * RR) + 3 * up(4 * RR) + up(2 * RR) + up(G * G + 6)
    return mazes_per_workgroup * per_maze + (32 if mazes_per_workgroup == 1 else 0)


def test_describe_generate_every_grid(abi):
    forms = set()
    for G in range(5, 65):
        RR = M.rooms_per_side(G) ** 2
        for mazes in (1, 4, 5, 259, 65536):
            line = abi.describe_generate(G, mazes)
            m = re.match(r"generate_kernel<(wave|workgroup), (\d+)> grid=", line)
            assert m, line
            f = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}
            mpw, rpl = f["mazes_per_workgroup"], int(m.group(2))
            wave = G <= 33
            assert m.group(1) == ("wave" if wave else "workgroup") and mpw == (4 if wave else 1), line
            assert f["block"] == 256 and f["grid"] * mpw >= mazes > (f["grid"] - 1) * mpw, line
            threads = 256 // mpw
            assert rpl in (1, 2, 4) and rpl * threads >= RR and (rpl == 1 or (rpl // 2) * threads < RR), line
            assert f["lds"] == plan_lds(G, mpw), line
            assert f["lds"] <= 40 << 10, line                              # at least four workgroups per CU at any G
            forms.add((m.group(1), rpl))
    assert forms == {("wave", 1), ("wave", 2), ("wave", 4), ("workgroup", 1), ("workgroup", 2), ("workgroup", 4)}
    for G, want in ((5, "generate_kernel<wave, 1>"), (33, "generate_kernel<wave, 4>"), (34, "generate_kernel<workgroup, 1>"),
                    (64, "generate_kernel<workgroup, 4>")):
        assert abi.describe_generate(G, 7).startswith(want + " grid=%d block=256" % (2 if G <= 33 else 7))


# ------------------------------------------------------------- the Python entry
def test_mazes_argument_errors_need_no_device(abi):
    import torch
    L = importlib.import_module("gym-lmaze_amd.layouts")
    for G in (4, 3, 0, 65):
        with pytest.raises(ValueError, match="grid side"):
            L.mazes(4, G, "cuda")
    for loops in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="loops"):
            L.mazes(4, 11, "cuda", loops=loops)
    with pytest.raises(ValueError):
        L.mazes(4, 11, "cuda", maze_base=-1)
    for out in (torch.zeros((4, 11, 11), dtype=torch.uint8), torch.zeros((4, 11, 11), dtype=torch.int32), np.zeros((4, 11, 11), np.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            L.mazes(4, 11, "cuda", out=out)
    assert abi.epsilon_u32(0.25) == 1 << 30


# ------------------------------------------------------------- what the kernels need
@pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not installed")
def test_generate_kernels_use_no_scratch():
    usage = H.kernel_usage("lmaze_generate.hip")
    mine = {k: v for k, v in usage.items() if "generate_kernel" in k}
    assert len(mine) == 6, sorted(usage)                                   # 3 wave forms + 3 workgroup forms
    for name, v in mine.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["VGPRs"] <= 128, (name, v)                                # four waves per SIMD at the least
