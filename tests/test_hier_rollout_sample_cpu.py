"""CPU: the sampling closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_sample) without a GPU -- that the restatement's
cases take every path of the rule and show every action and (for the distributions) at least 20 goals, the selection text of
lmaze_hier_sample.h compiled for the host under the address and undefined-behaviour sanitizers against its numpy restatement,
thresholds made from weights sampled back, the two symbols and the header's statement of the rule, the launch the describe call
names on both sides of the 16 384-byte rule for both tables, every documented refusal in its order (answered before any device
call, on fabricated pointers), what the 12 new kernels need per wave, and the Python argument errors that need no device."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hier_sample_ref as R
from closed_loop_ref import fields as _fields
from closed_loop_ref import test_numpy_philox_is_the_oracles  # noqa: F401  (collected here: the restatement draws with philox)
from foveal_sample_ref import sample_action, thresholds, widths
from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_v5_rollout_sample", "lmaze_describe_v5_rollout_sample")
MAX_ENVS = 1 << 30
VID = {"v1": 1, "v2": 2, "v4": 4, "v5": 5, "v6": 6}


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


# ------------------------------------------------------------- the restatement's own parts
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_case_takes_every_path(shape):
    """The GPU module's coverage conditions, here where the seeds were chosen: with the oracle alone."""
    for ckey in R.CKEYS:
        for kind in R.KINDS:
            lays, lay, controller, planner, p, start, start_visit, out = R.case(shape, ckey, kind, R.SEEDS[shape])
            R.check_coverage(out.coverage, kind)
            L = lay.shape[0]
            assert controller.dtype == planner.dtype == np.uint32
            assert controller.shape == (R.controller_table_keys(ckey, shape.G, L), 4) and planner.shape == (L * shape.G ** 2, 24)
            assert out.rows["key"].min() >= 0 and out.rows["key"].max() < controller.shape[0]
            assert set(np.unique(out.rows["action"])) == {0, 1, 2, 3}
            planned = out.rows["goal_key"] >= 0
            assert (planned == (out.rows["goal"] >= 0)).all() and planned.any() and not planned.all()
            assert out.rows["goal_key"].max() < planner.shape[0] and out.rows["goal"].max() <= 24
            assert start["done"].any() and start["foveal_done"].any() and not (start["done"] | start["foveal_done"]).all()
            assert R.controller_side(shape, L, ckey) == ("lds" if ckey == "offset" else "global")
            assert R.planner_side(shape, L) == shape.planner
            if kind == "peaked":                                        # equal adjacent thresholds: actions of zero weight
                assert (widths(controller, 4) == 0).any() and (widths(planner, 25) == 0).any()
                assert (np.diff(planner.astype(np.int64), axis=1) >= 0).all()
            if kind == "raw":                                           # nothing is validated
                for t in (controller[:, :3], planner):
                    assert (np.diff(t.astype(np.int64), axis=1) < 0).any()
                    assert (t == 0).all(axis=1).any() and (t == 0xFFFFFFFF).all(axis=1).any()
                assert (controller[:, 3] != 0).any()                    # the reserved word: anything


# ------------------------------------------------------------- lmaze_hier_sample.h on the host
@pytest.fixture(scope="module")
def sample_host(tmp_path_factory):
    """tests/csrc/hier_sample_host.cpp: a stand-alone program around lmaze_hier_sample.h, built with the address and
    undefined-behaviour sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("hier_sample")
    exe = str(tmp / "hier_sample_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "csrc", "hier_sample_host.cpp")])

    def run(G, L, ck, controller, planner, ints, words):
        m = len(ints[0])
        src, dst = str(tmp / "in"), str(tmp / "out")
        with open(src, "wb") as fh:
            fh.write(np.array([m], np.int64).tobytes() + np.array([G, L, ck], np.int32).tobytes())
            fh.write(np.ascontiguousarray(controller, np.uint32).tobytes() + np.ascontiguousarray(planner, np.uint32).tobytes())
            for a in ints:
                fh.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
            for a in words:
                fh.write(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        return np.frombuffer(open(dst, "rb").read(), np.int32).reshape(4, m)
    return run


def _edge_rows(rs, S, W, A):
    """a table of S rows: a third the converter's monotone rows (entries of zero weight: equal thresholds), the rest unsorted
    random words; rows of 0, of 0xFFFFFFFF and of one repeated word among them"""
    t = rs.randint(0, 1 << 32, (S, W), dtype=np.uint64).astype(np.uint32)
    n = S // 3
    t[:n, :A - 1] = thresholds(rs.rand(n, A) ** 4 * (rs.rand(n, A) > 0.3) + 1e-12)[:, :A - 1]
    pick = rs.rand(S)
    t[pick < 0.04] = 0
    t[(pick >= 0.04) & (pick < 0.08)] = 0xFFFFFFFF
    same = (pick >= 0.08) & (pick < 0.12)
    t[same] = t[same, :1]
    return t


@pytest.mark.parametrize("G,L,ckey", [(18, 5, "offset"), (18, 5, "cell"), (12, 1, "offset"), (5, 1, "cell"), (64, 2, "offset"),
                                      (12, 2, "cell")])
def test_host_selection_text_is_the_numpy_one(sample_host, G, L, ckey):
    """Both row widths and both key modes: keys from states on and far off the grid and foveal goals at every offset (the tables
    are allocated exactly, the controller's even without its last reserved word: a key outside them or a fourth compare is the
    sanitizer's to report), rows that are monotone, unsorted, all 0, all 0xFFFFFFFF and all equal, draws at 0, 2^32 - 1, c_k - 1,
    c_k, c_k + 1 and random."""
    rs = np.random.RandomState(G * 100 + L + 7)
    imax, imin = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    edge = np.array([0, 1, -1, G - 1, G, G + 1, -G, 1 << 30, -(1 << 30), imax, imin], np.int64)
    m = 6000
    lid = np.where(rs.rand(m) < 0.3, rs.choice(np.array([-1, -7, L, L + 3, 1 << 20], np.int64), m), rs.randint(0, L, m))
    bx = np.where(rs.rand(m) < 0.3, rs.choice(edge, m), rs.randint(0, G, m))
    by = np.where(rs.rand(m) < 0.3, rs.choice(edge, m), rs.randint(0, G, m))
    fgx = np.where(rs.rand(m) < 0.2, rs.choice(edge, m), np.clip(bx + rs.randint(-6, 8, m), imin, imax))
    fgy = np.where(rs.rand(m) < 0.2, rs.choice(edge, m), np.clip(by + rs.randint(-6, 8, m), imin, imax))
    cells = L * G * G
    controller = _edge_rows(rs, R.controller_table_keys(ckey, G, L), 4, 4)
    planner = _edge_rows(rs, cells, 24, 25)
    ball, fg = np.stack([bx, by], axis=1), np.stack([fgx, fgy], axis=1)
    want_kp = R.planner_keys(G, L, np.clip(lid, imin, imax), np.clip(ball, 0, G - 1))     # int64 in, as the rule clamps
    d, raw = R.controller_keys("offset", G, L, lid, ball, fg)           # the offset is taken from the ball as it is
    want_kc = (want_kp.astype(np.int64) * 100 + d).astype(np.int32) if ckey == "cell" else d

    def draws(rows, n):
        c = rows[np.arange(m), rs.randint(0, n, m)].astype(np.int64)
        pick = rs.randint(0, 6, m)
        return np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4],
                         [np.zeros(m, np.int64), np.full(m, (1 << 32) - 1), np.clip(c - 1, 0, None), c, np.clip(c + 1, None, (1 << 32) - 1)],
                         rs.randint(0, 1 << 32, m, dtype=np.uint64).astype(np.int64)).astype(np.uint64)
    rz, rx = draws(planner[want_kp], 24), draws(controller[want_kc], 3)
    kp, kc, goal, action = sample_host(G, L, R.CKEYS.index(ckey), controller.reshape(-1), planner, (lid, bx, by, fgx, fgy), (rx, rz))
    assert (kp == want_kp).all() and kp.min() >= 0 and kp.max() < cells
    assert (kc == want_kc).all() and kc.min() >= 0 and kc.max() < controller.shape[0]
    assert ((raw < 0) | (raw > 9)).any() and not ((raw < 0) | (raw > 9)).all()
    want_goal, want_action = sample_action(planner[want_kp], rz, 24), sample_action(controller[want_kc], rx, 3)
    assert (goal == want_goal).all() and (action == want_action).all()
    assert set(np.unique(goal)) == set(range(25)) and set(np.unique(action)) == set(range(4))
    # the unsorted rows pin the sum: a search for the first threshold above the draw gives another goal for many of them
    first_above = np.array([int(np.argmax(np.append(planner[want_kp[i]].astype(np.uint64) > rz[i], True))) for i in range(m)])
    assert (first_above != want_goal).any()
    # the reserved word is never compared: 4 would show where it is 0
    assert (controller[want_kc, 3] == 0).any() and action.max() == 3


# ------------------------------------------------------------- thresholds from weights
def test_thresholds_from_weights_sample_back_the_weights(abi):
    """sampling_thresholds(probs, actions=25) -> 2^20 numpy uint32 draws through the rule reproduce the weights within binomial
    error (6 sigma of the count, at least 6 counts), and an action of zero weight is never drawn."""
    rs = np.random.RandomState(5)
    p = rs.rand(6, 25) ** 3
    p[1, rs.rand(25) < 0.4] = 0.0
    p[2] = 0.0
    p[2, [3, 24]] = (1.0, 3.0)
    p[3] = 1.0
    p[4, :5] = 0.0                                                      # leading zeros
    p[5, 20:] = 0.0                                                     # trailing zeros
    table = abi.sampling_thresholds(torch.from_numpy(p), actions=25)
    assert table.dtype == torch.uint32 and tuple(table.shape) == (6, 24)
    table = table.view(torch.int32).numpy().view(np.uint32)
    assert (table == thresholds(p)).all()
    n = 1 << 20
    r = rs.randint(0, 1 << 32, n, dtype=np.uint64)
    for row in range(6):
        got = np.bincount(sample_action(np.broadcast_to(table[row], (n, 24)), r, 24), minlength=25)
        q = p[row] / p[row].sum()
        sigma = np.sqrt(n * q * (1 - q))
        assert (np.abs(got - n * q) <= np.maximum(6 * sigma, 6) * (q > 0)).all(), (row, got, n * q)
        assert (got[q == 0] == 0).all(), (row, got)
    ctl = abi.sampling_thresholds(torch.from_numpy(p[:, :4] + np.array([0, 0, 1e-3, 0])), actions=4)
    assert tuple(ctl.shape) == (6, 4) and bool((ctl.view(torch.int32)[:, 3] == 0).all())


# ------------------------------------------------------------- the C ABI
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in NAMES:
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    env = importlib.import_module("gym-lmaze_amd").LmazeFovealVecEnv
    assert callable(env.rollout_hier_sample) and callable(abi.describe_v5_rollout_sample)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("drawn on every env-step", "only r.x and r.z are used", "sum over k < 24 of (r.z >= planner_thresholds[kp][k])",
                   "sum over k < 3 of (r.x >= controller_thresholds[kc][k])", "no plannerStep is ever skipped", "both are -1",
                   "at most 16 384 bytes", "binary search is not equivalent", "controller=lds|global planner=lds|global",
                   "a table that is not 16-byte aligned is LMAZE_E_ALIGN", "keep refusing v5/v6", "The caller advances its epoch by T."):
        assert phrase in flat, phrase
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "lmaze_hier_sample.hip" in makefile and "lmaze_hier_sample.h" in makefile


def test_header_compiles_as_c99_with_a_caller_of_the_new_entries(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include "lmaze.h"\n'
                   'int main(void){ LmazeFovealParams f = {0}; char text[8];\n'
                   '  int (*run)(const LmazeFovealParams*, const uint8_t*, const uint32_t*, int32_t, const uint32_t*, int32_t,\n'
                   '             const LmazeFovealBuffers*, int64_t, uint64_t, uint64_t, int64_t, float*, uint8_t*, float*, uint8_t*,\n'
                   '             int32_t*, int32_t*, int32_t*, int32_t*, float*, float*, int32_t, void*) = lmaze_v5_rollout_sample;\n'
                   '  int (*say)(const LmazeFovealParams*, int64_t, int32_t, int32_t, int32_t, char*, int32_t) = lmaze_describe_v5_rollout_sample;\n'
                   '  (void)f; (void)text; return run != 0 && say != 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "probe.o")])


def _params(abi, variant="v5", G=18, L=5, hint=0):
    return abi.LmazeFovealParams(VID.get(variant, variant), G, L, 10, 50, -1.0, -0.01, 100.0, hint)


BUFS = ("ball_xy", "goal_xy", "fgoal_xy", "layout_id", "step_count", "foveal_step_count", "reward", "foveal_reward", "done",
        "foveal_done", "visit", "obs", "ball1_xy", "fovea_xy", "last_xy", "foveal_goal", "obs_local", "visit_clock")


def _call(abi, variant="v5", G=18, L=5, hint=0, params=True, layouts=64, controller=64, ck=0, planner=128, T=6, bufs=True, n=100,
          obs_t=None, obs_local_t=None, every=0, **bkw):
    """fabricated device addresses: nothing is dereferenced before the refusals"""
    p = _params(abi, variant, G, L, hint)
    ptrs = {name: 4096 for name in BUFS}
    ptrs.update(bkw)
    b = abi.LmazeFovealBuffers(**ptrs)
    return abi.lib.lmaze_v5_rollout_sample(C.byref(p) if params else None, layouts, controller, ck, planner, T,
                                           C.byref(b) if bufs else None, n, 1, 0, 0, None, None, None, None, None, None, None, None,
                                           obs_t, obs_local_t, every, None)


@pytest.mark.parametrize("variant", ["v5", "v6"])
def test_refusals_in_their_documented_order(abi, variant):
    kw = dict(variant=variant)
    # 1. the recording request, before anything else -- even NULL params, another variant or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_local_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=4096, obs_local_t=4096 + 8, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, params=False, n=-1, **kw) == E_NULL
    assert _call(abi, every=-1, params=False, controller=None, T=-1, **kw) == E_COUNT
    assert _call(abi, variant="v2", obs_t=4096 + 8, every=1) == E_ALIGN
    # 2. the params' own, before the variant's refusal and the counts
    assert _call(abi, params=False, T=-1, **kw) == E_NULL
    assert _call(abi, variant=3, T=-1) == E_VARIANT
    assert _call(abi, variant=0, n=-1) == E_VARIANT
    assert _call(abi, G=4, T=-1, **kw) == E_GRID
    assert _call(abi, G=65, n=-1, **kw) == E_GRID
    assert _call(abi, variant="v2", G=4) == E_GRID                        # before 3.
    assert _call(abi, L=0, T=-1, **kw) == E_LAYOUT
    assert _call(abi, L=17, planner=None, **kw) == E_LAYOUT
    assert _call(abi, hint=0x400, T=-1, **kw) == E_LAYOUT
    # 3. anything but v5/v6, before the counts and before "nothing to do"
    for other in ("v1", "v2", "v4"):
        L = 1 if other == "v1" else 5
        assert _call(abi, variant=other, L=L) == E_VARIANT
        assert _call(abi, variant=other, L=L, T=-1, n=-1, ck=7) == E_VARIANT
        assert _call(abi, variant=other, L=L, T=0) == E_VARIANT
        assert _call(abi, variant=other, L=L, n=0, controller=None, planner=None, layouts=None, bufs=False) == E_VARIANT
    # 4. the counts, controller_key among them, before "nothing to do" and before the pointers
    assert _call(abi, T=-1, **kw) == E_COUNT
    assert _call(abi, n=-1, **kw) == E_COUNT
    assert _call(abi, n=MAX_ENVS + 1, **kw) == E_COUNT
    assert _call(abi, T=-1, n=0, **kw) == E_COUNT
    for ck in (-1, 2, 100):
        assert _call(abi, ck=ck, **kw) == E_COUNT
        assert _call(abi, ck=ck, T=0, **kw) == E_COUNT
        assert _call(abi, ck=ck, n=0, controller=None, planner=None, layouts=None, bufs=False, **kw) == E_COUNT
    # 5. nothing to do: 0 whatever the pointers, odd and misaligned ones included
    for T, n in ((0, 100), (6, 0), (0, 0), (0, MAX_ENVS)):
        for ck in (0, 1):
            assert _call(abi, T=T, n=n, ck=ck, controller=None, planner=None, layouts=None, bufs=False, **kw) == 0
            assert _call(abi, T=T, n=n, ck=ck, controller=65, planner=67, obs=4096 + 4, **kw) == 0
            assert _call(abi, T=T, n=n, ck=ck, planner=None, obs_t=4096, every=4, **kw) == 0
    assert _call(abi, T=2, n=0, obs_t=None, every=3, **kw) == 0           # T / every == 0: no slot wanted, obs_t may be NULL
    # 6. the pointers, both tables among them; then alignment, the tables' last
    assert _call(abi, controller=None, **kw) == E_NULL
    assert _call(abi, planner=None, **kw) == E_NULL
    assert _call(abi, layouts=None, **kw) == E_NULL
    assert _call(abi, bufs=False, **kw) == E_NULL
    for name in BUFS:
        assert _call(abi, **dict(kw, **{name: None})) == E_NULL, name
    assert _call(abi, planner=None, obs=4096 + 4, **kw) == E_NULL         # NULL before alignment
    assert _call(abi, controller=None, planner=64 + 4, **kw) == E_NULL    # a missing table before a misaligned one
    assert _call(abi, controller=64 + 8, ball_xy=None, **kw) == E_NULL    # the tables' alignment after every pointer
    assert _call(abi, obs=4096 + 4, **kw) == E_ALIGN
    assert _call(abi, obs_local=4096 + 4, **kw) == E_ALIGN
    assert _call(abi, visit=4096 + 32, **kw) == E_ALIGN
    for off in (1, 4, 8, 12):
        assert _call(abi, controller=64 + off, **kw) == E_ALIGN
        assert _call(abi, planner=128 + off, **kw) == E_ALIGN


def _foveal_lds(G, L, epb):
    """lmaze_foveal_defs.h foveal_lds for v5/v6: per-env strings and flags, row masks, layout characters, visit samples"""
    return epb * 64 + (3 * L * G + 2 * G) * 8 + ((L * G * G + 15) & ~15) + epb * (2 * 25 * 4 + 8)


DESCRIBED = [("v5", 18, 5), ("v6", 18, 5), ("v5", 12, 1), ("v5", 12, 2), ("v5", 13, 1), ("v5", 14, 1), ("v5", 5, 3), ("v5", 64, 2)]


@pytest.mark.parametrize("variant,G,L", DESCRIBED)
def test_describe_names_the_kernel_and_where_the_tables_live(abi, variant, G, L):
    """Each table of at most 16 384 bytes: staged in LDS on the next 16-byte boundary behind the layout characters and counted in
    the launch's LDS; above: global, no extra LDS.  A rule, whatever n, T, the recording and the hint; any grid runs at any envs
    per workgroup.  13 x 13 (16 224 B of planner table) and 14 x 14 (18 816 B) pin the boundary."""
    cells = L * G * G
    for ckey in R.CKEYS:
        cbytes, pbytes = 16 * R.controller_table_keys(ckey, G, L), 96 * cells
        sides = ("lds" if cbytes <= 16384 else "global", "lds" if pbytes <= 16384 else "global")
        assert sides[0] == ("lds" if ckey == "offset" else "global")
        staged = sum(b for b, s in zip((cbytes, pbytes), sides) if s == "lds")
        for n, hint, epb in ((333, 0, 32), (333, 0x30, 64), (333, 0x40, 128), (333, 0x120, 32), (40000, 0, 64), (1 << 20, 0x20, 32)):
            for every in (0, 1, 5):
                line = abi.describe_v5_rollout_sample(_params(abi, variant, G, L, hint), n, 24, ckey, every)
                f = _fields(line)
                base = _foveal_lds(G, L, f["envs_per_workgroup"])
                want = ((base + 15) & ~15) + staged if staged else base
                if ((_foveal_lds(G, L, epb) + 15) & ~15) + staged <= 64 << 10:   # the launcher assumes 64 KiB without a device
                    assert f["envs_per_workgroup"] == epb, line
                assert line.startswith("foveal_hier_sample_kernel<v5, %d, %d%s> controller=%s planner=%s T=24 grid="
                                       % (f["envs_per_workgroup"], G if G == 18 else 0, ", obs_t" if every else "", *sides)), line
                assert f["lds"] == want and f["block"] == 256, (line, want)
                chunks = ((hint >> 8) & 3) + 1
                assert f["chunks"] == chunks and f["grid"] == -(-(-(-n // f["envs_per_workgroup"])) // chunks), line
    # bits 0-3: the cap pads the LDS and is reported
    f = _fields(abi.describe_v5_rollout_sample(_params(abi, variant, G, L, 0x25), 333, 24, "offset", 0))
    assert f["workgroups_per_cu"] in (0, 5) and f["lds"] >= _foveal_lds(G, L, 32)


def test_the_boundary_and_the_shapes_of_the_gpu_test(abi):
    assert " planner=lds " in abi.describe_v5_rollout_sample(_params(abi, "v5", 13, 1), 333, 24, "offset", 0)
    assert " planner=global " in abi.describe_v5_rollout_sample(_params(abi, "v5", 14, 1), 333, 24, "offset", 0)
    assert (5, 3) in [(G, L) for _, G, L in DESCRIBED] and _foveal_lds(5, 3, 32) % 16 == 8   # a sum the staged rows must round up
    for shape in R.SHAPES:
        L = shape.L or 5
        assert R.planner_side(shape, L) == shape.planner
        for ckey in R.CKEYS:
            line = abi.describe_v5_rollout_sample(_params(abi, shape.variant, shape.G, L), R.N, R.T, ckey, 0)
            assert " controller=%s planner=%s " % (R.controller_side(shape, L, ckey), shape.planner) in line, line
            assert line.startswith("foveal_hier_sample_kernel<v5, 32, %d> " % (18 if shape.G == 18 else 0)), line


def test_describe_refusals_and_empty_lines(abi):
    d = abi.lib.lmaze_describe_v5_rollout_sample
    buf = C.create_string_buffer(256)
    p = _params(abi)
    assert d(C.byref(p), 100, 6, 0, 0, None, 256) == E_NULL
    assert d(C.byref(p), 100, 6, 0, 0, buf, 0) == E_NULL
    assert d(None, -1, -1, 5, -1, None, 256) == E_NULL                  # the text first
    assert d(C.byref(p), 100, 6, 0, -1, buf, 256) == E_COUNT
    assert d(None, 100, 6, 0, -1, buf, 256) == E_COUNT                  # the recording request before the params
    assert d(None, 100, 6, 0, 0, buf, 256) == E_NULL
    assert d(C.byref(_params(abi, 3)), 100, -1, 0, 0, buf, 256) == E_VARIANT
    assert d(C.byref(_params(abi, "v5", 4)), 100, -1, 0, 0, buf, 256) == E_GRID
    assert d(C.byref(_params(abi, "v5", 18, 17)), 100, -1, 0, 0, buf, 256) == E_LAYOUT
    for other, L in (("v1", 1), ("v2", 5), ("v4", 5)):
        assert d(C.byref(_params(abi, other, 18, L)), 100, 6, 0, 0, buf, 256) == E_VARIANT
        assert d(C.byref(_params(abi, other, 18, L)), 0, -1, 2, 3, buf, 256) == E_VARIANT
    assert d(C.byref(p), 100, -1, 0, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), -1, 6, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), MAX_ENVS + 1, 6, 0, 3, buf, 256) == E_COUNT
    for ck in (-1, 2):
        assert d(C.byref(p), 100, 6, ck, 0, buf, 256) == E_COUNT
        assert d(C.byref(p), 0, 6, ck, 0, buf, 256) == E_COUNT          # before "nothing to do"
    buf.value = b"stale"
    assert d(C.byref(p), 0, 6, 0, 0, buf, 256) == 0 and buf.value == b""
    buf.value = b"stale"
    assert d(C.byref(p), 100, 0, 1, 3, buf, 256) == 0 and buf.value == b""
    assert d(C.byref(p), 100, 6, 0, 0, buf, 8) == 0 and buf.value == b"foveal_"      # truncated to len, always terminated
    assert abi.describe_v5_rollout_sample(p, 333, 24, "offset", 5).startswith(
        "foveal_hier_sample_kernel<v5, 32, 18, obs_t> controller=lds planner=global T=24 grid=")
    # the siblings keep refusing v5/v6, and the epsilon-greedy twin keeps its own line
    for name in ("lmaze_describe_foveal_rollout_policy", "lmaze_describe_foveal_rollout_sample"):
        assert getattr(abi.lib, name)(C.byref(p), 100, 6, 1, 0, buf, 256) == E_VARIANT
    assert abi.describe_v5_rollout_policy(p, 333, 24, "offset", 0).startswith("foveal_hier_policy_kernel<v5, 32, 18> controller=lds planner=lds ")


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_no_scratch_and_at_least_three_waves():
    """12 kernels (v5 x 32 / 64 / 128 envs x G = 18 / any x row or recording form), none with scratch, none below 3 waves per
    SIMD -- the epsilon-greedy twin's own occupancy, which its row form at 32 envs and G = 18 still meets without scratch."""
    new = kernel_usage("lmaze_hier_sample.hip")
    pat = re.compile(r"_ZN5lmaze25foveal_hier_sample_kernelILi5ELi(32|64|128)ELi(18|0)ELb1EEEvNS_10FovealArgsENS_"
                     r"(17FovealRollHierSmp|20FovealRollObsHierSmp)E")
    assert len(new) == 12, sorted(new)
    seen = set()
    for name, v in new.items():
        m = pat.fullmatch(name)
        assert m, name
        seen.add(m.groups())
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["Occupancy"] >= 3, (name, v)
    assert len(seen) == 12
    twin = kernel_usage("lmaze_hier_policy.hip")["_ZN5lmaze25foveal_hier_policy_kernelILi5ELi32ELi18ELb1EEEvNS_10FovealArgsENS_14FovealRollHierE"]
    assert twin.get("ScratchSize", 0) == 0 and twin["Occupancy"] >= 3


# ------------------------------------------------------------- the Python surface without a device
def test_python_argument_errors_that_need_no_device(abi, monkeypatch):
    """What rollout_hier_sample() refuses before it touches the device, on an env object that never saw one (its tensors are
    the host's)."""
    pkg = importlib.import_module("gym-lmaze_amd")
    env = object.__new__(pkg.LmazeFovealVecEnv)
    env.variant, env._two_level, env.num_envs, env.grid, env.n_layouts = "v5", True, 8, 5, 1
    env.device = torch.device("cpu")
    cp, pp = torch.ones(100, 4), torch.ones(25, 25)
    ct, pt = abi.sampling_thresholds(cp), abi.sampling_thresholds(pp, actions=25)
    ok = dict(controller_thresholds=ct, planner_thresholds=pt)
    # torch's capture query needs a device; it is answered here, "no", for everything but the first check
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    with monkeypatch.context() as m:                                    # under stream capture, before the tables are looked at
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="stream capture"):
            env.rollout_hier_sample(4, controller_probs=object(), planner_probs=object())
    for T in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="T must be an int"):
            env.rollout_hier_sample(T, **ok)
    # zero or two sources per level
    for kw in (dict(), dict(controller_probs=cp), dict(planner_probs=pp), dict(ok, controller_probs=cp), dict(ok, planner_logits=pp),
               dict(controller_probs=cp, controller_logits=cp, planner_probs=pp),
               dict(controller_probs=cp, planner_probs=pp, planner_logits=pp, planner_thresholds=pt)):
        with pytest.raises(ValueError, match="exactly one of"):
            env.rollout_hier_sample(4, **kw)
    for bad in ("goal", 2, -1):
        with pytest.raises(ValueError, match="controller_key"):
            env.rollout_hier_sample(4, controller_key=bad, **ok)
    # shapes: the other level's width, a row short, the other key mode's table
    for kw in (dict(ok, controller_thresholds=None, controller_probs=torch.ones(100, 25)), dict(ok, planner_thresholds=None, planner_probs=torch.ones(25, 4)),
               dict(ok, controller_thresholds=None, controller_probs=torch.ones(99, 4)), dict(ok, planner_thresholds=None, planner_logits=torch.ones(24, 25)),
               dict(ok, controller_thresholds=None, controller_logits=torch.ones(4)), dict(ok, controller_key="cell"),
               dict(ok, controller_thresholds=ct.view(torch.int32)[:, :3].contiguous()), dict(ok, planner_thresholds=abi.sampling_thresholds(torch.ones(25, 26), actions=26)),
               dict(ok, planner_thresholds=pt.view(torch.int32)[:24])):
        with pytest.raises(ValueError, match=r"must be a .*tensor \["):
            env.rollout_hier_sample(4, **kw)
    # dtype: thresholds that are not 32-bit words, weights that are not floats
    for kw in (dict(ok, controller_thresholds=ct.view(torch.int32).to(torch.int64)), dict(ok, planner_thresholds=pt.view(torch.int32).float()),
               dict(ok, controller_thresholds=None, controller_probs=torch.ones(100, 4, dtype=torch.int32)),
               dict(ok, planner_thresholds=None, planner_logits=torch.ones(25, 25, dtype=torch.int64))):
        with pytest.raises(ValueError, match=r"must be a .*tensor \["):
            env.rollout_hier_sample(4, **kw)
    # alignment and contiguity
    flat = torch.zeros(100 * 4 + 1, dtype=torch.int32)
    assert flat.data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="16-byte aligned"):
        env.rollout_hier_sample(4, **dict(ok, controller_thresholds=flat[1:].view(100, 4)))
    with pytest.raises(ValueError, match="contiguous"):
        env.rollout_hier_sample(4, **dict(ok, planner_thresholds=torch.zeros(25, 48, dtype=torch.int32)[:, ::2]))
    # temperature
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            env.rollout_hier_sample(4, controller_logits=cp, planner_thresholds=pt, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            env.rollout_hier_sample(4, controller_thresholds=ct, planner_logits=pp, planner_temperature=bad)
        with pytest.raises(ValueError, match="temperature"):                 # the planner's defaults to temperature
            env.rollout_hier_sample(4, controller_thresholds=ct, planner_logits=pp, temperature=bad)
    # obs_t / obs_local_t without obs_every
    for kw in (dict(obs_t=torch.zeros(1)), dict(obs_local_t=torch.zeros(1))):
        with pytest.raises(ValueError, match="need obs_every"):
            env.rollout_hier_sample(4, **dict(ok, **kw))
    for variant in ("v1", "v2", "v4"):
        env.variant, env._two_level = variant, False
        with pytest.raises(ValueError, match="v5/v6"):
            env.rollout_hier_sample(4, **ok)
    env.variant, env._two_level = "v5", True
    with pytest.raises(ValueError, match="v5/v6"):                       # rollout_sample() stays as it is
        env.rollout_sample(4, probs=pp)
