"""CPU: the closed-loop rollouts with a table per env (include/lmaze.h lmaze_env_rollout_policy / lmaze_env_rollout_sample /
lmaze_describe_env_rollout) without a GPU -- the symbols, every documented refusal in its order of precedence (answered
before any device call), the new LDS kind of csrc/lmaze_rollout_lds.h written whole under the sanitizers, the launch the
describe call names, and what the eight new kernel forms need per wave."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import pytest

from closed_loop_ref import fields as _fields, grid_params as _params, perenv_lds as _perenv_lds, shared_lds as _shared_lds
from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_env_rollout_policy", "lmaze_env_rollout_sample", "lmaze_describe_env_rollout")
ENV_BYTES = 4                                     # LMAZE_TAB_ENV_BYTES
PER_ENV_EPB = (4, 8, 16, 32, 64)


def _up16(x):
    return (x + 15) & ~15


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in NAMES:
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
        # the sweep of tests/test_rollout_entries_cpu.py over the grid rollout entries goes by these prefixes
        assert not name.startswith(("lmaze_rollout", "lmaze_describe_rollout"))
    assert abi.lib.lmaze_abi_version() == 4
    assert C.sizeof(abi.LmazeParams) == 32
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("i G^2 + c", "LOCAL index", "n G^2 > INT32_MAX", "4-byte aligned", "policy=env, table=lds", "sample=env, table=global",
                   "stale after it", "v0:146-237", "v3:220-402", "v0:64-110"):
        assert phrase in flat, phrase
    pkg = importlib.import_module("gym-lmaze_amd")
    assert "key=\"env\"" in pkg.LmazeVecEnv.rollout_policy.__doc__ and "key=\"env\"" in pkg.LmazeVecEnv.rollout_sample.__doc__


def _call(abi, form, variant="v0", G=11, mode=None, T=6, n=100, table=64, obs_t=None, every=0, params=True, layout=64, ball=64,
          goal=None, obs=None, key_t=None):
    """Fabricated device addresses: every refusal is returned before anything is dereferenced or queued."""
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else (abi.VARIANT_V0 if variant == "v0" else variant), G,
                        abi.LAYOUT_PER_ENV if mode is None else mode, 100, -1.0, -0.01, 100.0)
    head = (C.byref(p) if params else None, layout, table)
    tail = (T, ball, goal, 64, 64, 64, None, obs, None, None, None, key_t, n, 1, 1, 0, 0, obs_t, every, None)
    if form == "policy":
        return abi.lib.lmaze_env_rollout_policy(*head, 0, *tail)
    return abi.lib.lmaze_env_rollout_sample(*head, *tail)


@pytest.mark.parametrize("form", ["policy", "sample"])
def test_refusals_in_order_of_precedence(abi, form):
    """lmaze_rollout_policy's refusals in its order; in the key mode's place the int32 row count; the table's alignment (4
    bytes for the byte tables, 16 for the thresholds) among the alignment refusals."""
    kw = dict(form=form)
    G64_OVER, G64_FITS = 1 << 19, (1 << 19) - 1          # n * 64 * 64 = 2^31, and the largest n below it
    # 1. the recording request, before anything else -- even NULL params or a bad count
    assert _call(abi, every=-1, **kw) == E_COUNT
    assert _call(abi, obs_t=4096, every=0, **kw) == E_COUNT
    assert _call(abi, obs_t=None, every=3, **kw) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3, **kw) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, n=-1, params=False, **kw) == E_NULL
    assert _call(abi, every=-1, table=None, G=64, n=G64_OVER, **kw) == E_COUNT
    # 2. params, variant, T -- before the row count
    assert _call(abi, params=False, **kw) == E_NULL
    assert _call(abi, G=2, n=1 << 30, **kw) == E_GRID
    assert _call(abi, G=65, n=1 << 30, **kw) == E_GRID
    assert _call(abi, mode=5, G=64, n=G64_OVER, **kw) == E_LAYOUT
    assert _call(abi, n=-1, **kw) == E_COUNT
    assert _call(abi, variant=2, G=64, n=G64_OVER, **kw) == E_VARIANT
    assert _call(abi, T=-1, **kw) == E_COUNT
    # 3. n * G^2 > INT32_MAX: with or without key_t, before "nothing to do" and before the pointers, both layout modes
    for mode in (abi.LAYOUT_PER_ENV, abi.LAYOUT_SHARED):
        for variant, goal in (("v0", None), ("v3", 64)):
            m = dict(kw, mode=mode, variant=variant, goal=goal)
            assert _call(abi, G=64, n=G64_OVER, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, key_t=64, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, T=0, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, table=None, layout=None, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, table=64 + 1, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_FITS, table=None, **m) == E_NULL           # the largest batch passes on to the pointers
            assert _call(abi, G=64, n=G64_FITS, T=0, table=None, **m) == 0
    assert 121 * 17747798 <= 2 ** 31 - 1 < 121 * 17747799
    assert _call(abi, G=11, n=17747799, **kw) == E_COUNT
    assert _call(abi, G=11, n=17747798, table=None, **kw) == E_NULL
    assert _call(abi, G=3, n=1 << 30, **kw) == E_COUNT
    # 4. pointers: the table among them; then alignment, the table's own among them
    assert _call(abi, table=None, **kw) == E_NULL
    assert _call(abi, variant="v3", goal=None, **kw) == E_NULL
    assert _call(abi, layout=None, **kw) == E_NULL
    assert _call(abi, table=None, ball=68, **kw) == E_NULL              # NULL before alignment
    assert _call(abi, layout=None, table=64 + 1, **kw) == E_NULL
    assert _call(abi, ball=68, **kw) == E_ALIGN
    assert _call(abi, obs=4096 + 8, **kw) == E_ALIGN
    assert _call(abi, layout=72, **kw) == E_ALIGN
    for mode in (abi.LAYOUT_PER_ENV, abi.LAYOUT_SHARED):
        for off in (1, 2, 3) if form == "policy" else (4, 8, 12):
            assert _call(abi, table=4096 + off, mode=mode, **kw) == E_ALIGN
            assert _call(abi, variant="v3", goal=64, table=4096 + off, mode=mode, **kw) == E_ALIGN


@pytest.mark.parametrize("form", ["policy", "sample"])
@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("T,n", [(0, 100), (6, 0), (0, 0)])
def test_nothing_to_do_reads_no_pointer_and_no_alignment(abi, form, variant, T, n):
    assert _call(abi, form, variant=variant, T=T, n=n, table=None, layout=None, ball=None) == 0
    assert _call(abi, form, variant=variant, T=T, n=n, table=4096 + 1, layout=72, ball=68, obs=4096 + 8) == 0
    assert _call(abi, form, variant=variant, T=T, n=n, table=None, every=3 if T < 3 else 7) == 0       # T / k == 0 slots
    assert _call(abi, form, variant=variant, T=-1, n=n, table=None) == E_COUNT


# ------------------------------------------------------------- the new LDS kind under the sanitizers
@pytest.fixture(scope="module")
def env_layouts(tmp_path_factory):
    """{(G, epb): (total, [(array, offset, bytes), ...])} as tests/csrc/rollout_lds_env_host.cpp printed them.  It is built
    with the sanitizers and run as a program (never loaded into this process): any report fails the run."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("rollout_lds_env") / "rollout_lds_env_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "csrc", "rollout_lds_env_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert lines[-1].startswith("read_back ")
    cases = {}
    for line in lines[:-1]:
        w = line.split()
        assert w[0] == "perenv" and int(w[3]) == ENV_BYTES
        cases[(int(w[1]), int(w[2]))] = (int(w[4]), [(w[i], int(w[i + 1]), int(w[i + 2])) for i in range(5, len(w), 3)])
    return cases


def test_the_staged_tables_lie_behind_the_layouts(env_layouts):
    """Every G and envs per workgroup; ballflat, goalflat, lay and tab written whole (lay and tab twice: by dwords and by
    bytes, one extent each), pairwise disjoint, inside exactly `total` bytes; tab on a 16-byte boundary, the size of the
    layouts; the total is the layouts' own sum rounded up to 16 plus the tables rounded up to 16."""
    assert set(env_layouts) == {(G, epb) for G in range(3, 65) for epb in PER_ENV_EPB}
    for (G, epb), (total, arrays) in env_layouts.items():
        assert {a[0] for a in arrays} == {"ballflat", "goalflat", "lay", "tab"}
        extent = {}
        for name, off, size in arrays:
            lo, hi = extent.get(name, (off, off + size))
            assert lo == off, (G, epb, name)
            extent[name] = (lo, max(hi, off + size))
        spans = sorted(extent.values())
        assert spans[0][0] == 0 and spans[-1][1] <= total, (G, epb, spans, total)
        for (_, hi), (lo, _) in zip(spans, spans[1:]):
            assert hi <= lo, (G, epb, spans)
        lo, hi = extent["tab"]
        assert lo % 16 == 0 and hi - lo == epb * G * G and lo >= extent["lay"][1], (G, epb, extent)
        assert lo == _up16(_perenv_lds(G, epb)), (G, epb, lo)
        assert total == _up16(_perenv_lds(G, epb)) + _up16(epb * G * G), (G, epb, total)


# ------------------------------------------------------------- describe lines
def _total(abi, mode, form, G, epb):
    """The header's total for the body and table kind of the form"""
    if mode == abi.LAYOUT_PER_ENV:
        return _up16(_perenv_lds(G, epb)) + (_up16(epb * G * G) if form == "policy" else 0)
    return _up16(_shared_lds(G, epb))


@pytest.mark.parametrize("form", ["policy", "sample"])
@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("per_env", [True, False])
def test_describe_lines(abi, env_layouts, form, variant, per_env):
    """The name says the kernel, the form and where the table is read; lds is the header's total for the envs per workgroup
    the same line names and never above 160 KiB; the envs per workgroup are a multiple of 4 and those of the ball-keyed
    sibling, halved only where the staged tables would not fit; launch_hint bit 8 is not read."""
    mode = abi.LAYOUT_PER_ENV if per_env else abi.LAYOUT_SHARED
    kernel = "rollout_perenv_kernel" if per_env else "rollout_shared_kernel"
    where = "lds" if per_env and form == "policy" else "global"
    sibling = abi.describe_rollout_policy if form == "policy" else abi.describe_rollout_sample
    clamped = 0
    for G in (8, 11, 18, 32, 64):
        for n in (777, 16384, 65536):
            for k in range(8):
                for T, every in ((16, 3), (16, 0), (1, 0)):
                    p = _params(abi, variant, G, mode, k << 12)
                    line = abi.describe_env_rollout(p, n, T, obs_every=every, form=form)
                    head = "%s<v%s, %s=env, table=%s%s> T=%d every=%d " % (kernel, variant[1], form, where, ", obs_t" if every else "", T, every)
                    assert line.startswith(head), line
                    f = _fields(line)
                    epb = f["envs_per_workgroup"]
                    assert epb % 4 == 0 and epb >= 4 and f["grid"] == -(-n // epb) and f["block"] == 256, line
                    assert f["lds"] == _total(abi, mode, form, G, epb) <= 160 << 10, line
                    if where == "lds":
                        assert f["lds"] == env_layouts[(G, epb)][0], line
                    base = _fields(sibling(p, n, T, obs_every=every, key="ball"))["envs_per_workgroup"]
                    if epb != base:
                        assert where == "lds" and epb < base and _total(abi, mode, form, G, 2 * epb) > 160 << 10, (line, base)
                        clamped += 1
                    assert abi.describe_env_rollout(_params(abi, variant, G, mode, (k << 12) | 0x100), n, T, obs_every=every,
                                                    form=form) == line                      # bit 8: no T-launch fallback
    assert (clamped > 0) == (where == "lds")          # G = 64 hinted to 32 or 64 envs: 2 x 128 KiB does not fit
    p = _params(abi, variant, 11, mode, 1 << 15)
    assert ", obs_t, nt> " in abi.describe_env_rollout(p, 4099, 8, obs_every=2, form=form)
    assert ", nt" not in abi.describe_env_rollout(p, 4099, 8, obs_every=0, form=form)
    assert "obs_t" not in abi.describe_env_rollout(p, 4099, 8, with_obs=False, form=form)


def test_describe_refusals_and_empty_lines(abi):
    p = _params(abi, "v0", 11, abi.LAYOUT_PER_ENV)
    buf = C.create_string_buffer(256)
    d = abi.lib.lmaze_describe_env_rollout
    assert d(C.byref(p), 100, 6, 1, 1, -1, 0, buf, 256) == E_COUNT
    assert d(C.byref(p), 100, 6, 1, 2, 0, 0, buf, 256) == E_COUNT        # no narrow planes
    for form in (-1, 2, 7):
        assert d(C.byref(p), 100, 6, 1, 1, 0, form, buf, 256) == E_COUNT
        assert d(None, 100, 6, 1, 1, 0, form, None, 256) == E_COUNT
    for form in (0, 1):
        assert d(C.byref(p), 100, 6, 1, 1, 0, form, None, 256) == E_NULL
        assert d(None, 100, 6, 1, 1, 0, form, buf, 256) == E_NULL
        assert d(C.byref(p), 100, -1, 1, 1, 0, form, buf, 256) == E_COUNT
        assert d(C.byref(_params(abi, "v0", 64, abi.LAYOUT_PER_ENV)), 1 << 19, 6, 1, 1, 0, form, buf, 256) == E_COUNT
        assert d(C.byref(_params(abi, "v0", 64, abi.LAYOUT_PER_ENV)), 1 << 19, 0, 1, 1, 0, form, buf, 256) == E_COUNT
        assert d(C.byref(_params(abi, "v0", 2, abi.LAYOUT_PER_ENV)), 100, 6, 1, 1, 0, form, buf, 256) == E_GRID
    for form in ("policy", "sample"):
        assert abi.describe_env_rollout(p, 0, 6, form=form) == "" and abi.describe_env_rollout(p, 100, 0, form=form) == ""
    # the existing entries keep refusing a third key mode
    assert abi.lib.lmaze_describe_rollout_policy(C.byref(p), 100, 6, 1, 1, 0, 2, buf, 256) == E_COUNT
    assert abi.lib.lmaze_describe_rollout_sample(C.byref(p), 100, 6, 1, 1, 0, 2, buf, 256) == E_COUNT
    assert abi.KEY_MODES == {"ball": 0, "goal": 1}


# ------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_env_table_kernels_no_scratch():
    """Exactly eight new instantiations (two kernels x v0 / v3 x two forms), none with scratch -- the condition.  Their waves
    per SIMD beside the ball-keyed sibling's of the same kernel and variant are printed: a lower value is not a failure
    here, it is recorded in DESIGN.md with the VGPR counts (measured at this writing: equal, 8 shared / 7 per-env)."""
    kernels = kernel_usage("lmaze_step.hip")
    new = {k: v for k, v in kernels.items() if "RolloutEnvBytesArgs" in k or "RolloutEnvRowsArgs" in k}
    assert len(new) == 8, sorted(new)
    for frag in ("21rollout_shared_kernelILi0E", "21rollout_shared_kernelILi3E", "21rollout_perenv_kernelILi0E",
                 "21rollout_perenv_kernelILi3E"):
        assert sum(frag in k and "19RolloutEnvBytesArgs" in k for k in new) == 1, frag
        assert sum(frag in k and "18RolloutEnvRowsArgs" in k for k in new) == 1, frag
    for name, v in sorted(new.items()):
        twin = name.replace("19RolloutEnvBytesArgs", "17RolloutPolicyArgs").replace("18RolloutEnvRowsArgs", "17RolloutSampleArgs")
        assert twin in kernels and twin != name, name
        print("%s: VGPRs %d, waves per SIMD %d (sibling: %d, %d)" % (name, v["VGPRs"], v["Occupancy"], kernels[twin]["VGPRs"],
                                                                   kernels[twin]["Occupancy"]))
        assert v.get("ScratchSize", 0) == 0, (name, v)
    # the names the older tests count by stay apart from the new structs'
    for old in ("11RolloutArgs", "14RolloutObsArgs", "RolloutPolicyArgs", "RolloutPolicy8Args", "RolloutSampleArgs", "RolloutSample8Args"):
        assert not any(old in k for k in new), old


# ------------------------------------------------------------- plan, then act: the GPU test's control, on the oracle's model
def test_rolled_tables_miss_the_distance_in_the_oracle_model():
    """tests/test_gpu_env_rollout.py lets every env of 777 random mazes follow the table solved for ITS maze and asks for the
    first done at exactly the fewest steps; its control gives env i the table of env i - 1 and asks that more than half of
    the reachable envs miss.  Here the same on the CPU, with the oracle's own model of every maze and the numpy solver of
    solve_ref.py (one of the four cases the GPU test runs; all four, measured when the seeds were chosen: v0 G = 8 607 of
    656 reachable envs miss, v0 G = 11 672 of 695, v3 G = 8 593 of 631, v3 G = 11 644 of 658 -- and none with its own table)."""
    import numpy as np

    import env_table_ref as R
    import solve_ref as SR
    case = R.plan_case("v0", 8)
    pol = SR.solve_many("v0", case["lay"], case["goals"], R.PLAN_GAMMA, R.PLAN_SWEEPS).policy
    reach = np.isfinite(case["dist"])
    assert reach.sum() == 656 and case["T"] == 15
    own = R.follow(case, pol, case["T"])
    assert not R.missed(case, own).any() and (own[~reach] < 0).all()
    rolled = R.missed(case, R.follow(case, np.roll(pol, 1, 0), case["T"]))
    assert rolled.sum() == 607 and rolled.mean() > 0.5
