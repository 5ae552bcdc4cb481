"""CPU: the LDS layout of the workgroup rollout kernels, csrc/lmaze_rollout_lds.h -- the one text from which bodies 2-4 of
lmaze_rollout_body.h take their pointers and rollout_plan the bytes a launch requests.  tests/csrc/rollout_lds_host.cpp
compiles it for the host under the address and undefined-behaviour sanitizers and, for G = 3..64 (u8: 4..64), every envs
per workgroup the plan can pick and all four table kinds, writes every array's whole extent into exactly `total` bytes
through a pointer of the array's element type; here the extents are checked to be disjoint, the totals to be what the
host requested before there was a shared text, and the describe lines to request exactly the header's total."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

import launch_matrix as M
from closed_loop_ref import fields, perenv_lds, shared_lds, u8_lds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, BYTES, ROWS, GLOBAL = 0, 1, 2, 3          # LMAZE_TAB_*
EPB = {"shared": (4, 8, 16, 32, 64, 128, 256), "perenv": (4, 8, 16, 32, 64), "u8": (16, 32, 64, 128, 256)}


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """{(body, G, epb, kind): (total, [(array, offset, bytes), ...])} as the program printed them.  It is built with the
    sanitizers and run as a program (never loaded into this process): any report fails the run."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("rollout_lds") / "rollout_lds_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "csrc", "rollout_lds_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    cases = {}
    lines = out.stdout.splitlines()
    assert lines[-1].startswith("read_back ")
    for line in lines[:-1]:
        w = line.split()
        arrays = [(w[i], int(w[i + 1]), int(w[i + 2])) for i in range(5, len(w), 3)]
        cases[(w[0], int(w[1]), int(w[2]), int(w[3]))] = (int(w[4]), arrays)
    return cases


def test_the_sweep_is_whole(layouts):
    want = {(body, G, epb, kind) for body, sizes in EPB.items() for G in range(4 if body == "u8" else 3, 65) for epb in sizes
            for kind in (NONE, BYTES, ROWS, GLOBAL)}
    assert set(layouts) == want


def test_every_array_is_written_and_none_overlaps_another(layouts):
    """The arrays each body indexes, by name; inside [0, total); pairwise disjoint (the per-env layouts are written twice,
    by dwords and by bytes: one extent)."""
    names = {"shared": {"pat", "ballflat", "goalflat", "lay", "spawn"}, "perenv": {"ballflat", "goalflat", "lay"},
             "u8": {"pat", "ballflat", "goalflat", "lay", "spawn"}}
    for (body, G, epb, kind), (total, arrays) in layouts.items():
        assert {a[0] for a in arrays} == names[body] | ({"tab"} if kind in (BYTES, ROWS) else set()), (body, G, epb, kind)
        extent = {}
        for name, off, size in arrays:
            lo, hi = extent.get(name, (off, off + size))
            assert lo == off, (body, G, epb, kind, name)
            extent[name] = (lo, max(hi, off + size))
        spans = sorted(extent.values())
        assert spans[0][0] == 0 and spans[-1][1] <= total, (body, G, epb, kind, spans, total)
        for (_, hi), (lo, _) in zip(spans, spans[1:]):
            assert hi <= lo, (body, G, epb, kind, spans)
        if kind == ROWS:
            assert extent["tab"] == (total - 16 * G * G, total) and extent["tab"][0] % 16 == 0


def test_the_totals_are_what_the_host_requested_before(layouts):
    """The byte sums rollout_plan held before the shared text (restated in closed_loop_ref.py, which the describe tests of
    every form still use): the body's own arrays; the epsilon-greedy table adds G^2 rounded up to 16; the sampling forms
    round the arrays up to 16 and add 16 G^2 when the thresholds are staged.  The u8 body's own sum is rounded always."""
    own = {"shared": shared_lds, "perenv": perenv_lds, "u8": u8_lds}
    for (body, G, epb, kind), (total, _) in layouts.items():
        base = own[body](G, epb)
        want = {NONE: base, BYTES: base + ((G * G + 15) & ~15), ROWS: ((base + 15) & ~15) + 16 * G * G, GLOBAL: (base + 15) & ~15}[kind]
        assert total == want, (body, G, epb, kind, total, want)


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


BODY = {"rollout_shared_kernel": "shared", "rollout_perenv_kernel": "perenv", "rollout_shared_u8_kernel": "u8"}


def _kind(line):
    if "table=lds" in line:
        return ROWS
    if "table=global" in line:
        return GLOBAL
    return BYTES if "policy=" in line else NONE


def test_every_describe_line_requests_the_headers_total(abi, layouts):
    """lmaze_describe_rollout, _policy and _sample over the shapes of launch_matrix.py (the rollout rows of its table and its
    sweep's grids and batch sizes) x launch_hint bits 12-14, int32 and narrow planes, with and without recorded slots, both
    key modes: `lds=` is the header's total for the body, the table kind and the envs per workgroup the same line names.
    The wave-autonomous 8x8 kernel and the T-launch fallback's step kernels are not these bodies."""
    shapes = {(r.layout, r.G, r.N) for r in M.ROWS if r.entry.startswith("rollout")}
    shapes |= {(lay, G, n) for lay in (M.SHARED, M.PER_ENV) for G in M.SWEEP_GRIDS for n in M.SWEEP_N}
    seen = set()
    for layout, G, N in sorted(shapes):
        for variant in ("v0", "v3"):
            for k in range(8):
                p = M.params(abi, variant, G, layout, M.hint(ro_epb=k))
                lines = []
                for with_obs in (True, "u8") if layout == M.SHARED and G >= 4 else (True,):
                    lines += [abi.describe_rollout(p, N, 16, auto_reset=True, with_obs=with_obs, obs_every=e) for e in (None, 0, 3)]
                    for key in ("ball", "goal") if variant == "v3" else ("ball",):
                        for d in (abi.describe_rollout_policy, abi.describe_rollout_sample):
                            lines += [d(p, N, 16, with_obs=with_obs, obs_every=e, key=key) for e in (0, 3)]
                for line in lines:
                    name = re.match(r"\w+", line).group(0)
                    f = fields(line)
                    if name not in BODY:
                        assert name == "rollout_shared_wave8_kernel" and f["lds"] == 0, line
                        continue
                    case = (BODY[name], G, f["envs_per_workgroup"], _kind(line))
                    assert f["lds"] == layouts[case][0], (line, case, layouts[case][0])
                    seen.add((case[0], case[3], ", obs_t" in line))
    assert seen == {(b, kind, rec) for b in BODY.values() for kind in (NONE, BYTES, ROWS, GLOBAL) for rec in (False, True)}
