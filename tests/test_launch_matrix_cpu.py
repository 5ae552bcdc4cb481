"""CPU: the launch-policy table of launch_matrix.py against the launchers' own description (no GPU).  Every kernel
instantiation the describe sweep names is run by some GPU row (test_gpu_launch_matrix.py), and every plan of the sweep
is one a gfx950 workgroup can launch: LDS within 160 KiB, the grid covering the batch, and a rollout plan that only its
own hint bits change."""
import importlib
import os
import subprocess
from collections import defaultdict

import pytest

import launch_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


@pytest.fixture(scope="module")
def swept(abi):
    return [(call, text) for call, text in M.sweep(abi) if text]


def test_every_kernel_the_sweep_names_has_a_gpu_row(abi, swept):
    where = defaultdict(list)
    for call, text in swept:
        where[M.kernel_key(text)].append(call)
    covered = {M.kernel_key(M.describe(abi, *r)) for r in M.ROWS}
    missing = sorted(set(where) - covered)
    assert not missing, "kernels no row of launch_matrix.ROWS runs (one call that picks each): " + "; ".join(
        "%s <- %s" % (k, where[k][0]) for k in missing)
    assert len(where) >= 150, len(where)              # the sweep still reaches what it did when the table was written


def test_every_plan_of_the_sweep_is_launchable(swept):
    for call, text in swept:
        lds, epb, grid = M.field(text, "lds"), M.field(text, "envs_per_workgroup"), M.field(text, "grid")
        assert lds <= M.LDS_PER_WORKGROUP, (call, text)
        if not text.startswith("rollout_"):
            continue
        n = call[4]
        assert (grid - 1) * epb < n <= grid * epb, (call, text)
        if text.startswith("rollout_shared_u8_kernel"):
            assert lds <= M.LDS_U8_ROLLOUT and epb in (16, 32, 64, 128, 256), (call, text)
        elif text.startswith("rollout_perenv_kernel"):
            assert epb in (4, 8, 16, 32, 64), (call, text)
        elif text.startswith("rollout_shared_kernel"):
            assert epb in (4, 8, 16, 32, 64, 128, 256), (call, text)


@pytest.mark.parametrize("other", [0x0F, 0x53, 0x200, 0x400, 0xC00, 0xEFF])
def test_rollout_plans_ignore_the_step_hint_bits(abi, other):
    """bits 0-7, 9, 10 and 11 belong to the step kernels: a one-launch rollout's plan never reads them"""
    checked = 0
    for variant in ("v0", "v3"):
        for layout in (M.SHARED, M.PER_ENV):
            for G in M.SWEEP_GRIDS:
                for n in M.SWEEP_N:
                    for h in M.ROLLOUT_HINTS:
                        for with_obs, k in ((True, None), (False, 3), ("u8", None), ("u8", 0)):
                            if with_obs == "u8" and (layout == M.PER_ENV or G < 4):
                                continue
                            base = abi.describe_rollout(M.params(abi, variant, G, layout, h), n, 16, True, with_obs, k)
                            if not base.startswith("rollout_"):
                                continue                    # the T-launch fallback: the step kernel, which reads them
                            assert abi.describe_rollout(M.params(abi, variant, G, layout, h | other), n, 16, True,
                                                        with_obs, k) == base, (variant, layout, G, n, hex(h))
                            checked += 1
    assert checked > 3000


@pytest.mark.parametrize("G", [50, 51, 57, 64])
def test_per_env_rollouts_past_g50_fit_one_workgroup(abi, G):
    """per-env layouts with 64 envs per workgroup (launch_hint bits 12-14 = 5..7) outgrow 160 KiB of LDS from G = 51
    on: the plan halves them to 32"""
    want = 64 if 64 * G * G + 2 * 64 * 4 <= M.LDS_PER_WORKGROUP else 32
    assert want == (64 if G == 50 else 32)
    for k in (5, 6, 7):
        for n in M.SWEEP_N:
            for with_obs, every in ((True, None), (False, None), (True, 3), (False, 0)):
                for variant in ("v0", "v3"):
                    text = abi.describe_rollout(M.params(abi, variant, G, M.PER_ENV, M.hint(ro_epb=k)), n, 16, True,
                                                with_obs, every)
                    assert text.startswith("rollout_perenv_kernel<%s" % variant), text
                    assert M.field(text, "envs_per_workgroup") == want, text
                    assert M.field(text, "lds") <= M.LDS_PER_WORKGROUP, text


def test_the_table_is_cheap_and_ragged(abi):
    """every row: a small T, planes within 256 MiB; N ragged against the envs per workgroup the row gets; each rollout
    family has a row with fewer envs than one workgroup holds; recordings leave trailing steps and odd slot sizes"""
    below = set()
    for r in M.ROWS:
        assert r.entry in M.ENTRIES and 1 <= r.T <= 16 and r.N * r.G * r.G * 4 <= 256 << 20, r
        assert (r.obs_every is not None) == (r.entry in (M.ROLLOUT_OBS, M.ROLLOUT_OBS_U8)), r
        text = M.describe(abi, *r)
        epb = M.field(text, "envs_per_workgroup")
        assert epb == 1 or r.N % epb, (r, text)
        if r.N < epb:
            below.add(text.split("<")[0])
    assert {"rollout_shared_kernel", "rollout_perenv_kernel", "rollout_shared_u8_kernel", "step_shared_kernel"} <= below
    rec = [r for r in M.ROWS if r.obs_every]
    assert any(r.T % r.obs_every for r in rec) and any(r.N * r.G * r.G % 2 for r in rec)
    assert any(r.hint & 0x8000 for r in rec)
    assert len(M.groups()) < 300
