"""CPU: the recording rollouts' C ABI without a GPU -- the symbols, the documented refusals (answered before any device
call), and what the recording kernels need per wave against their plain twins."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_COUNT, E_VARIANT, E_ALIGN = -1, -5, -3, -6


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_rollout_obs", "lmaze_foveal_rollout_obs"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4
    assert C.sizeof(abi.LmazeParams) == 32


def _grid(abi, T, obs_t, every, n=100):
    p = abi.make_params(abi.VARIANT_V0, 11, abi.LAYOUT_SHARED, 100, -1.0, -0.01, 100.0)
    # fabricated device addresses: every refusal below is returned before anything is dereferenced or queued
    return abi.lib.lmaze_rollout_obs(C.byref(p), 64, 64, T, 64, None, 64, 64, 64, None, None, None, None, n, 1, 1, 0, 0,
                                     obs_t, every, None)


def test_grid_refusals_need_no_device(abi):
    assert _grid(abi, 6, None, -1) == E_COUNT          # obs_every below 0
    assert _grid(abi, 6, 4096, 0) == E_COUNT           # obs_t with obs_every == 0
    assert _grid(abi, 6, None, 3) == E_NULL            # T / k > 0 slots and no obs_t
    assert _grid(abi, 6, 4096 + 4, 3) == E_ALIGN       # obs_t not 16-byte aligned
    assert _grid(abi, 6, None, 3, n=-1) == E_NULL      # the recording checks come first
    assert _grid(abi, 2, 4096 + 4, 3) == E_ALIGN
    assert _grid(abi, -1, None, 0) == E_COUNT          # then lmaze_rollout's own: T < 0
    assert _grid(abi, 6, None, 0, n=-1) == E_COUNT


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("T,n", [(0, 100), (6, 0), (0, 0)])
def test_plain_rollout_with_nothing_to_do_reads_no_pointer(abi, variant, T, n):
    """lmaze_rollout answers T == 0 or n == 0 with 0 once params are valid, before it looks at any pointer, as its siblings
    do: every pointer NULL, nothing launched."""
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, 11, abi.LAYOUT_SHARED, 100, -1.0, -0.01, 100.0)
    assert abi.lib.lmaze_rollout(C.byref(p), None, None, T, None, None, None, None, None, None, None, None, None, n, 1, 1, 0, 0,
                                 None) == 0
    assert abi.lib.lmaze_rollout(C.byref(p), None, None, -1, None, None, None, None, None, None, None, None, None, n, 1, 1, 0, 0,
                                 None) == E_COUNT                  # T < 0 still refused
    assert abi.lib.lmaze_rollout(None, None, None, T, None, None, None, None, None, None, None, None, None, n, 1, 1, 0, 0,
                                 None) == E_NULL                   # params first


def _foveal(abi, variant, T, obs_t, loc_t, every, goals=None, grid=18, n_layouts=5):
    p = abi.LmazeFovealParams(variant, grid, n_layouts, 50, 50, -1.0, -0.01, 100.0, 0)
    bufs = abi.LmazeFovealBuffers()
    return abi.lib.lmaze_foveal_rollout_obs(C.byref(p), 64, 64, goals, T, C.byref(bufs), 100, 0, 1, 0, 0,
                                            None, None, None, None, obs_t, loc_t, every, None)


def test_foveal_refusals_need_no_device(abi):
    v2, v5 = abi.VARIANT_V2, abi.VARIANT_V5
    assert _foveal(abi, v2, 6, 4096, None, 0) == E_COUNT       # no final-planes-only form here
    assert _foveal(abi, v2, 6, 4096, None, -2) == E_COUNT
    assert _foveal(abi, v2, 6, None, None, 3) == E_NULL        # slots and no obs_t
    assert _foveal(abi, v2, 6, 4096 + 8, None, 3) == E_ALIGN
    assert _foveal(abi, v5, 6, 4096, 4096 + 4, 3, goals=64) == E_ALIGN
    assert _foveal(abi, v5, 6, 4096, 4096, 3) == E_VARIANT      # the plain v5/v6 step, as lmaze_foveal_rollout
    assert _foveal(abi, v2, 0, None, None, 3) == 0              # T == 0: nothing to do
    assert _foveal(abi, v2, 2, None, None, 3) == E_NULL         # T < k: no slot, but no buffers either


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,plain_arg,rec_arg,n_rec", [("lmaze_step.hip", "11RolloutArgs", "14RolloutObsArgs", 6),
                                                         ("lmaze_foveal.hip", "10FovealRoll", "13FovealRollObs", 33)])
def test_recording_kernels_no_scratch_and_occupancy(src, plain_arg, rec_arg, n_rec):
    """No scratch anywhere.  The v0/v3 recording kernels and the v5/v6 two-level one keep their plain twin's waves per
    SIMD; v1 / v2 / v4 keep the floors of the plain foveal rollouts (6 / 6 / 4) -- their slot stores cost a wave against
    some twins (lmaze_foveal.hip, the recording overload of foveal_rollout_kernel)."""
    kernels = kernel_usage(src)
    recs = [k for k in kernels if rec_arg in k]
    assert len(recs) == n_rec, recs
    floors = {1: 6, 2: 6, 4: 4}
    for name in recs:
        v = kernels[name]
        twin = name.replace(rec_arg, plain_arg)
        assert twin in kernels, name
        assert v.get("ScratchSize", 0) == 0, (name, v)
        m = re.search(r"foveal_rollout_kernelILi(\d+)E", name)
        if m and int(m.group(1)) in floors:
            assert v["Occupancy"] >= floors[int(m.group(1))], (name, v)
        else:
            assert v["Occupancy"] >= kernels[twin]["Occupancy"], (name, v, kernels[twin])
