"""CPU: the one-launch foveal rollout's C ABI without a GPU -- the symbols, the argument checks (answered before any device
call), the launch the library would queue (lmaze_describe_foveal_rollout), and what its kernels need per wave."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

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


def _params(abi, variant, grid=18, n_layouts=5):
    return abi.LmazeFovealParams(variant, grid, n_layouts, 50, 50, -1.0, -0.01, 100.0, 0)


def _rollout(abi, p, T, n, goals=None, auto_reset=0, actions=None, layouts=None, bufs=None):
    return abi.lib.lmaze_foveal_rollout(C.byref(p) if p is not None else None, layouts, actions, goals, T,
                                        C.byref(bufs) if bufs is not None else None, n, auto_reset, 1, 0, 0,
                                        None, None, None, None, None)


def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_foveal_rollout", "lmaze_describe_foveal_rollout"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4


def test_refusals_need_no_device(abi):
    v2, v5 = _params(abi, abi.VARIANT_V2), _params(abi, abi.VARIANT_V5)
    bufs = abi.LmazeFovealBuffers()                   # every pointer NULL
    assert _rollout(abi, None, 0, 100) == 0           # T == 0: nothing looked at, NULL params included
    assert _rollout(abi, v2, 5, 0) == 0               # n == 0
    assert _rollout(abi, v2, -1, 100) == E_COUNT
    assert _rollout(abi, v2, 5, -1) == E_COUNT
    assert _rollout(abi, v2, 5, (1 << 40)) == E_COUNT
    assert _rollout(abi, v2, 5, 100) == E_NULL        # no layouts / buffers / actions
    assert _rollout(abi, v2, 5, 100, layouts=16, bufs=bufs, actions=16) == E_NULL
    assert _rollout(abi, v2, 5, 100, goals=16) == E_VARIANT          # planner goals: v5/v6 only
    assert _rollout(abi, _params(abi, abi.VARIANT_V1, 14, 1), 5, 100, goals=16) == E_VARIANT
    assert _rollout(abi, v5, 5, 100, auto_reset=1) == E_NULL          # v5/v6 restart through plannerStep: goals needed
    assert _rollout(abi, v5, 5, 100) == E_VARIANT                     # the plain v5/v6 step has no one-launch form
    assert _rollout(abi, _params(abi, 3), 5, 100, layouts=16, bufs=bufs, actions=16) == E_VARIANT


_ALIGN_CHILD = r"""
import ctypes as C, importlib, sys
sys.path.insert(0, sys.argv[1])
abi = importlib.import_module("gym-lmaze_amd._abi")
p = abi.LmazeFovealParams(abi.VARIANT_V2, 18, 5, 50, 50, -1.0, -0.01, 100.0, 0)
fake = {f: 1 << 20 for f in abi.FOVEAL_BUFFER_FIELDS}
fake["obs"] = (1 << 20) + 4
b = abi.LmazeFovealBuffers(**fake)
step = abi.lib.lmaze_foveal_step(C.byref(p), 64, 64, C.byref(b), 100, None)
roll = abi.lib.lmaze_foveal_rollout(C.byref(p), 64, 64, None, 3, C.byref(b), 100, 0, 1, 0, 0, None, None, None, None, None)
print(step, roll)
"""


def test_obs_alignment_as_the_step(abi):
    # fabricated addresses: refused by the argument checks before any device call.  Run where no device is visible, so
    # that a regression of the check could not reach a GPU
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _ALIGN_CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    step, roll = (int(x) for x in out.stdout.split()[-2:])
    assert step == E_ALIGN and roll == E_ALIGN


@pytest.mark.parametrize("n", [16384, 1 << 20])
@pytest.mark.parametrize("variant,auto_reset,two_level", [("v1", 0, 0), ("v1", 1, 0), ("v2", 0, 0), ("v2", 1, 0),
                                                          ("v4", 0, 0), ("v4", 1, 0), ("v5", 1, 1), ("v6", 1, 1)])
def test_describe_names_the_rollout_kernel(abi, variant, auto_reset, two_level, n):
    vid = {"v1": abi.VARIANT_V1, "v2": abi.VARIANT_V2, "v4": abi.VARIANT_V4, "v5": abi.VARIANT_V5, "v6": abi.VARIANT_V6}[variant]
    p = _params(abi, vid, 14 if variant == "v1" else 18, 1 if variant == "v1" else 5)
    text = abi.describe_foveal_rollout(p, n, 64, auto_reset, two_level)
    kv = "v5" if variant in ("v5", "v6") else variant
    kind = "two-level" if two_level else ("fused-reset" if auto_reset else "plain")
    assert re.match(r"foveal_rollout_kernel<%s, (32|64|128), (14|18), %s> T=64 " % (kv, kind), text), text
    assert "foveal_kernel<" not in text
    for hint, epb in ((0x20, 32), (0x30, 64), (0x40, 128), (0x145, 128)):
        p.launch_hint = hint
        assert "envs_per_workgroup=%d" % epb in abi.describe_foveal_rollout(p, n, 8, auto_reset, two_level)
    p.launch_hint = 0
    assert abi.describe_foveal_rollout(p, 0, 8, auto_reset, two_level) == ""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rollout_kernels_no_scratch_and_occupancy_floors():
    kernels = kernel_usage("lmaze_foveal.hip")
    floors = {1: 6, 2: 6, 4: 4, 5: 4}
    seen = set()
    for name, v in kernels.items():
        m = re.search(r"foveal_rollout_kernelILi(\d+)E", name)
        if not m:
            continue
        assert "foveal_kernelI" not in name
        seen.add(int(m.group(1)))
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v["Occupancy"] >= floors[int(m.group(1))], (name, v)
    assert seen == {1, 2, 4, 5}
