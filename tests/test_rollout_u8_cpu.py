"""CPU: the u8 rollouts' C ABI without a GPU -- the symbols, the launcher's own description of every grid rollout
(lmaze_describe_rollout), the documented refusals (answered before any device call), and what the new kernels need per
wave."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from helpers import HIPCC, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def _params(abi, variant="v0", G=11, layout=None, hint=0):
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, G,
                        abi.LAYOUT_SHARED if layout is None else layout, 100, -1.0, -0.01, 100.0)
    p.launch_hint = hint
    return p


def _epb(text):
    return int(re.search(r"envs_per_workgroup=(\d+)", text).group(1))


def _grid(text):
    return int(re.search(r"grid=(\d+)", text).group(1))


def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_rollout_u8", "lmaze_rollout_obs_u8", "lmaze_describe_rollout"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4


# ---------------------------------------------------------------- which kernel a rollout runs
@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("n,epb", [(1, 16), (777, 16), (16384, 16), (65535, 16), (65536, 64), (262144, 64), (1 << 20, 64)])
def test_describe_u8_names_the_u8_kernel_and_its_envs_per_workgroup(abi, variant, n, epb):
    p = _params(abi, variant)
    for T in (1, 16):
        text = abi.describe_rollout(p, n, T, with_obs="u8")
        assert text.startswith("rollout_shared_u8_kernel<%s> T=%d " % (variant, T)), text
        assert _epb(text) == epb and _grid(text) == (n + epb - 1) // epb, text
        assert "block=256" in text
    rec = abi.describe_rollout(p, n, 16, auto_reset=True, with_obs="u8", obs_every=3)
    assert rec.startswith("rollout_shared_u8_kernel<%s, obs_t> T=16 every=3 " % variant), rec
    assert _epb(rec) == (256 if n >= 262144 else epb), rec          # slots beyond the Infinity Cache: the widest workgroups
    fin = abi.describe_rollout(p, n, 16, with_obs="u8", obs_every=0)
    assert fin.startswith("rollout_shared_u8_kernel<%s, obs_t> T=16 every=0 " % variant) and _epb(fin) == epb, fin


@pytest.mark.parametrize("k,epb", [(1, 16), (2, 16), (3, 16), (4, 32), (5, 64), (6, 128), (7, 256)])
def test_describe_u8_hint_bits_are_clamped_to_multiples_of_16(abi, k, epb):
    for G in (4, 11, 33, 64):
        text = abi.describe_rollout(_params(abi, "v3", G, hint=k << 12), 100000, 8, with_obs="u8")
        assert _epb(text) == epb, (G, text)
        lds = int(re.search(r"lds=(\d+)", text).group(1))
        assert lds <= 64 << 10 and lds % 16 == 0, text


def test_describe_int32_names_launch_rollouts_kernels(abi):
    d = abi.describe_rollout
    PER_ENV = abi.LAYOUT_PER_ENV
    assert d(_params(abi, "v0", 8), 65536, 16).startswith("rollout_shared_wave8_kernel<v0, 64> T=16 ")
    assert d(_params(abi, "v3", 8), 65536, 16, obs_every=2).startswith("rollout_shared_wave8_kernel<v3, 64, obs_t> T=16 every=2 ")
    assert d(_params(abi, "v0", 11), 65536, 16).startswith("rollout_shared_kernel<v0> T=16 ")
    assert d(_params(abi, "v3", 12), 777, 9, obs_every=0).startswith("rollout_shared_kernel<v3, obs_t> T=9 every=0 ")
    assert d(_params(abi, "v0", 11, PER_ENV), 4096, 16).startswith("rollout_perenv_kernel<v0> T=16 ")
    assert d(_params(abi, "v3", 18, PER_ENV), 4096, 16, obs_every=1).startswith("rollout_perenv_kernel<v3, obs_t> T=16 every=1 ")
    # T == 1, launch_hint bit 8: the step kernel of the T-launch fallback
    assert d(_params(abi, "v0", 11), 4096, 1).startswith("step_shared_kernel<11, v0, step, ")
    assert d(_params(abi, "v0", 11, hint=0x100), 4096, 16).startswith("step_shared_kernel<11, v0, step, ")
    assert d(_params(abi, "v0", 11), 4096, 16, with_obs=False).startswith("rollout_shared_kernel<v0> T=16 ")
    # nothing to do: an empty line
    assert d(_params(abi, "v0", 11), 0, 16) == "" and d(_params(abi, "v0", 11), 100, 0, with_obs="u8") == ""


def test_describe_int32_sizing_rules(abi):
    """Every sizing rule of the grid rollouts, pinned by the launcher's own description."""
    d = abi.describe_rollout
    PER_ENV = abi.LAYOUT_PER_ENV
    tail = " block=256 lds=%d envs_per_workgroup=%d workgroups_per_cu=0 chunks=1"
    # shared layouts: 16 / 32 / 64 envs by batch size; beyond the caches the L2 fit (1M x 11x11: 16), but not for the
    # recording form, which keeps the size by batch
    assert d(_params(abi, "v0", 11), 4096, 16) == "rollout_shared_kernel<v0> T=16 grid=256" + tail % (996, 16)
    assert d(_params(abi, "v0", 11), 1 << 20, 16) == "rollout_shared_kernel<v0> T=16 grid=65536" + tail % (996, 16)
    assert d(_params(abi, "v0", 11), 1 << 20, 16, obs_every=1) == \
        "rollout_shared_kernel<v0, obs_t> T=16 every=1 grid=16384" + tail % (1380, 64)
    # per-env layouts: at most 32 KiB of layouts per workgroup (777 x 64x64: 8), the L2 fit (262 144 x 32x32: 8), and
    # the recording form's halving of 32 envs at 16 384 to 65 535 envs
    assert d(_params(abi, "v3", 64, PER_ENV), 777, 16) == "rollout_perenv_kernel<v3> T=16 grid=98" + tail % (32832, 8)
    assert d(_params(abi, "v0", 32, PER_ENV), 262144, 16) == "rollout_perenv_kernel<v0> T=16 grid=32768" + tail % (8256, 8)
    assert d(_params(abi, "v0", 11, PER_ENV), 16384, 16) == "rollout_perenv_kernel<v0> T=16 grid=512" + tail % (4128, 32)
    assert d(_params(abi, "v0", 11, PER_ENV), 16384, 16, obs_every=1) == \
        "rollout_perenv_kernel<v0, obs_t> T=16 every=1 grid=1024" + tail % (2064, 16)
    # launch_hint bits 12-14 = k: 4 << (k - 1) envs per workgroup, over the L2 fit; per-env at most 64; the on-die 8x8
    # form does not read them
    assert d(_params(abi, "v0", 11, hint=0x1000), 1 << 20, 16) == "rollout_shared_kernel<v0> T=16 grid=262144" + tail % (900, 4)
    assert d(_params(abi, "v0", 11, hint=0x3000), 1 << 20, 16) == "rollout_shared_kernel<v0> T=16 grid=65536" + tail % (996, 16)
    assert d(_params(abi, "v0", 11, hint=0x5000), 65536, 16) == "rollout_shared_kernel<v0> T=16 grid=1024" + tail % (1380, 64)
    assert d(_params(abi, "v0", 11, PER_ENV, hint=0x2000), 4096, 16) == "rollout_perenv_kernel<v0> T=16 grid=512" + tail % (1040, 8)
    assert d(_params(abi, "v0", 11, PER_ENV, hint=0x7000), 4096, 16) == "rollout_perenv_kernel<v0> T=16 grid=64" + tail % (8256, 64)
    assert d(_params(abi, "v3", 11, PER_ENV, hint=0x7000), 16384, 16, auto_reset=True, with_obs=False, obs_every=17) == \
        "rollout_perenv_kernel<v3, obs_t> T=16 every=17 grid=256" + tail % (8256, 64)
    assert d(_params(abi, "v3", 8, hint=0x7000), 65536, 16) == \
        "rollout_shared_wave8_kernel<v3, 64> T=16 grid=256 block=256 lds=0 envs_per_workgroup=256 workgroups_per_cu=0 chunks=1"


def test_describe_u8_sizing_rules(abi):
    d = abi.describe_rollout
    tail = " block=256 lds=%d envs_per_workgroup=%d workgroups_per_cu=0 chunks=1"
    # 64 envs from 65 536 on; recording slots at >= 262 144 envs: 256
    assert d(_params(abi, "v0", 11), 262144, 16, auto_reset=True, with_obs="u8") == \
        "rollout_shared_u8_kernel<v0> T=16 grid=4096" + tail % (1936, 64)
    assert d(_params(abi, "v0", 11), 262144, 16, auto_reset=True, with_obs="u8", obs_every=3) == \
        "rollout_shared_u8_kernel<v0, obs_t> T=16 every=3 grid=1024" + tail % (3472, 256)
    # launch_hint bits 12-14 over that rule, rounded up to 16
    assert d(_params(abi, "v3", 32, hint=0x1000), 1 << 20, 16, auto_reset=True, with_obs="u8", obs_every=1) == \
        "rollout_shared_u8_kernel<v3, obs_t> T=16 every=1 grid=65536" + tail % (11472, 16)


def test_describe_refusals(abi):
    buf = C.create_string_buffer(256)
    f = abi.lib.lmaze_describe_rollout
    assert f(C.byref(_params(abi, "v0", 11, abi.LAYOUT_PER_ENV)), 100, 4, 0, 2, -1, buf, 256) == E_LAYOUT
    assert f(C.byref(_params(abi, "v0", 3)), 100, 4, 0, 2, -1, buf, 256) == E_GRID
    assert f(C.byref(_params(abi, "v0", 11)), 100, -1, 0, 2, -1, buf, 256) == E_COUNT
    assert f(C.byref(_params(abi, "v0", 11)), 100, 4, 0, 2, -1, None, 256) == E_NULL
    bad = _params(abi, "v0", 11)
    bad.variant = abi.VARIANT_V1
    assert f(C.byref(bad), 100, 4, 0, 2, -1, buf, 256) == E_VARIANT


# ---------------------------------------------------------------- refusals before anything is queued
def _plain(abi, T=6, n=100, obs8=4096, actions=64, G=11, layout=None, variant="v0", ball=64):
    p = _params(abi, variant, G, layout)
    # fabricated device addresses: every refusal below is returned before anything is dereferenced or queued
    return abi.lib.lmaze_rollout_u8(C.byref(p), 64, actions, T, ball, 64 if variant == "v3" else None, 64, 64, 64, None, obs8,
                                    None, None, n, 1, 1, 0, 0, None)


def _rec(abi, obs_t8, every, T=6, n=100, obs8=4096, actions=64, G=11, layout=None):
    p = _params(abi, "v0", G, layout)
    return abi.lib.lmaze_rollout_obs_u8(C.byref(p), 64, actions, T, 64, None, 64, 64, 64, None, obs8, None, None, n, 1, 1, 0, 0,
                                        obs_t8, every, None)


def test_u8_refusals_need_no_device(abi):
    assert _plain(abi, actions=None) == E_NULL                          # null pointers
    assert _plain(abi, ball=None) == E_NULL
    assert _plain(abi, variant="v3", obs8=4096 + 3) == E_ALIGN
    assert _plain(abi, layout=abi.LAYOUT_PER_ENV) == E_LAYOUT           # per-env layouts
    assert _plain(abi, G=3) == E_GRID                                   # G < 4
    assert _plain(abi, obs8=4096 + 5) == E_ALIGN                        # obs8 not 16-byte aligned
    assert _plain(abi, ball=64 + 4) == E_ALIGN
    assert _plain(abi, T=-1) == E_COUNT
    assert _plain(abi, n=-1) == E_COUNT
    assert _plain(abi, T=0, actions=None, ball=None) == 0               # T == 0: nothing read, ahead of the null checks
    assert _plain(abi, n=0, actions=None, ball=None) == 0
    assert _rec(abi, None, -1) == E_COUNT                               # obs_every < 0
    assert _rec(abi, 4096, 0) == E_COUNT                                # obs_t8 with obs_every == 0
    assert _rec(abi, None, 3) == E_NULL                                 # T / k > 0 slots and no obs_t8
    assert _rec(abi, 4096 + 7, 3) == E_ALIGN                            # obs_t8's base (slot 0) not 16-byte aligned
    assert _rec(abi, 4096 + 7, 3, n=-1) == E_ALIGN                      # the recording checks come first
    assert _rec(abi, 4096, 3, layout=abi.LAYOUT_PER_ENV) == E_LAYOUT
    assert _rec(abi, 4096, 3, G=3) == E_GRID
    assert _rec(abi, 4096, 3, obs8=4096 + 1) == E_ALIGN
    assert _rec(abi, 4096, 3, actions=None) == E_NULL
    assert _rec(abi, None, 0, T=0, actions=None) == 0                   # T == 0
    assert _rec(abi, None, 7, T=6, n=0, actions=None) == 0              # n == 0


# ---------------------------------------------------------------- what the new kernels need per wave
# measured with -Rpass-analysis=kernel-resource-usage when the kernels were added: the plain forms 72 / 85 VGPRs (v0 / v3),
# the recording forms 75 / 86
U8_FLOORS = {("0", "11RolloutArgs"): 7, ("3", "11RolloutArgs"): 5, ("0", "15RolloutObs8Args"): 6, ("3", "15RolloutObs8Args"): 5}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_u8_rollout_kernels_no_scratch_and_occupancy():
    kernels = kernel_usage("lmaze_step.hip")
    found = {}
    for name, v in kernels.items():
        m = re.search(r"rollout_shared_u8_kernelILi(\d)EEEvNS_8StepArgsENS_(\w+)E$", name)
        if m:
            found[(m.group(1), m.group(2))] = v
    assert sorted(found) == sorted(U8_FLOORS), sorted(found)
    for key, v in found.items():
        assert v.get("ScratchSize", 0) == 0, (key, v)
        assert v["Occupancy"] >= U8_FLOORS[key], (key, v)
