"""CPU: the refusals of the grid step / observe entry points and lmaze_reset (include/lmaze.h), their codes and their
order.  No device is needed and none is touched: every call passes n = 0 (or n < 0), so a call that is not refused
returns 0 from the launcher before anything is queued -- the refusals all stand before that -- and fabricated, aligned
addresses stand for the buffers.  Nothing is dereferenced."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
V0, V3 = 0, 3

# name -> (arguments behind params in the order of include/lmaze.h, variants taken, narrow planes, pointers that must not be
# NULL (goal_xy: v3 only)); "obs" is obs8 for the narrow entries
STATE = ("layout", "action", "ball_xy", "step_count", "reward", "done")
RESET = ("seed", "epoch", "env_base", "epoch_in", "epoch_out")
ENTRIES = {
    "lmaze_step_v0": (("layout", "action", "ball_xy", "step_count", "reward", "done", "goal_count", "obs", "n", "stream"),
                      (V0,), False, STATE),
    "lmaze_step_v3": (("layout", "action", "ball_xy", "goal_xy", "step_count", "reward", "done", "obs", "n", "stream"),
                      (V3,), False, STATE + ("goal_xy",)),
    "lmaze_step_v0_autoreset": (("layout", "action", "ball_xy", "step_count", "reward", "done", "goal_count", "obs", "n") + RESET
                                + ("stream",), (V0,), False, STATE),
    "lmaze_step_v3_autoreset": (("layout", "action", "ball_xy", "goal_xy", "step_count", "reward", "done", "obs", "n") + RESET
                                + ("stream",), (V3,), False, STATE + ("goal_xy",)),
    "lmaze_step_u8": (("layout", "action", "ball_xy", "goal_xy", "step_count", "reward", "done", "goal_count", "obs", "n",
                       "auto_reset") + RESET + ("stream",), (V0, V3), True, STATE + ("goal_xy",)),
    "lmaze_observe": (("layout", "ball_xy", "goal_xy", "obs", "n", "stream"), (V0, V3), False, ("layout", "ball_xy", "obs", "goal_xy")),
    "lmaze_observe_u8": (("layout", "ball_xy", "goal_xy", "mask", "obs", "n", "stream"), (V0, V3), True,
                         ("layout", "ball_xy", "obs", "goal_xy")),
    "lmaze_reset": (("layout", "mask", "seed", "epoch", "env_base", "ball_xy", "goal_xy", "step_count", "reward", "done", "obs", "n",
                     "stream"), (V0, V3), False, ("layout", "ball_xy", "step_count", "reward", "done", "goal_xy")),
}
# fabricated addresses, each on a 4-KiB boundary; scalars
VALID = dict(layout=0x10000, action=0x11000, ball_xy=0x12000, goal_xy=0x13000, step_count=0x14000, reward=0x15000, done=0x16000,
             goal_count=0x17000, obs=0x18000, mask=0x19000, epoch_in=0x1a000, epoch_out=0x1a008, n=0, stream=None, seed=7, epoch=3,
             env_base=0, auto_reset=1)
# the documented alignments (ball_xy / goal_xy 8, obs 16, layout 16): the offset that breaks each
OFF = dict(ball_xy=4, goal_xy=4, obs=8, layout=1)

CASES = [(name, v) for name, e in ENTRIES.items() for v in e[1]]


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def call(abi, name, variant=None, G=11, mode=0, params=True, **over):
    order, variants, _, _ = ENTRIES[name]
    assert over.get("n", 0) <= 0, "a call of this file never gets as far as a launch"
    p = abi.make_params(variants[0] if variant is None else variant, G, mode, 50, -1.0, -0.01, 100.0)
    args = dict(VALID, **over)
    return getattr(abi.lib, name)(C.byref(p) if params else None, *[args[k] for k in order])


@pytest.mark.parametrize("name,variant", CASES)
def test_valid_arguments_with_no_envs_return_0(abi, name, variant):
    order = ENTRIES[name][0]
    assert call(abi, name, variant) == 0
    # goal_count, the mask and (but for the observe entries, which write nothing else) the planes are optional
    optional = [k for k in ("goal_count", "mask") if k in order] + ([] if "observe" in name else ["obs"])
    for k in optional:
        assert call(abi, name, variant, **{k: None}) == 0, k
    assert call(abi, name, variant, **{k: None for k in optional}) == 0
    if variant == V0 and "goal_xy" in order:
        assert call(abi, name, variant, goal_xy=None) == 0           # v0 keeps no goal
    if "epoch_in" in order:
        assert call(abi, name, variant, epoch_in=None, epoch_out=None) == 0
        assert call(abi, name, variant, epoch_out=None) == 0
    for G in (3, 4, 64):
        if not (ENTRIES[name][2] and G == 3):
            assert call(abi, name, variant, G=G) == 0, G
    if not ENTRIES[name][2]:
        assert call(abi, name, variant, mode=1) == 0                  # per-env layouts


@pytest.mark.parametrize("name,variant", CASES)
def test_params_are_refused_first(abi, name, variant):
    assert call(abi, name, variant, params=False) == E_NULL
    assert call(abi, name, variant, G=2) == E_GRID
    assert call(abi, name, variant, G=65) == E_GRID
    assert call(abi, name, variant, mode=2) == E_LAYOUT
    assert call(abi, name, variant, mode=-1) == E_LAYOUT
    assert call(abi, name, variant, n=-1) == E_COUNT
    # ... in that order, and before the variant and every pointer
    assert call(abi, name, variant, G=2, mode=2, n=-1) == E_GRID
    assert call(abi, name, variant, mode=2, n=-1) == E_LAYOUT
    assert call(abi, name, 1, n=-1, layout=None) == E_COUNT
    assert call(abi, name, 1, G=65, ball_xy=VALID["ball_xy"] + 4) == E_GRID


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_wrong_variant_is_refused_before_any_pointer(abi, name):
    _, variants, _, required = ENTRIES[name]
    wrong = [v for v in (V0, 1, 2, V3, 4, 5, 6, 7, -1) if v not in variants]
    for v in wrong:
        assert call(abi, name, v) == E_VARIANT, v
        for k in required:
            assert call(abi, name, v, **{k: None}) == E_VARIANT, (v, k)
        assert call(abi, name, v, ball_xy=VALID["ball_xy"] + 4) == E_VARIANT, v


@pytest.mark.parametrize("name,variant", [c for c in CASES if ENTRIES[c[0]][2]])
def test_the_narrow_planes_refuse_per_env_layouts_and_g3(abi, name, variant):
    assert call(abi, name, variant, mode=1) == E_LAYOUT
    assert call(abi, name, variant, G=3) == E_GRID
    assert call(abi, name, variant, mode=1, G=3) == E_LAYOUT             # the layout mode first
    assert call(abi, name, 1, mode=1, G=3) == E_VARIANT                  # after the variant
    assert call(abi, name, variant, mode=1, layout=None) == E_LAYOUT     # before the pointers
    assert call(abi, name, variant, G=3, obs=VALID["obs"] + 8) == E_GRID


@pytest.mark.parametrize("name,variant", CASES)
def test_each_required_pointer(abi, name, variant):
    order, _, _, required = ENTRIES[name]
    for k in required:
        if k == "goal_xy" and variant == V0:
            continue
        assert call(abi, name, variant, **{k: None}) == E_NULL, k
        # a NULL pointer together with a misaligned one: LMAZE_E_NULL
        other = "obs" if k == "ball_xy" else "ball_xy"
        assert call(abi, name, variant, **{k: None, other: VALID[other] + OFF[other]}) == E_NULL, (k, other)
        if "epoch_in" in order:
            assert call(abi, name, variant, **{k: None, "epoch_in": VALID["epoch_in"] + 4}) == E_NULL, k


@pytest.mark.parametrize("name,variant", CASES)
def test_each_aligned_pointer(abi, name, variant):
    order, _, u8, _ = ENTRIES[name]
    for k, off in OFF.items():
        if k not in order:
            continue
        want = 0 if (k == "layout" and u8) else E_ALIGN                 # the narrow entries read the layout by bytes
        assert call(abi, name, variant, **{k: VALID[k] + off}) == want, k
    # any smaller offset too
    for off in (1, 2, 4, 8):
        assert call(abi, name, variant, obs=VALID["obs"] + off) == E_ALIGN, off
    for off in (1, 2, 4):
        assert call(abi, name, variant, ball_xy=VALID["ball_xy"] + off) == E_ALIGN, off
    if not u8:
        for off in (2, 4, 8):
            assert call(abi, name, variant, layout=VALID["layout"] + off) == E_ALIGN, off


@pytest.mark.parametrize("name,variant", [c for c in CASES if "epoch_in" in ENTRIES[c[0]][0]])
def test_the_epoch_words(abi, name, variant):
    w = VALID["epoch_in"]
    assert call(abi, name, variant, epoch_in=w + 4) == E_ALIGN
    assert call(abi, name, variant, epoch_out=w + 12) == E_ALIGN
    assert call(abi, name, variant, epoch_in=w, epoch_out=w) == E_ALIGN          # the same word
    assert call(abi, name, variant, epoch_in=None) == E_ALIGN                    # out without in
    assert call(abi, name, variant, epoch_in=w + 8, epoch_out=w) == 0


def test_every_grid_step_entry_of_the_header_is_covered(abi):
    grid = [s for s in abi.SYMBOLS if s.startswith(("lmaze_step_", "lmaze_observe")) or s == "lmaze_reset"]
    assert sorted(grid) == sorted(ENTRIES)
