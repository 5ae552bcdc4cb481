"""CPU: the refusals of the foveal step, reset, goal and visit-map entry points (include/lmaze.h), their codes and their
order -- the foveal twin of test_step_entries_cpu.py.  No device is needed and none is touched: every call passes n = 0
(or n < 0), so a call that is not refused returns 0 from the launcher before anything is queued -- the refusals all stand
before that -- and a real LmazeFovealBuffers holds fabricated, aligned addresses.  Nothing is dereferenced.

The order is recorded as it is, uneven places included: v5/v6 answer a misaligned obs_local before the NULLs of the
buffers every variant needs; a misaligned visit is refused for the variants that keep no visit map too; an entry's own
variant refusal and its own pointers stand behind every refusal of the buffers; the visit-map pair looks at neither the
variant, n_layouts nor launch_hint."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
V1, V2, V4, V5, V6 = 1, 2, 4, 5, 6
FOVEAL = (V1, V2, V4, V5, V6)
NOT_FOVEAL = (0, 3, 7, -1)

RESET = ("seed", "epoch", "env_base", "epoch_in", "epoch_out")
# name -> (arguments behind params in the order of include/lmaze.h, variants taken, the entry's own pointers that must
# not be NULL)
ENTRIES = {
    "lmaze_foveal_step": (("layouts", "action", "bufs", "n", "stream"), FOVEAL, ("action",)),
    "lmaze_foveal_step_autoreset": (("layouts", "action", "bufs", "n") + RESET + ("stream",), (V1, V2, V4), ("action",)),
    "lmaze_v5_hier_step": (("layouts", "action", "planner_goal", "bufs", "n") + RESET + ("stream",), (V5, V6),
                           ("action", "planner_goal")),
    "lmaze_foveal_reset": (("layouts", "mask", "place", "seed", "epoch", "env_base", "bufs", "n", "stream"), FOVEAL, ()),
    "lmaze_v1_set_foveal_goal": (("layouts", "ij", "mask", "bufs", "n", "stream"), (V1,), ("ij",)),
    "lmaze_v5_planner_step": (("layouts", "goal", "mask", "bufs", "n", "stream"), (V5, V6), ("goal",)),
    "lmaze_v6_safe_foveal_goal": (("layouts", "seed", "epoch", "env_base", "bufs", "out_goal", "n", "stream"), (V5, V6),
                                  ("out_goal",)),
}
# the visit-map pair: (params, bufs, out / in, n, stream), checks of their own
VISIT = ("lmaze_foveal_materialise_visit", "lmaze_foveal_load_visit")

# fabricated addresses, each on a 4-KiB boundary; scalars
VALID = dict(layouts=0x10000, action=0x11000, planner_goal=0x12000, ij=0x13000, goal=0x14000, out_goal=0x15000, mask=0x16000,
             epoch_in=0x1a000, epoch_out=0x1a008, n=0, stream=None, seed=7, epoch=3, env_base=0, place=1, other=0x1b000)
COMMON = ("ball_xy", "step_count", "reward", "done", "obs")
FGOAL = ("fgoal_xy", "foveal_step_count", "foveal_reward", "foveal_done")
TWO_LEVEL = FGOAL + ("visit", "ball1_xy", "fovea_xy", "last_xy", "foveal_goal", "obs_local")
# the buffer fields each variant family needs, in the order the refusals look at them
REQUIRED = {V1: COMMON + FGOAL, V2: COMMON + ("goal_xy", "layout_id"), V4: COMMON + ("goal_xy", "layout_id", "visit", "visit_clock")}
REQUIRED[V5] = REQUIRED[V6] = TWO_LEVEL + COMMON + ("goal_xy", "layout_id", "visit_clock")

CASES = [(name, v) for name, e in ENTRIES.items() for v in e[1]]


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def buffers(abi, **over):
    """an LmazeFovealBuffers of fabricated 4-KiB-aligned addresses; over: field -> address, None or an offset ("+8")"""
    fields = {f: 0x100000 + 0x1000 * i for i, f in enumerate(abi.FOVEAL_BUFFER_FIELDS)}
    for k, v in over.items():
        fields[k] = fields[k] + int(v) if isinstance(v, str) else v
    return abi.LmazeFovealBuffers(**fields)


def call(abi, name, variant, G=13, L=5, hint=0, params=True, bufs=True, fields=None, **over):
    assert over.get("n", 0) <= 0, "a call of this file never gets as far as a launch"
    p = abi.LmazeFovealParams(variant, G, L, 50, 10, -1.0, -0.01, 100.0, hint)
    b = buffers(abi, **(fields or {}))
    args = dict(VALID, bufs=C.byref(b) if bufs else None, **over)
    order = ENTRIES[name][0] if name in ENTRIES else ("bufs", "other", "n", "stream")
    return getattr(abi.lib, name)(C.byref(p) if params else None, *[args[k] for k in order])


@pytest.mark.parametrize("name,variant", CASES)
def test_valid_arguments_with_no_envs_return_0(abi, name, variant):
    order = ENTRIES[name][0]
    assert call(abi, name, variant) == 0
    if "mask" in order:
        assert call(abi, name, variant, mask=None) == 0
    # the buffer fields the variant does not keep are optional
    spare = {f: None for f in abi.FOVEAL_BUFFER_FIELDS if f not in REQUIRED[variant]}
    assert call(abi, name, variant, fields=spare) == 0
    if "epoch_in" in order:
        assert call(abi, name, variant, epoch_in=None, epoch_out=None) == 0
        assert call(abi, name, variant, epoch_out=None) == 0
    for G in (5, 14, 18, 64):
        assert call(abi, name, variant, G=G) == 0, G
    for L in (1, 16):
        assert call(abi, name, variant, L=L) == 0, L
    for hint in (0x35, 0x220, 0x3ff):
        assert call(abi, name, variant, hint=hint) == 0, hint


@pytest.mark.parametrize("name,variant", CASES)
def test_params_are_refused_first(abi, name, variant):
    assert call(abi, name, variant, params=False) == E_NULL
    assert call(abi, name, variant, layouts=None) == E_NULL
    assert call(abi, name, variant, bufs=False) == E_NULL
    for v in NOT_FOVEAL:
        assert call(abi, name, v) == E_VARIANT, v
    assert call(abi, name, variant, G=4) == E_GRID
    assert call(abi, name, variant, G=65) == E_GRID
    assert call(abi, name, variant, L=0) == E_LAYOUT
    assert call(abi, name, variant, L=17) == E_LAYOUT
    assert call(abi, name, variant, n=-1) == E_COUNT
    assert call(abi, name, variant, hint=0x400) == E_LAYOUT
    assert call(abi, name, variant, hint=-1) == E_LAYOUT
    # ... in that order, and before every buffer
    assert call(abi, name, 3, G=4, layouts=None) == E_NULL
    assert call(abi, name, 3, G=4, L=0, n=-1, hint=0x400) == E_VARIANT
    assert call(abi, name, variant, G=4, L=0, n=-1, hint=0x400) == E_GRID
    assert call(abi, name, variant, L=17, n=-1, hint=0x400) == E_LAYOUT
    assert call(abi, name, variant, n=-1, hint=0x400) == E_COUNT
    assert call(abi, name, variant, n=-1, fields=dict(ball_xy=None)) == E_COUNT
    assert call(abi, name, variant, hint=0x400, fields=dict(ball_xy=None)) == E_LAYOUT
    assert call(abi, name, variant, hint=0x400, fields=dict(obs="+4")) == E_LAYOUT


@pytest.mark.parametrize("name,variant", CASES)
def test_each_required_buffer_field(abi, name, variant):
    for f in REQUIRED[variant]:
        assert call(abi, name, variant, fields={f: None}) == E_NULL, f
        # a NULL field together with a misaligned obs: LMAZE_E_NULL
        if f != "obs":
            assert call(abi, name, variant, fields={f: None, "obs": "+8"}) == E_NULL, f
    # v5/v6 judge their own fields and obs_local's alignment before the fields every variant needs
    two = variant in (V5, V6)
    assert call(abi, name, variant, fields=dict(ball_xy=None, obs_local="+8")) == (E_ALIGN if two else E_NULL)
    assert call(abi, name, variant, fields=dict(fgoal_xy=None, obs_local="+8")) == (E_NULL if two or variant == V1 else 0)


@pytest.mark.parametrize("name,variant", CASES)
def test_each_aligned_buffer_field(abi, name, variant):
    for off in (1, 2, 4, 8):
        assert call(abi, name, variant, fields=dict(obs="+%d" % off)) == E_ALIGN, off
    # a visit map that is given is judged, whether or not the variant keeps one: a tile is one 64-byte sector
    for off in (4, 16, 32):
        assert call(abi, name, variant, fields=dict(visit="+%d" % off)) == E_ALIGN, off
    for off in (4, 8):
        assert call(abi, name, variant, fields=dict(obs_local="+%d" % off)) == (E_ALIGN if variant in (V5, V6) else 0), off
    # the entry's own pointers stand behind the buffers' alignment
    for k in ENTRIES[name][2]:
        assert call(abi, name, variant, fields=dict(obs="+8"), **{k: None}) == E_ALIGN, k


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_entry_variant_stands_between_the_buffers_and_the_entry_pointers(abi, name):
    _, variants, own = ENTRIES[name]
    for v in [v for v in FOVEAL if v not in variants]:
        assert call(abi, name, v) == E_VARIANT, v
        # behind every refusal of the params and the buffers, which are judged for the variant given ...
        assert call(abi, name, v, n=-1) == E_COUNT, v
        assert call(abi, name, v, hint=0x400) == E_LAYOUT, v
        for f in REQUIRED[v]:
            assert call(abi, name, v, fields={f: None}) == E_NULL, (v, f)
        assert call(abi, name, v, fields=dict(obs="+8")) == E_ALIGN, v
        # ... and before the entry's own pointers and epoch words
        for k in own:
            assert call(abi, name, v, **{k: None}) == E_VARIANT, (v, k)
        if "epoch_in" in ENTRIES[name][0]:
            assert call(abi, name, v, epoch_in=VALID["epoch_in"] + 4) == E_VARIANT, v


@pytest.mark.parametrize("name,variant", CASES)
def test_the_entry_pointers(abi, name, variant):
    order, _, own = ENTRIES[name]
    for k in own:
        assert call(abi, name, variant, **{k: None}) == E_NULL, k
        if "epoch_in" in order:
            assert call(abi, name, variant, **{k: None, "epoch_in": VALID["epoch_in"] + 4}) == E_NULL, k


@pytest.mark.parametrize("name,variant", [c for c in CASES if "epoch_in" in ENTRIES[c[0]][0]])
def test_the_epoch_words(abi, name, variant):
    w = VALID["epoch_in"]
    assert call(abi, name, variant, epoch_in=w + 4) == E_ALIGN
    assert call(abi, name, variant, epoch_out=w + 12) == E_ALIGN
    assert call(abi, name, variant, epoch_in=w, epoch_out=w) == E_ALIGN          # the same word
    assert call(abi, name, variant, epoch_in=None) == E_ALIGN                    # out without in
    assert call(abi, name, variant, epoch_in=w + 8, epoch_out=w) == 0


@pytest.mark.parametrize("name", VISIT)
def test_the_visit_map_pair(abi, name):
    for v in FOVEAL + NOT_FOVEAL:                                   # the variant is not looked at, nor n_layouts, nor the hint
        assert call(abi, name, v) == 0, v
    assert call(abi, name, V4, L=0) == 0
    assert call(abi, name, V4, L=17, hint=0x400) == 0
    spare = {f: None for f in abi.FOVEAL_BUFFER_FIELDS if f not in ("visit", "visit_clock")}
    assert call(abi, name, V4, fields=spare) == 0
    assert call(abi, name, V4, params=False) == E_NULL
    assert call(abi, name, V4, bufs=False) == E_NULL
    assert call(abi, name, V4, other=None) == E_NULL
    assert call(abi, name, V4, fields=dict(visit=None)) == E_NULL
    assert call(abi, name, V4, fields=dict(visit_clock=None)) == E_NULL
    assert call(abi, name, V4, G=4) == E_GRID
    assert call(abi, name, V4, G=65) == E_GRID
    assert call(abi, name, V4, n=-1) == E_COUNT
    for off in (4, 16, 32):
        assert call(abi, name, V4, fields=dict(visit="+%d" % off)) == E_ALIGN, off
    for off in (1, 2):
        assert call(abi, name, V4, other=VALID["other"] + off) == E_ALIGN, off
    assert call(abi, name, V4, other=VALID["other"] + 4) == 0
    # NULL, grid, count, alignment: in that order
    assert call(abi, name, V4, G=4, n=-1, other=None) == E_NULL
    assert call(abi, name, V4, G=4, n=-1, fields=dict(visit="+4")) == E_GRID
    assert call(abi, name, V4, n=-1, fields=dict(visit="+4")) == E_COUNT


def describe_step(abi, variant, n, G=13, L=5, hint=0, auto_reset=0, params=True, text=True, length=256):
    p = abi.LmazeFovealParams(variant, G, L, 50, 10, -1.0, -0.01, 100.0, hint)
    buf = C.create_string_buffer(b"x" * 255, 256)
    rc = abi.lib.lmaze_describe_foveal_step(C.byref(p) if params else None, n, auto_reset, buf if text else None, length)
    return rc, buf.value.decode()


@pytest.mark.parametrize("variant", FOVEAL)
def test_the_step_describe(abi, variant):
    assert describe_step(abi, variant, 0) == (0, "")
    assert describe_step(abi, variant, 0, auto_reset=1) == (0, "")
    assert describe_step(abi, variant, 0, hint=0x400) == (0, "")    # the describe does not look at the hint's range
    assert describe_step(abi, variant, -1, hint=-1)[0] == E_COUNT
    assert describe_step(abi, variant, 0, params=False)[0] == E_NULL
    assert describe_step(abi, variant, 0, text=False)[0] == E_NULL
    assert describe_step(abi, variant, 0, length=0)[0] == E_NULL
    for v in NOT_FOVEAL:
        assert describe_step(abi, v, 0)[0] == E_VARIANT, v
    assert describe_step(abi, variant, 0, G=4)[0] == E_GRID
    assert describe_step(abi, variant, 0, G=65)[0] == E_GRID
    assert describe_step(abi, variant, 0, L=0)[0] == E_LAYOUT
    assert describe_step(abi, variant, 0, L=17)[0] == E_LAYOUT
    assert describe_step(abi, variant, -1)[0] == E_COUNT
    # NULL, variant, grid, n_layouts, count: in that order; a refusal leaves the text alone
    assert describe_step(abi, 3, -1, G=4, L=0, length=0)[0] == E_NULL
    assert describe_step(abi, 3, -1, G=4, L=0) == (E_VARIANT, "x" * 255)
    assert describe_step(abi, variant, -1, G=4, L=0)[0] == E_GRID
    assert describe_step(abi, variant, -1, L=17)[0] == E_LAYOUT


def test_the_visit_bytes(abi):
    f = abi.lib.lmaze_foveal_visit_bytes
    assert f(18, 0) == 0 and f(0, 10) == 0 and f(65, 10) == 0 and f(18, -1) == 0
    assert f(18, 3) == 3 * (5 * 5 * 16 + 28) * 4 and f(1, 1) == (16 + 28) * 4


def test_every_foveal_entry_of_the_header_is_covered(abi):
    foveal = [s for s in abi.SYMBOLS if ("foveal" in s or s.startswith(("lmaze_v5_", "lmaze_v6_"))) and "rollout" not in s]
    others = ["lmaze_describe_foveal_step", "lmaze_foveal_visit_bytes"]          # test_the_step_describe, test_the_visit_bytes
    assert sorted(foveal) == sorted(list(ENTRIES) + list(VISIT) + others)
