"""CPU: the refusals of the grid rollout entry points and their three describes (include/lmaze.h), their codes and their
order.  No device is needed and none is touched: every call of a launch entry is either refused or has T == 0 or n == 0,
which returns 0 before anything is queued, and the describes never queue anything.  Fabricated, aligned addresses stand
for the buffers.  Nothing is dereferenced.

The launch entries refuse in this order: (1) the recording request (the _obs and closed-loop entries), (2) the params --
NULL, grid, layout mode, count --, (3) the variant, (4) the narrow planes' own refusals -- layout, then G < 4 --, (5) T < 0,
(6) closed loop only: a key_mode outside {0, 1} (LMAZE_E_COUNT), then key_mode 1 on v0 (LMAZE_E_VARIANT); (7) T == 0 or
n == 0 returns 0 with nothing read; (8) LMAZE_E_NULL, the table among the pointers; (9) LMAZE_E_ALIGN, the thresholds' 16
bytes among them.  Each describe has an order of its own, stated at its tests."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
V0, V3 = 0, 3
SHARED, PER_ENV = 0, 1

# name -> (arguments behind params in the order of include/lmaze.h, narrow planes, the action source: the pointer that
# stands where the actions come from, and the alignment it must have (1: none)); "obs" / "obs_t" are obs8 / obs_t8 for
# the narrow entries
STATE = ("ball_xy", "goal_xy", "step_count", "reward", "done", "goal_count", "obs", "reward_t", "done_t")
TAIL = ("n", "auto_reset", "seed", "epoch", "env_base")
REC = ("obs_t", "obs_every")
OPEN = ("layout", "actions", "T") + STATE + TAIL
POLICY = ("layout", "policy", "key_mode", "epsilon", "T") + STATE + ("actions_t", "key_t") + TAIL + REC + ("stream",)
SAMPLE = ("layout", "thresholds", "key_mode", "T") + STATE + ("actions_t", "key_t") + TAIL + REC + ("stream",)
ENTRIES = {
    "lmaze_rollout": (OPEN + ("stream",), False, "actions", 1),
    "lmaze_rollout_obs": (OPEN + REC + ("stream",), False, "actions", 1),
    "lmaze_rollout_u8": (OPEN + ("stream",), True, "actions", 1),
    "lmaze_rollout_obs_u8": (OPEN + REC + ("stream",), True, "actions", 1),
    "lmaze_rollout_policy": (POLICY, False, "policy", 1),
    "lmaze_rollout_policy_u8": (POLICY, True, "policy", 1),
    "lmaze_rollout_sample": (SAMPLE, False, "thresholds", 16),
    "lmaze_rollout_sample_u8": (SAMPLE, True, "thresholds", 16),
}
DESCRIBES = ("lmaze_describe_rollout", "lmaze_describe_rollout_policy", "lmaze_describe_rollout_sample")
# fabricated addresses, each on a 4-KiB boundary; scalars.  T and n as a real call has them: a test that wants "nothing
# to do" says so
VALID = dict(layout=0x10000, actions=0x11000, policy=0x11000, thresholds=0x11000, ball_xy=0x12000, goal_xy=0x13000,
             step_count=0x14000, reward=0x15000, done=0x16000, goal_count=0x17000, obs=0x18000, reward_t=0x19000, done_t=0x1a000,
             actions_t=0x1b000, key_t=0x1c000, obs_t=None, obs_every=0, key_mode=0, epsilon=0, T=6, n=100, auto_reset=1, seed=7,
             epoch=3, env_base=0, stream=None)
# the documented alignments (ball_xy / goal_xy 8, the planes 16, the layout 16 unless the planes are narrow): the offset
# that breaks each
OFF = dict(ball_xy=4, goal_xy=4, obs=8, layout=1)

CASES = [(name, v) for name in ENTRIES for v in (V0, V3)]
RECORDING = [c for c in CASES if "obs_t" in ENTRIES[c[0]][0]]
CLOSED = [c for c in CASES if "key_mode" in ENTRIES[c[0]][0]]
NARROW = [c for c in CASES if ENTRIES[c[0]][1]]


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def check(abi, name, want, variant=V0, G=11, mode=SHARED, params=True, **over):
    """Call the launch entry `name` and require the code `want`.  want == 0 only with nothing to do: a call of this file
    never gets as far as a launch."""
    order = ENTRIES[name][0]
    args = dict(VALID, **over)
    assert want != 0 or args["T"] == 0 or args["n"] == 0, "a call of this file never gets as far as a launch"
    assert set(over) <= set(order), sorted(set(over) - set(order))
    p = abi.make_params(variant, G, mode, 50, -1.0, -0.01, 100.0)
    got = getattr(abi.lib, name)(C.byref(p) if params else None, *[args[k] for k in order])
    assert got == want, (name, variant, G, mode, params, over, got)


def required(name, variant):
    return ("layout", ENTRIES[name][2], "ball_xy", "step_count", "reward", "done") + (("goal_xy",) if variant == V3 else ())


# ---------------------------------------------------------------- the launch entries
@pytest.mark.parametrize("name,variant", CASES)
def test_nothing_to_do_returns_0_and_reads_no_pointer(abi, name, variant):
    order, u8, source, _ = ENTRIES[name]
    for T, n in ((0, 100), (6, 0), (0, 0)):
        check(abi, name, 0, variant, T=T, n=n)
        # (7) before (8) and (9): no pointer is missed, no alignment judged
        check(abi, name, 0, variant, T=T, n=n, **{k: None for k in required(name, variant)})
        check(abi, name, 0, variant, T=T, n=n, layout=None, ball_xy=VALID["ball_xy"] + 4)
        check(abi, name, 0, variant, T=T, n=n, ball_xy=VALID["ball_xy"] + 4, obs=VALID["obs"] + 8, **{source: VALID[source] + 4})
        for G in (3, 4, 64):
            if not (u8 and G == 3):
                check(abi, name, 0, variant, G=G, T=T, n=n)
        if not u8:
            check(abi, name, 0, variant, mode=PER_ENV, T=T, n=n)
        if "key_mode" in order and variant == V3:
            check(abi, name, 0, variant, key_mode=1, T=T, n=n)
    if "obs_t" in order:
        check(abi, name, 0, variant, T=0, obs_t=None, obs_every=3)              # T / every == 0 slots: none needed
        check(abi, name, 0, variant, n=0, T=2, obs_t=None, obs_every=3)
        check(abi, name, 0, variant, n=0, T=6, obs_t=0x20000, obs_every=3)


@pytest.mark.parametrize("name,variant", RECORDING)
def test_the_recording_request_is_refused_first(abi, name, variant):
    check(abi, name, E_COUNT, variant, obs_every=-1)
    check(abi, name, E_COUNT, variant, obs_t=0x20000, obs_every=0)
    check(abi, name, E_NULL, variant, obs_t=None, obs_every=3)
    check(abi, name, E_NULL, variant, obs_t=None, obs_every=6)
    check(abi, name, E_ALIGN, variant, obs_t=0x20000 + 8, obs_every=3)
    check(abi, name, E_ALIGN, variant, obs_t=0x20000 + 8, obs_every=7)          # misaligned, needed or not
    # ... its own order: the count, the missing slots, their alignment
    check(abi, name, E_COUNT, variant, obs_t=0x20000 + 8, obs_every=0)
    check(abi, name, E_COUNT, variant, obs_t=0x20000 + 8, obs_every=-1)
    # (1) before (2): NULL params, a bad grid, a bad count
    check(abi, name, E_ALIGN, variant, obs_t=0x20000 + 8, obs_every=3, params=False)
    check(abi, name, E_COUNT, variant, obs_every=-1, params=False)
    check(abi, name, E_NULL, variant, obs_t=None, obs_every=3, G=2)
    check(abi, name, E_ALIGN, variant, obs_t=0x20000 + 4, obs_every=3, n=-1)
    # ... and before everything behind: the variant, T < 0, nothing to do, the pointers
    check(abi, name, E_COUNT, 1, obs_every=-1)
    check(abi, name, E_ALIGN, variant, obs_t=0x20000 + 8, obs_every=3, T=-1)
    check(abi, name, E_COUNT, variant, obs_every=-1, n=0)
    check(abi, name, E_COUNT, variant, obs_t=0x20000, obs_every=0, T=0)
    check(abi, name, E_ALIGN, variant, obs_t=0x20000 + 8, obs_every=3, layout=None)


@pytest.mark.parametrize("name,variant", CASES)
def test_the_params_in_their_order(abi, name, variant):
    check(abi, name, E_NULL, variant, params=False)
    check(abi, name, E_GRID, variant, G=2)
    check(abi, name, E_GRID, variant, G=65)
    check(abi, name, E_LAYOUT, variant, mode=2)
    check(abi, name, E_LAYOUT, variant, mode=-1)
    check(abi, name, E_COUNT, variant, n=-1)
    check(abi, name, E_COUNT, variant, n=(1 << 30) + 1)
    # grid, layout mode, count: each pair, the earlier code
    check(abi, name, E_GRID, variant, G=2, mode=2)
    check(abi, name, E_LAYOUT, variant, mode=2, n=-1)
    check(abi, name, E_GRID, variant, G=65, mode=2, n=-1)
    # (2) before (3): the variant; and before everything behind
    check(abi, name, E_COUNT, 1, n=-1)
    check(abi, name, E_NULL, variant, params=False, T=-1)
    check(abi, name, E_NULL, variant, params=False, n=0)
    check(abi, name, E_LAYOUT, variant, mode=2, T=0)
    check(abi, name, E_GRID, variant, G=65, ball_xy=VALID["ball_xy"] + 4)
    check(abi, name, E_LAYOUT, 1, mode=2, layout=None)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_variant(abi, name):
    order, u8, source, _ = ENTRIES[name]
    for v in (1, 2, 4, 5, 6, 7, -1):
        check(abi, name, E_VARIANT, v)
        # (3) before (4): the narrow planes' refusals
        if u8:
            check(abi, name, E_VARIANT, v, mode=PER_ENV)
            check(abi, name, E_VARIANT, v, G=3)
        # ... before (5) T < 0, (6) the key mode, (7) nothing to do, (8) the pointers, (9) the alignments
        check(abi, name, E_VARIANT, v, T=-1)
        if "key_mode" in order:
            check(abi, name, E_VARIANT, v, key_mode=7)
        check(abi, name, E_VARIANT, v, n=0)
        check(abi, name, E_VARIANT, v, T=0)
        check(abi, name, E_VARIANT, v, **{source: None})
        check(abi, name, E_VARIANT, v, ball_xy=VALID["ball_xy"] + 4)


@pytest.mark.parametrize("name,variant", NARROW)
def test_the_narrow_planes_refuse_per_env_layouts_then_g3(abi, name, variant):
    order = ENTRIES[name][0]
    check(abi, name, E_LAYOUT, variant, mode=PER_ENV)
    check(abi, name, E_GRID, variant, G=3)
    check(abi, name, E_LAYOUT, variant, mode=PER_ENV, G=3)                      # the layout mode first
    # (4) before (5) T < 0, (6) the key mode, (7) nothing to do, (8) and (9)
    check(abi, name, E_GRID, variant, G=3, T=-1)
    check(abi, name, E_LAYOUT, variant, mode=PER_ENV, T=-1)
    if "key_mode" in order:
        check(abi, name, E_GRID, variant, G=3, key_mode=1 if variant == V0 else 7)
    check(abi, name, E_GRID, variant, G=3, n=0)
    check(abi, name, E_LAYOUT, variant, mode=PER_ENV, T=0)
    check(abi, name, E_LAYOUT, variant, mode=PER_ENV, layout=None)
    check(abi, name, E_GRID, variant, G=3, obs=VALID["obs"] + 8)


@pytest.mark.parametrize("name,variant", CASES)
def test_a_negative_t(abi, name, variant):
    order, _, source, _ = ENTRIES[name]
    check(abi, name, E_COUNT, variant, T=-1)
    # (5) before (6b): goal-keyed on v0; before (7), (8), (9)
    if "key_mode" in order:
        check(abi, name, E_COUNT, V0, T=-1, key_mode=1)
        check(abi, name, E_COUNT, variant, T=-1, key_mode=7)
    check(abi, name, E_COUNT, variant, T=-1, n=0)
    check(abi, name, E_COUNT, variant, T=-1, **{source: None})
    check(abi, name, E_COUNT, variant, T=-1, ball_xy=VALID["ball_xy"] + 4)


@pytest.mark.parametrize("name,variant", CLOSED)
def test_the_key_mode(abi, name, variant):
    source = ENTRIES[name][2]
    for km in (-1, 2, 7):
        check(abi, name, E_COUNT, variant, key_mode=km)
        # (6a) before (7), (8), (9): a bad argument is refused whether or not there is anything to do
        check(abi, name, E_COUNT, variant, key_mode=km, T=0)
        check(abi, name, E_COUNT, variant, key_mode=km, n=0)
        check(abi, name, E_COUNT, variant, key_mode=km, **{source: None})
        check(abi, name, E_COUNT, variant, key_mode=km, ball_xy=VALID["ball_xy"] + 4)
    if variant == V0:                                                            # (6b): v0 keeps no goal_xy
        check(abi, name, E_VARIANT, V0, key_mode=1)
        check(abi, name, E_VARIANT, V0, key_mode=1, T=0)
        check(abi, name, E_VARIANT, V0, key_mode=1, n=0)
        check(abi, name, E_VARIANT, V0, key_mode=1, **{source: None})
        check(abi, name, E_VARIANT, V0, key_mode=1, layout=VALID["layout"] + 1, obs=VALID["obs"] + 8)


@pytest.mark.parametrize("name,variant", CASES)
def test_each_required_pointer(abi, name, variant):
    order, u8, source, align = ENTRIES[name]
    key_modes = (0, 1) if "key_mode" in order and variant == V3 else (0,)
    for km in key_modes:
        kw = {"key_mode": km} if "key_mode" in order else {}
        for k in required(name, variant):
            check(abi, name, E_NULL, variant, **{k: None}, **kw)
            # (8) before (9): a NULL pointer together with a misaligned one
            other = "obs" if k == "ball_xy" else "ball_xy"
            check(abi, name, E_NULL, variant, **{k: None, other: VALID[other] + OFF[other]}, **kw)
            if align > 1 and k != source:
                check(abi, name, E_NULL, variant, **{k: None, source: VALID[source] + 4}, **kw)
        check(abi, name, E_NULL, variant, **{k: None for k in required(name, variant)}, **kw)
    if variant == V0:
        check(abi, name, E_NULL, variant, goal_xy=None, layout=None)             # v0 keeps no goal: not what is missed
        check(abi, name, E_ALIGN, variant, goal_xy=None, ball_xy=VALID["ball_xy"] + 4)


@pytest.mark.parametrize("name,variant", CASES)
def test_each_aligned_pointer(abi, name, variant):
    order, u8, source, align = ENTRIES[name]
    for k, off in OFF.items():
        if k == "layout" and u8:                                                 # the narrow entries read the layout by bytes
            continue
        check(abi, name, E_ALIGN, variant, **{k: VALID[k] + off})
    for off in (1, 2, 4, 8):
        check(abi, name, E_ALIGN, variant, obs=VALID["obs"] + off)
    for off in (1, 2, 4):
        check(abi, name, E_ALIGN, variant, ball_xy=VALID["ball_xy"] + off)
        check(abi, name, E_ALIGN, variant, goal_xy=VALID["goal_xy"] + off)       # judged on v0 too, when given
    if not u8:
        for off in (2, 4, 8):
            check(abi, name, E_ALIGN, variant, layout=VALID["layout"] + off)
    if align > 1:                                                                # the thresholds' 16 bytes
        for off in (1, 4, 8, 12):
            check(abi, name, E_ALIGN, variant, **{source: VALID[source] + off})
            if variant == V3:
                check(abi, name, E_ALIGN, variant, key_mode=1, **{source: VALID[source] + off})


# ---------------------------------------------------------------- the describes
def describe(abi, name, want, variant=V0, G=11, mode=SHARED, params=True, n=100, T=6, auto_reset=1, with_obs=1, obs_every=0,
             key_mode=0, text=True, length=256):
    """Call the describe `name`, require the code `want`, return the line (None without a text buffer)."""
    p = abi.make_params(variant, G, mode, 50, -1.0, -0.01, 100.0)
    buf = C.create_string_buffer(b"untouched", 256) if text else None
    mid = (key_mode,) if name != "lmaze_describe_rollout" else ()
    got = getattr(abi.lib, name)(C.byref(p) if params else None, n, T, auto_reset, with_obs, obs_every, *mid, buf, length)
    assert got == want, (name, variant, G, mode, params, n, T, with_obs, obs_every, key_mode, text, length, got)
    return buf.value.decode() if text else None


def test_describe_rollout_in_its_own_order(abi):
    """lmaze_describe_rollout: (1) the params and the variant, without the narrow planes' refusals, (2) T < 0, (3) a null or
    empty text buffer, (4) nothing to do: an empty line, (5) the narrow refusals, (6) obs_every < 0 means the plain form --
    no recording request is judged."""
    d = "lmaze_describe_rollout"
    for v in (V0, V3):
        assert describe(abi, d, 0, v).startswith("rollout_shared_kernel<v%d, obs_t> T=6 every=0 " % v)
        describe(abi, d, E_NULL, v, params=False)
        describe(abi, d, E_GRID, v, G=2)
        describe(abi, d, E_GRID, v, G=65)
        describe(abi, d, E_LAYOUT, v, mode=2)
        describe(abi, d, E_COUNT, v, n=-1)
        describe(abi, d, E_GRID, v, G=2, mode=2)
        describe(abi, d, E_LAYOUT, v, mode=2, n=-1)
        describe(abi, d, E_COUNT, v, T=-1)
        # (1) before (2), (3), (4), (5)
        describe(abi, d, E_NULL, v, params=False, T=-1)
        describe(abi, d, E_GRID, v, G=65, text=False)
        describe(abi, d, E_LAYOUT, v, mode=2, n=0)
        describe(abi, d, E_COUNT, v, n=-1, with_obs=2, mode=PER_ENV)
        # (2) before (3), (4), (5): here T is judged before the narrow planes, unlike the launch entries
        describe(abi, d, E_COUNT, v, T=-1, text=False)
        describe(abi, d, E_COUNT, v, T=-1, n=0)
        describe(abi, d, E_COUNT, v, T=-1, with_obs=2, mode=PER_ENV)
        describe(abi, d, E_COUNT, v, T=-1, with_obs=2, G=3)
        # (3) before (4), (5)
        describe(abi, d, E_NULL, v, text=False)
        describe(abi, d, E_NULL, v, length=0)
        describe(abi, d, E_NULL, v, text=False, n=0)
        describe(abi, d, E_NULL, v, length=0, T=0)
        describe(abi, d, E_NULL, v, text=False, with_obs=2, mode=PER_ENV)
        describe(abi, d, E_NULL, v, text=False, with_obs=2, G=3)
        # (4) before (5): nothing to do answers an empty line whatever the narrow planes would refuse
        for kw in (dict(n=0), dict(T=0), dict(n=0, T=0)):
            assert describe(abi, d, 0, v, **kw) == ""
            assert describe(abi, d, 0, v, with_obs=2, mode=PER_ENV, **kw) == ""
            assert describe(abi, d, 0, v, with_obs=2, G=3, **kw) == ""
        # (5) layout, then G < 4; the int32 planes take both
        describe(abi, d, E_LAYOUT, v, with_obs=2, mode=PER_ENV)
        describe(abi, d, E_GRID, v, with_obs=2, G=3)
        describe(abi, d, E_LAYOUT, v, with_obs=2, mode=PER_ENV, G=3)
        assert describe(abi, d, 0, v, mode=PER_ENV, G=3).startswith("rollout_perenv_kernel<v%d, obs_t> T=6 every=0 " % v)
        assert describe(abi, d, 0, v, with_obs=2).startswith("rollout_shared_u8_kernel<v%d, obs_t> T=6 every=0 " % v)
        # (6) any negative obs_every: the plain form; 0 and k > 0 the recording form, whatever T / k is
        for k in (-1, -5):
            assert describe(abi, d, 0, v, obs_every=k).startswith("rollout_shared_kernel<v%d> T=6 grid=" % v)
            assert describe(abi, d, 0, v, obs_every=k, with_obs=2).startswith("rollout_shared_u8_kernel<v%d> T=6 grid=" % v)
        assert describe(abi, d, 0, v, obs_every=3).startswith("rollout_shared_kernel<v%d, obs_t> T=6 every=3 " % v)
        assert describe(abi, d, 0, v, obs_every=7).startswith("rollout_shared_kernel<v%d, obs_t> T=6 every=7 " % v)
    for v in (1, 2, 4, 5, 6, -1):                                                # the variant: with the params
        describe(abi, d, E_VARIANT, v)
        describe(abi, d, E_VARIANT, v, T=-1)
        describe(abi, d, E_VARIANT, v, text=False)
        describe(abi, d, E_VARIANT, v, n=0)
        describe(abi, d, E_VARIANT, v, with_obs=2, mode=PER_ENV)
        describe(abi, d, E_COUNT, v, n=-1)


@pytest.mark.parametrize("d,form", [("lmaze_describe_rollout_policy", "policy=%s"), ("lmaze_describe_rollout_sample", "sample=%s, table=lds")])
def test_describe_closed_loop_in_its_own_order(abi, d, form):
    """lmaze_describe_rollout_policy / _sample: (1) obs_every < 0, (2) the text buffer, (3) the params, the variant, the
    narrow planes, T < 0 and the key mode as the launch entries judge them, then nothing to do: an empty line."""
    for v in (V0, V3):
        assert describe(abi, d, 0, v).startswith("rollout_shared_kernel<v%d, %s> T=6 every=0 " % (v, form % "ball"))
        describe(abi, d, E_COUNT, v, obs_every=-1)
        # (1) before (2) and (3)
        describe(abi, d, E_COUNT, v, obs_every=-1, text=False)
        describe(abi, d, E_COUNT, v, obs_every=-1, params=False)
        describe(abi, d, E_COUNT, v, obs_every=-1, G=2)
        describe(abi, d, E_COUNT, 1, obs_every=-1)
        # (2) before (3)
        describe(abi, d, E_NULL, v, text=False)
        describe(abi, d, E_NULL, v, length=0)
        describe(abi, d, E_NULL, v, text=False, G=2)
        describe(abi, d, E_NULL, v, text=False, mode=2)
        describe(abi, d, E_NULL, 1, text=False)
        describe(abi, d, E_NULL, v, text=False, T=-1)
        describe(abi, d, E_NULL, v, text=False, key_mode=7)
        describe(abi, d, E_NULL, v, length=0, n=0)
        # (3) in the launch entries' order
        describe(abi, d, E_NULL, v, params=False)
        describe(abi, d, E_GRID, v, G=2, mode=2)
        describe(abi, d, E_LAYOUT, v, mode=2, n=-1)
        describe(abi, d, E_COUNT, 1, n=-1)
        describe(abi, d, E_VARIANT, 1, with_obs=2, mode=PER_ENV)
        describe(abi, d, E_VARIANT, 2, T=-1)
        describe(abi, d, E_LAYOUT, v, with_obs=2, mode=PER_ENV, G=3)
        describe(abi, d, E_GRID, v, with_obs=2, G=3, T=-1)                        # the narrow planes before T, here
        describe(abi, d, E_LAYOUT, v, with_obs=2, mode=PER_ENV, n=0)
        describe(abi, d, E_COUNT, V0, T=-1, key_mode=1)
        describe(abi, d, E_COUNT, v, T=-1, n=0)
        for km in (-1, 2, 7):
            describe(abi, d, E_COUNT, v, key_mode=km)
            describe(abi, d, E_COUNT, v, key_mode=km, n=0)
            describe(abi, d, E_COUNT, v, key_mode=km, T=0)
        for kw in (dict(n=0), dict(T=0), dict(n=0, T=0)):
            assert describe(abi, d, 0, v, **kw) == ""
            assert describe(abi, d, 0, v, obs_every=3, **kw) == ""
    describe(abi, d, E_VARIANT, V0, key_mode=1)
    describe(abi, d, E_VARIANT, V0, key_mode=1, n=0)
    describe(abi, d, E_VARIANT, V0, key_mode=1, T=0)
    assert describe(abi, d, 0, V3, key_mode=1).startswith("rollout_shared_kernel<v3, %s> T=6 every=0 " % (form.replace("lds", "global") % "goal"))
    # no recording request is judged: k > T, and T / k == 0 slots
    assert describe(abi, d, 0, V0, obs_every=7).startswith("rollout_shared_kernel<v0, %s> T=6 every=7 " % (form % "ball"))
    assert describe(abi, d, 0, V0, obs_every=3).startswith("rollout_shared_kernel<v0, %s, obs_t> T=6 every=3 " % (form % "ball"))


def test_every_grid_rollout_entry_of_the_header_is_covered(abi):
    grid = [s for s in abi.SYMBOLS if s.startswith(("lmaze_rollout", "lmaze_describe_rollout"))]
    assert sorted(grid) == sorted(list(ENTRIES) + list(DESCRIBES))
