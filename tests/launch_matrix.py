"""The launch-policy case table: which entry point, shape and LmazeParams.launch_hint each GPU row of
test_gpu_launch_matrix.py runs against the C oracle, and the sweep of the launchers' own description
(lmaze_describe_step / lmaze_describe_rollout) that test_launch_matrix_cpu.py checks the table against.

launch_hint is "performance only, never results" (include/lmaze.h): every hint field picks another kernel
instantiation or another envs-per-workgroup size, i.e. other GPU code.  The table must reach every one of them the
launchers can choose -- the CPU test fails when the sweep names a kernel that no row runs."""
import re
from collections import namedtuple

import numpy as np

# entry points: T step launches (with the fused reset or not), and the grid rollouts with auto_reset on
STEP, STEP_RESET = "step", "step_reset"
ROLLOUT, ROLLOUT_OBS, ROLLOUT_U8, ROLLOUT_OBS_U8 = "rollout", "rollout_obs", "rollout_u8", "rollout_obs_u8"
ENTRIES = (STEP, STEP_RESET, ROLLOUT, ROLLOUT_OBS, ROLLOUT_U8, ROLLOUT_OBS_U8)
SHARED, PER_ENV = "shared", "per_env"

# obs_every: None for the entry points that do not record
Row = namedtuple("Row", "entry variant layout G N T obs_every hint")

STREAM_BYTES = 192 << 20            # planes beyond this take the streaming ("nt") step kernels (lmaze_step.hip)
LDS_PER_WORKGROUP = 160 << 10       # gfx950
LDS_U8_ROLLOUT = 64 << 10           # what rollout_plan fits the u8 rollout into
STEP_LIMIT = 12                     # short episodes: resets inside every run


def hint(per_cu=0, chunks=0, bit8=False, no_stagger=False, sel=0, ro_epb=0, nt_slots=False):
    """LmazeParams.launch_hint from its fields (include/lmaze.h)"""
    return ((per_cu & 15) | ((chunks & 15) << 4) | (0x100 if bit8 else 0) | (0x200 if no_stagger else 0) | ((sel & 3) << 10)
            | ((ro_epb & 7) << 12) | (0x8000 if nt_slots else 0))


def streaming_n(G):
    """the smallest odd N whose int32 planes lie beyond STREAM_BYTES"""
    return ((STREAM_BYTES // (4 * G * G)) + 1) | 1


# ---------------------------------------------------------------- the table
# odd N: ragged against every envs-per-workgroup size (all powers of two), N G^2 odd at odd G (recorded slots start off a
# 16-byte boundary); 13 and 3 lie below most of the sizes
N_RAGGED, N_SMALL, N_TINY = 515, 13, 3
SPECIALISED = (8, 11, 12, 14, 18, 32)
GENERIC = (5, 21, 64)
SELS = {8: (0, 1, 2), 11: (0, 1, 2, 3), 12: (0, 1, 2, 3), 14: (0, 1, 2), 18: (0, 1, 2), 32: (0, 1, 2)}
POLICIES = (hint(1, 1), hint(3, 2), hint(8, 15), hint(5, 1, no_stagger=True), hint(2, 15, no_stagger=True), hint(0, 0, no_stagger=True))


def _sels(G):
    return SELS.get(G, (0, 1, 2, 3))


def _step_rows():
    rows = []
    for v in ("v0", "v3"):
        for entry in (STEP, STEP_RESET):
            # bits 10-11 at every specialised and a few generic sizes: the planes inside the caches ("plain" kernels);
            # 8x8 takes the workgroup kernel there only with bit 8, its wave-autonomous kernel reads bits 0-7 instead
            for G in SPECIALISED + GENERIC:
                b8 = G == 8
                for N in (N_RAGGED, N_TINY):
                    rows += [Row(entry, v, SHARED, G, N, 4, None, hint(sel=s, bit8=b8)) for s in _sels(G)]
                rows += [Row(entry, v, SHARED, G, N_RAGGED, 4, None, h | hint(sel=2, bit8=b8)) for h in POLICIES]
            rows += [Row(entry, v, SHARED, 8, N_RAGGED, 4, None, hint(wpb, epw)) for wpb, epw in ((1, 1), (2, 2), (4, 3), (0, 0))]
            rows += [Row(entry, v, SHARED, 8, 65537, 3, None, 0)]
            # per-env layouts: the register-tiled wave kernel (G^2 a multiple of 256) and the LDS kernel
            for G in (8, 9, 11, 12, 14, 16, 18, 32, 48, 64):
                rows.append(Row(entry, v, PER_ENV, G, N_RAGGED, 4, None, hint(3, 2)))
        # the streaming ("nt") instantiations: one step size past STREAM_BYTES, two steps, every selector and some policies
        for G in SPECIALISED + (64,):
            rows += [Row(STEP_RESET, v, SHARED, G, streaming_n(G), 2, None, hint(sel=s)) for s in _sels(G)]
            rows += [Row(STEP, v, SHARED, G, streaming_n(G), 2, None, h | hint(sel=1)) for h in POLICIES[:3]]
        for G in (16, 32, 48, 64):
            rows.append(Row(STEP_RESET, v, PER_ENV, G, streaming_n(G), 2, None, 0))
    return rows


def _rollout_rows():
    rows = []
    for v in ("v0", "v3"):
        # shared layouts, envs per workgroup 4-256 (bits 12-14), plain and recording (k = 3 leaves T % 3 steps unrecorded,
        # k = 0 the final planes only), bit 15 on the recording form, and bit 8 / T = 1 (the T-launch fallback)
        for G, N in ((11, N_RAGGED), (11, N_SMALL), (32, N_RAGGED), (5, N_RAGGED)):
            for k in range(8):
                rows.append(Row(ROLLOUT, v, SHARED, G, N, 9, None, hint(ro_epb=k)))
                rows.append(Row(ROLLOUT_OBS, v, SHARED, G, N, 8, 3, hint(ro_epb=k)))
                rows.append(Row(ROLLOUT_OBS, v, SHARED, G, N, 8, 3, hint(ro_epb=k, nt_slots=True)))
            rows.append(Row(ROLLOUT_OBS, v, SHARED, G, N, 8, 0, 0))
            rows.append(Row(ROLLOUT, v, SHARED, G, N, 9, None, hint(bit8=True)))
            rows.append(Row(ROLLOUT_OBS, v, SHARED, G, N, 8, 3, hint(bit8=True)))
        rows.append(Row(ROLLOUT, v, SHARED, 11, N_RAGGED, 1, None, 0))
        rows.append(Row(ROLLOUT_OBS, v, SHARED, 11, N_RAGGED, 1, 1, 0))
        # 8x8: the wave-autonomous rollout (one wave per workgroup, four from 65 536 envs on); bit 8 leaves it
        for N in (N_RAGGED, 65539):
            rows.append(Row(ROLLOUT, v, SHARED, 8, N, 7, None, 0))
            rows.append(Row(ROLLOUT_OBS, v, SHARED, 8, N, 7, 3, 0))
        rows.append(Row(ROLLOUT, v, SHARED, 8, N_RAGGED, 7, None, hint(ro_epb=3, bit8=True)))
        # per-env layouts: 4-64 envs per workgroup; past G = 50 the LDS caps 64 at 32
        for G, N in ((11, N_RAGGED), (11, N_SMALL), (32, N_RAGGED), (51, 131), (64, 131)):
            for k in range(8):
                rows.append(Row(ROLLOUT, v, PER_ENV, G, N, 9, None, hint(ro_epb=k)))
                rows.append(Row(ROLLOUT_OBS, v, PER_ENV, G, N, 8, 3, hint(ro_epb=k)))
                rows.append(Row(ROLLOUT_OBS, v, PER_ENV, G, N, 8, 3, hint(ro_epb=k, nt_slots=True)))
        # the u8 rollouts: 16-256 envs per workgroup
        for G, N in ((11, N_RAGGED), (11, N_SMALL), (4, N_RAGGED), (64, N_RAGGED)):
            for k in range(8):
                rows.append(Row(ROLLOUT_U8, v, SHARED, G, N, 9, None, hint(ro_epb=k)))
                rows.append(Row(ROLLOUT_OBS_U8, v, SHARED, G, N, 8, 3, hint(ro_epb=k)))
            rows.append(Row(ROLLOUT_OBS_U8, v, SHARED, G, N, 8, 0, 0))
    return rows


ROWS = _step_rows() + _rollout_rows()


def group_key(r):
    """rows that differ in launch_hint only: one env, one oracle run"""
    return r[:-1]


def groups():
    out = {}
    for r in ROWS:
        out.setdefault(group_key(r), []).append(r.hint)
    return out


# ---------------------------------------------------------------- the launcher's description
def params(abi, variant, G, layout, launch_hint=0, step_limit=STEP_LIMIT):
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else abi.VARIANT_V0, G,
                        abi.LAYOUT_PER_ENV if layout == PER_ENV else abi.LAYOUT_SHARED, step_limit, -1.0, -0.01, 100.0)
    p.launch_hint = launch_hint
    return p


def describe(abi, entry, variant, layout, G, N, T, obs_every, launch_hint, auto_reset=True):
    """what the launcher would queue for this row (lmaze_describe_step / lmaze_describe_rollout)"""
    p = params(abi, variant, G, layout, launch_hint)
    if entry in (STEP, STEP_RESET):
        return abi.describe_step(p, N, auto_reset=entry == STEP_RESET, with_obs=True)
    return abi.describe_rollout(p, N, T, auto_reset=auto_reset, with_obs="u8" if entry.endswith("u8") else True,
                                obs_every=obs_every)


def field(text, name):
    return int(re.search(r"\b%s=(\d+)" % name, text).group(1))


def kernel_key(text):
    """the kernel instantiation a description names: the step kernels' template arguments as printed; the rollout
    kernels (one template each for v0 / v3, folded together) with their recording / slot-store form and envs per
    workgroup"""
    m = re.match(r"(\w+)<([^>]*)>", text)
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    if not name.startswith("rollout_"):
        return "%s<%s>" % (name, ", ".join(args))
    return "%s<%s> epb=%d" % (name, ", ".join(args[1:]), field(text, "envs_per_workgroup"))


SWEEP_GRIDS = (3, 4, 5, 8, 9, 11, 12, 14, 16, 18, 21, 32, 33, 48, 64)
SWEEP_N = (1, 1000, 70000, 1 << 20)
STEP_HINTS = tuple(hint(c & 15, c >> 4, bit8=b8, sel=s) for c in (0, 0x11, 0x22, 0x34) for b8 in (False, True) for s in range(4))
ROLLOUT_HINTS = tuple(hint(bit8=b8, ro_epb=k, nt_slots=nt) for b8 in (False, True) for k in range(8) for nt in (False, True))


def sweep(abi, grids=SWEEP_GRIDS, ns=SWEEP_N):
    """(call, description) for every launch the describe sweep covers: the step entry points over bits 0-11 (those
    that select: the wave-autonomous kernel's 4-7, bit 8, bits 10-11), with and without planes; the grid rollouts over
    bits 8 and 12-15, T = 1 and 16, plain / recording (k = 3, k = 0) / u8, auto_reset on and off."""
    for variant in ("v0", "v3"):
        for layout in (SHARED, PER_ENV):
            for G in grids:
                for n in ns:
                    for h in STEP_HINTS:
                        p = params(abi, variant, G, layout, h)
                        for ar in (False, True):
                            for with_obs in (False, True):
                                yield (("step", variant, layout, G, n, h, ar, with_obs),
                                       abi.describe_step(p, n, auto_reset=ar, with_obs=with_obs))
                    for h in ROLLOUT_HINTS:
                        p = params(abi, variant, G, layout, h)
                        for T in (1, 16):
                            for ar in (False, True):
                                for with_obs in (False, True, "u8"):
                                    if with_obs == "u8" and (layout == PER_ENV or G < 4):
                                        continue
                                    for k in (None, 0, 3):
                                        yield (("rollout", variant, layout, G, n, h, T, ar, with_obs, k),
                                               abi.describe_rollout(p, n, T, auto_reset=ar, with_obs=with_obs, obs_every=k))


# ---------------------------------------------------------------- inputs of a GPU row
def layouts(n, G, seed, p_wall=0.2):
    """uint8[n,G,G] bordered random mazes with one 'X' and one 'S' each (vectorised: per-env batches of 10^5)"""
    rs = np.random.RandomState(seed)
    lay = np.where(rs.rand(n, G, G) < p_wall, ord("W"), ord("B")).astype(np.uint8)
    lay[:, 0, :] = lay[:, -1, :] = lay[:, :, 0] = lay[:, :, -1] = ord("W")
    x = rs.randint(1, G - 1, (n, 2))
    s = np.where((x == 1).all(1, keepdims=True), G - 2, 1) * np.ones((1, 2), np.int64)
    idx = np.arange(n)
    lay[idx, x[:, 0], x[:, 1]] = ord("X")
    lay[idx, np.where(x[:, 0] > 1, x[:, 0] - 1, x[:, 0] + 1), x[:, 1]] = ord("B")    # a way into the goal
    lay[idx, s[:, 0], s[:, 1]] = ord("S")
    return lay
