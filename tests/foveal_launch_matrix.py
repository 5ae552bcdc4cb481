"""The foveal launch-policy case table: which entry point, shape and LmazeFovealParams.launch_hint each GPU row of
test_gpu_foveal_launch_matrix.py runs against the C oracle, and the sweep of the launchers' own description
(lmaze_describe_foveal_step / lmaze_describe_foveal_rollout / lmaze_describe_foveal_rollout_obs) that
test_foveal_launch_matrix_cpu.py checks the table against.  The foveal twin of launch_matrix.py.

launch_hint is "performance only, never results" (include/lmaze.h).  For the foveal variants its fields pick envs per
workgroup 32-256 (another instantiation), 1-4 chunks per workgroup (the grid-stride loop over chunks), an LDS pad that
caps the workgroups per CU, and -- hint 0 past a size threshold -- a default the launcher substitutes itself; past
STREAM_BYTES of observation the step kernels also take their non-temporal stores.  The table must reach every kernel
the launchers can choose: the CPU test fails when the sweep names one that no row runs."""
import re
from collections import namedtuple

import numpy as np

# entry points.  STEP: T plain step launches; STEP_RESET: T launches of the fused reset (v1, v2, v4) or of the two-level
# step hier_step (v5, v6).  ROLLOUT / ROLLOUT_OBS: LmazeFovealVecEnv.rollout with resets -- fused (v1, v2, v4), two-level
# with goal rows (v5, v6) -- plain and recording; *_PLAIN: the same without resets (v5 / v6: T step launches, the only
# form their plain step has).
STEP, STEP_RESET = "step", "step_reset"
ROLLOUT, ROLLOUT_OBS, ROLLOUT_PLAIN, ROLLOUT_OBS_PLAIN = "rollout", "rollout_obs", "rollout_plain", "rollout_obs_plain"
ENTRIES = (STEP, STEP_RESET, ROLLOUT, ROLLOUT_OBS, ROLLOUT_PLAIN, ROLLOUT_OBS_PLAIN)
RECORDING = (ROLLOUT_OBS, ROLLOUT_OBS_PLAIN)
VARIANTS = ("v1", "v2", "v4", "v5", "v6")
TWO_LEVEL = ("v5", "v6")
CHANNELS = {"v1": 4, "v2": 5, "v4": 7, "v5": 7, "v6": 7}

# obs_every: None for the entry points that do not record
Row = namedtuple("Row", "entry variant G n_layouts N T obs_every hint")

STREAM_BYTES = 192 << 20            # observations beyond this are streamed ("nt": kFovealStreamBytes, lmaze_foveal_defs.h)
LDS_PER_WORKGROUP = 160 << 10       # gfx950
LDS_WITHOUT_DEVICE = 64 << 10       # what the launcher assumes when it cannot ask a device
MAX_LAYOUTS = 16
E_GRID, E_COUNT = -2, -5            # LMAZE_E_GRID, LMAZE_E_COUNT (include/lmaze.h)


def hint(per_cu=0, epb_code=0, chunks=1):
    """LmazeFovealParams.launch_hint from its fields: bits 0-3 workgroups per CU, bits 4-7 the envs-per-workgroup code
    (2: 32 ... 5: 256), bits 8-9 chunks per workgroup - 1"""
    assert 0 <= per_cu <= 15 and 0 <= epb_code <= 15 and 1 <= chunks <= 4
    return per_cu | (epb_code << 4) | ((chunks - 1) << 8)


def default_layouts(variant):
    return 1 if variant == "v1" else 5


def streaming_n(per_env_bytes):
    """the smallest odd N with N * per_env_bytes > STREAM_BYTES"""
    return (STREAM_BYTES // per_env_bytes + 1) | 1


def n_past_plain(variant):
    """past the plain step's (and v5 / v6's two-level step's) threshold, N C 100 B: nt set, default hint substituted"""
    return streaming_n(CHANNELS[variant] * 100)


N_PAST_FUSED = streaming_n(400)     # past the fused reset's threshold, N 400 B (v1, v2, v4)


def nt_set(variant, N):
    """the step launchers' runtime flag (not printed in the description): non-temporal observation stores"""
    return N * CHANNELS[variant] * 100 > STREAM_BYTES


# ---------------------------------------------------------------- the table
# 2571 = 10 * 256 + 11: at 256 envs x 4 chunks 11 chunks on 3 workgroups, 3 chunks in the last workgroup and 11 envs in the
# last chunk; odd, so ragged against every envs-per-workgroup size.  13 and 1 lie below one chunk; 32769 is the first
# size at which the rollouts take 64 envs per workgroup by default
N_RAGGED, N_SMALL, N_ONE, N_ROLL64 = 2571, 13, 1, 32769
STEP_GRIDS = (18, 14, 13, 33, 64)                 # the two specialisations; generic: off the 4x4 tile, above 32, the maximum
ROLL_GT = {"v1": 14, "v2": 18, "v4": 18, "v5": 18, "v6": 18}
# every envs-per-workgroup code the step reads (1 and 6: unsupported, the default) x chunks, and the cap values
STEP_CROSS = tuple(hint(0, c, m) for c in (1, 2, 3, 4, 5, 6) for m in (1, 2, 3, 4))
CAPS = (hint(2, 3, 1), hint(5, 2, 3), hint(8, 4, 2), hint(12, 5, 4), hint(2, 0, 1), hint(5, 0, 2), hint(1, 5, 1))
ROLL_CROSS = tuple(hint(0, c, m) for c in (1, 2, 3, 4, 5) for m in (1, 2, 3, 4))
SOME = (0, hint(0, 2, 4), hint(5, 3, 2), hint(0, 4, 3), hint(2, 5, 4), hint(9, 6, 2))


def _step_rows():
    rows = []
    for entry in (STEP, STEP_RESET):
        for v in ("v1", "v2", "v4", "v5"):
            L = default_layouts(v)
            for G in STEP_GRIDS:
                hints = (0,) + STEP_CROSS + CAPS if G in (18, 14, 13) else SOME + STEP_CROSS[4::5]
                rows += [Row(entry, v, G, L, N_RAGGED, 4, None, h) for h in hints]
            if v != "v1":
                # one layout, and the most: at G = 64 the layout tables alone are about 90 KiB of LDS, so the halving
                # fallback and the cap's pad meet
                for G, Ls in ((18, (1, MAX_LAYOUTS)), (13, (MAX_LAYOUTS,)), (64, (1, MAX_LAYOUTS))):
                    for Ln in Ls:
                        rows += [Row(entry, v, G, Ln, N_RAGGED, 4, None, h) for h in SOME + CAPS + STEP_CROSS[::4]]
            for N in (N_SMALL, N_ONE):
                rows += [Row(entry, v, ROLL_GT[v], L, N, 5, None, h) for h in (0,) + STEP_CROSS[::3] + CAPS[:2]]
            rows += [Row(entry, v, 13, L, N_SMALL, 5, None, h) for h in SOME]
        # v6: v5's kernels behind its own variant id
        for G, N in ((18, N_RAGGED), (13, N_RAGGED), (18, N_SMALL)):
            rows += [Row(entry, "v6", G, 5, N, 4, None, h) for h in SOME + STEP_CROSS[5::6]]
    # the streaming regime, T = 2: nt is a runtime flag every instantiation reads, so every size x chunks again at both
    # specialisations and one generic grid; hint 0 is where the launcher substitutes its own default
    stream = (0,) + tuple(hint(0, c, m) for c in (2, 3, 4, 5) for m in (1, 3)) + (hint(5, 3, 2),)
    for v in ("v1", "v2", "v4", "v5"):
        L = default_layouts(v)
        for G in (18, 14, 13):
            rows += [Row(STEP, v, G, L, n_past_plain(v), 2, None, h) for h in stream]
            # v2 / v4: between the two thresholds -- nt on, the fused reset's default hint not yet substituted
            rows += [Row(STEP_RESET, v, G, L, n_past_plain(v), 2, None, h) for h in stream]
        if v in ("v2", "v4"):
            rows += [Row(STEP_RESET, v, 18, L, N_PAST_FUSED, 2, None, h) for h in (0, hint(0, 2, 1), hint(5, 3, 2))]
    for entry in (STEP, STEP_RESET):
        rows += [Row(entry, "v6", 18, 5, n_past_plain("v6"), 2, None, h) for h in (0, hint(0, 2, 1), hint(5, 3, 2))]
    return rows


def _rollout_rows():
    rows = []
    for v in VARIANTS:
        L, GT = default_layouts(v), ROLL_GT[v]
        few = v == "v6"
        plain = () if v in TWO_LEVEL else (ROLLOUT_PLAIN,)
        for entry in (ROLLOUT,) + plain:
            for G in ((GT,) if few else (GT, 13, 33)):
                hints = (0,) + ROLL_CROSS + CAPS if G in (GT, 13) and not few else SOME + ROLL_CROSS[4::5]
                rows += [Row(entry, v, G, L, N_RAGGED, 6, None, h) for h in hints]
            if few:
                continue
            if v != "v1":
                for G, Ls in ((18, (1, MAX_LAYOUTS)), (64, (1, MAX_LAYOUTS))):
                    for Ln in Ls:
                        rows += [Row(entry, v, G, Ln, N_RAGGED, 5, None, h) for h in SOME + CAPS + ROLL_CROSS[::4]]
            else:
                rows += [Row(entry, v, 64, 1, N_RAGGED, 5, None, h) for h in SOME + CAPS]
            for N in (N_SMALL, N_ONE):
                rows += [Row(entry, v, GT, L, N, 7, None, h) for h in (0,) + ROLL_CROSS[::3]]
        # 32769 envs: 64 per workgroup by default
        rows += [Row(ROLLOUT, v, GT, L, N_ROLL64, 4, None, h) for h in (0, hint(0, 2, 3), hint(5, 4, 4))]
        if v == "v5":
            rows += [Row(ROLLOUT, v, 13, L, N_ROLL64, 4, None, h) for h in (0, hint(0, 3, 2))]     # off G = 18: forced to 32
        # the recording form: k = 3 leaves T % 3 steps unrecorded, k = 1 fills a slot every step; v5 / v6 with obs_local_t
        rec_entries = (ROLLOUT_OBS,) if v in TWO_LEVEL else (ROLLOUT_OBS, ROLLOUT_OBS_PLAIN)
        for entry in rec_entries:
            rows += [Row(entry, v, GT, L, N_RAGGED, 8, 3, h) for h in ((0,) + ROLL_CROSS + CAPS if not few else SOME)]
            rows += [Row(entry, v, GT, L, N_RAGGED, 4, 1, h) for h in SOME]
            if few:
                continue
            rows += [Row(entry, v, GT, L, N_SMALL, 7, 3, h) for h in (0,) + ROLL_CROSS[::3]]
            # off the specialised grid: v2 / v4 record in one launch (GT = 0), v1 and v5 / v6 are refused by the C layer
            # (LMAZE_E_GRID) and LmazeFovealVecEnv.rollout records through T step launches
            rows += [Row(entry, v, 13, L, N_RAGGED, 8, 3, h) for h in SOME + ROLL_CROSS[4:16]]
            if v in ("v2", "v4"):
                rows += [Row(entry, v, 64, MAX_LAYOUTS, N_RAGGED, 5, 3, h) for h in SOME + CAPS]
        rows += [Row(ROLLOUT_OBS, v, GT, L, N_ROLL64, 4, 3, h) for h in (0, hint(0, 4, 2))]
    # v5 / v6 without goals: rollout() is T launches of the plain step, recording by copies
    rows += [Row(ROLLOUT_PLAIN, "v5", 18, 5, N_RAGGED, 5, None, h) for h in SOME]
    rows += [Row(ROLLOUT_OBS_PLAIN, "v6", 18, 5, N_RAGGED, 7, 3, h) for h in SOME[:3]]
    # the streaming regime: 128 envs per workgroup by default for v1 / v2 / v4
    for v in ("v1", "v2", "v4", "v5"):
        rows += [Row(ROLLOUT, v, ROLL_GT[v], default_layouts(v), n_past_plain(v), 2, None, h)
                 for h in (0, hint(0, 2, 2), hint(5, 3, 1))]
    rows += [Row(ROLLOUT_OBS, "v2", 18, 5, n_past_plain("v2"), 2, 1, h) for h in (0, hint(0, 3, 2), hint(0, 2, 1))]
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
def params(abi, variant, G, n_layouts, launch_hint=0):
    """LmazeFovealParams as LmazeFovealVecEnv builds them (the description reads variant, grid, n_layouts, launch_hint)"""
    vid = {"v1": abi.VARIANT_V1, "v2": abi.VARIANT_V2, "v4": abi.VARIANT_V4, "v5": abi.VARIANT_V5, "v6": abi.VARIANT_V6}[variant]
    return abi.LmazeFovealParams(vid, G, n_layouts, 50, 10, -1.0, -0.01, 100.0, launch_hint)


def one_launch(entry, variant, G):
    """does LmazeFovealVecEnv.rollout run this entry as ONE launch (else: T step launches)?"""
    if entry in (STEP, STEP_RESET):
        return False
    if variant in TWO_LEVEL:
        return entry in (ROLLOUT, ROLLOUT_OBS) and (entry == ROLLOUT or G == 18)
    return entry not in RECORDING or variant != "v1" or G == 14


def describe(abi, entry, variant, G, n_layouts, N, T, obs_every, launch_hint):
    """what the launcher queues for this row: the rollout kernel, or the step kernel of each of its T launches"""
    p = params(abi, variant, G, n_layouts, launch_hint)
    resets = entry in (STEP_RESET, ROLLOUT, ROLLOUT_OBS)
    if not one_launch(entry, variant, G):
        return abi.describe_foveal_step(p, N, auto_reset=resets)
    return abi.describe_foveal_rollout(p, N, T, auto_reset=resets, two_level=variant in TWO_LEVEL,
                                       obs_every=obs_every if entry in RECORDING else None)


def field(text, name):
    return int(re.search(r"\b%s=(\d+)" % name, text).group(1))


def kernel_key(text, N, variant):
    """what selects GPU code in a description: the kernel's template arguments as printed (variant, mode, envs per
    workgroup, grid specialisation, plain / fused-reset / two-level, the recording form), whether a workgroup takes
    more than one chunk (the grid-stride loop runs again), and, step kernels, the runtime nt flag -- not printed:
    computed from N and the documented threshold (the rollouts never set it)"""
    m = re.match(r"(\w+)<([^>]*)>", text)
    name = m.group(1)
    nt = name == "foveal_kernel" and nt_set(variant, N)
    return "%s<%s>%s%s" % (name, m.group(2), " chunks>1" if field(text, "chunks") > 1 else "", " nt" if nt else "")


SWEEP_GRIDS = (5, 13, 14, 18, 33, 64)
SWEEP_LAYOUTS = (1, 5, MAX_LAYOUTS)
SWEEP_N = (1, 1000, 70000, 1 << 20)
SWEEP_HINTS = range(0x400)


def sweep(abi, grids=SWEEP_GRIDS, variants=VARIANTS):
    """(call, description) for every launch the describe sweep covers: the plain and the fused step, the plain, fused /
    two-level and recording rollouts, over every launch_hint 0..0x3ff.  call = (entry, variant, G, n_layouts, N, hint);
    description None where the C layer refuses the recording form (v1 off 14, v5 / v6 off 18)."""
    for variant in variants:
        two = variant in TWO_LEVEL
        for G in grids:
            for L in ((1,) if variant == "v1" else SWEEP_LAYOUTS):
                for n in SWEEP_N:
                    for h in SWEEP_HINTS:
                        p = params(abi, variant, G, L, h)
                        yield (STEP, variant, G, L, n, h), abi.describe_foveal_step(p, n, auto_reset=False)
                        yield (STEP_RESET, variant, G, L, n, h), abi.describe_foveal_step(p, n, auto_reset=True)
                        for entry in (ROLLOUT, ROLLOUT_OBS) + (() if two else (ROLLOUT_PLAIN, ROLLOUT_OBS_PLAIN)):
                            rec = entry in RECORDING
                            if rec and ((two and G != 18) or (variant == "v1" and G != 14)):
                                continue
                            yield ((entry, variant, G, L, n, h),
                                   abi.describe_foveal_rollout(p, n, 16, auto_reset=entry in (ROLLOUT, ROLLOUT_OBS),
                                                               two_level=two, obs_every=3 if rec else None))


def swept(abi):
    """{description: [calls]} of the whole sweep (about 1.5 million calls, some 50 000 distinct descriptions)"""
    out = {}
    for call, text in sweep(abi):
        out.setdefault(text, []).append(call)
    return out


def check_coverage(abi, by_text, floor):
    """every kernel_key the sweep names has a row in ROWS; by_text = swept(abi), under whatever LDS limit the launcher
    sees in this process (64 KiB without a device)"""
    where, seen = {}, set()
    for text, calls in by_text.items():
        for call in calls:
            nt = nt_set(call[1], call[4])
            if (text, nt) not in seen:                  # the key reads N and the variant for nt alone
                seen.add((text, nt))
                where.setdefault(kernel_key(text, call[4], call[1]), call)
    covered = {kernel_key(describe(abi, *r), r.N, r.variant) for r in ROWS}
    missing = sorted(set(where) - covered)
    assert not missing, "kernels no row of foveal_launch_matrix.ROWS runs (one call that picks each): " + "; ".join(
        "%s <- %s" % (k, where[k]) for k in missing)
    assert len(where) >= floor, len(where)            # the sweep still reaches what it did when the table was written


# ---------------------------------------------------------------- inputs of a GPU row
def layouts(G, count, seed, p_wall=0.2):
    """`count` random mazes of side G (uint8 character codes) with the 4-cell 'W' padding the teleporting variants need
    (lmaze_env_v2.py:309-326), one 'S' and one 'X' each"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        g = np.full((G, G), ord("W"), np.uint8)
        inner = np.where(rs.rand(G - 8, G - 8) < p_wall, ord("W"), ord("B")).astype(np.uint8)
        inner[0, 0], inner[-1, -1] = ord("S"), ord("X")
        g[4:-4, 4:-4] = inner
        out.append(g)
    return out
