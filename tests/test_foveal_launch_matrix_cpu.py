"""CPU: the foveal launch-policy table of foveal_launch_matrix.py against the launchers' own description (no GPU).
Every kernel the describe sweep names -- instantiation, more than one chunk per workgroup, non-temporal stores -- is run
by some GPU row (test_gpu_foveal_launch_matrix.py), and every plan of the sweep is one a gfx950 workgroup can launch:
LDS within 160 KiB and the grid covering the batch.

Without a device the launcher takes 64 KiB as the LDS a workgroup may ask for, so its halving fallback lands elsewhere
than on an MI355X: this module checks the coverage under that limit, the GPU module repeats the assertion under the
device's, and the table covers the union."""
import importlib
import os
import subprocess

import pytest

import foveal_launch_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


@pytest.fixture(scope="module")
def swept(abi):
    return M.swept(abi)


def test_every_kernel_the_sweep_names_has_a_gpu_row(abi, swept):
    M.check_coverage(abi, swept, 480)


def test_every_plan_of_the_sweep_is_launchable(swept):
    for text, calls in swept.items():
        lds, epb, grid, chunks = (M.field(text, f) for f in ("lds", "envs_per_workgroup", "grid", "chunks"))
        assert lds <= M.LDS_PER_WORKGROUP, (calls[0], text)
        assert grid >= 1 and 1 <= chunks <= 4 and M.field(text, "block") == 256, (calls[0], text)
        rollout = text.startswith("foveal_rollout_kernel")
        assert epb in ((32, 64, 128) if rollout else (32, 64, 128, 256)), (calls[0], text)
        for call in calls:
            n = call[4]
            assert grid * epb * chunks >= n, (call, text)
            assert (grid - 1) * chunks * epb < n + epb, (call, text)       # and no workgroup without a chunk


def test_the_cap_is_reported_when_the_pad_took_effect(abi, swept):
    """bits 0-3 pad the dynamic LDS up to a size that caps the workgroups per CU, and only ever upwards; a rollout's
    description names the cap exactly when the pad took effect (the step's: whenever the pad is at least considered)"""
    by_call = {call: text for text, calls in swept.items() for call in calls}
    parsed = {text: (M.field(text, "workgroups_per_cu"), M.field(text, "lds"), text.split("<")[1].split(">")[0]) for text in swept}
    checked = 0
    for call, text in by_call.items():
        entry, variant, G, L, n, h = call
        if not h & 15:
            if h == 0:                  # the launcher may substitute its own default, cap included
                continue
            assert parsed[text][0] == 0, (call, text)
            continue
        bare = by_call[(entry, variant, G, L, n, h & ~15)]
        if h == (h & 0xf):              # hint = cap bits only: not hint 0, so the launcher substitutes no default
            bare = None
        wpc, lds, kernel = parsed[text]
        assert wpc in (0, h & 15) and (wpc == 0 or wpc <= 8), (call, text)
        if bare is None:
            continue
        assert kernel == parsed[bare][2], (call, text, bare)
        lds0 = parsed[bare][1]
        assert lds >= lds0, (call, text, bare)
        if text.startswith("foveal_rollout_kernel"):
            assert (wpc != 0) == (lds > lds0), (call, text, bare)
        elif lds > lds0:
            assert wpc == (h & 15), (call, text, bare)
        checked += 1
    assert checked > 500000


def test_unsupported_size_codes_take_the_default(abi):
    """bits 4-7 outside 2-5 (step) / 2-4 (rollout) pick no size: the description is that of code 0"""
    checked = 0
    for variant in M.VARIANTS:
        two = variant in M.TWO_LEVEL
        for G in M.SWEEP_GRIDS:
            for L in ((1,) if variant == "v1" else M.SWEEP_LAYOUTS):
                for n in M.SWEEP_N:
                    for rest in (M.hint(1, 0, 1), M.hint(0, 0, 2), M.hint(5, 0, 4), M.hint(9, 0, 3)):   # hint 0 substitutes
                        for ar in (False, True):
                            want = abi.describe_foveal_step(M.params(abi, variant, G, L, rest), n, auto_reset=ar)
                            for code in (1, 6, 7, 11, 15):
                                got = abi.describe_foveal_step(M.params(abi, variant, G, L, rest | code << 4), n, auto_reset=ar)
                                assert got == want, (variant, G, L, n, hex(rest), code, ar)
                                checked += 1
                        for ar, k in ((True, None), (False, None), (True, 3)):
                            if (two and (not ar or (k and G != 18))) or (variant == "v1" and k and G != 14):
                                continue
                            want = abi.describe_foveal_rollout(M.params(abi, variant, G, L, rest), n, 16, ar, two, k)
                            for code in (1, 5, 6, 9, 15):
                                got = abi.describe_foveal_rollout(M.params(abi, variant, G, L, rest | code << 4), n, 16, ar, two, k)
                                assert got == want, (variant, G, L, n, hex(rest), code, ar, k)
                                checked += 1
    assert checked > 10000


def test_the_recording_description_answers_the_entry_points_refusals(abi):
    """lmaze_describe_foveal_rollout_obs: LMAZE_E_GRID for v1 off G = 14 and v5 / v6 off G = 18, LMAZE_E_COUNT for
    obs_every < 1 (before anything else), and the recording form of the kernel where lmaze_foveal_rollout_obs runs"""
    for variant in M.VARIANTS:
        two = variant in M.TWO_LEVEL
        for G in M.SWEEP_GRIDS:
            p = M.params(abi, variant, G, M.default_layouts(variant), 0)
            refused = (variant == "v1" and G != 14) or (two and G != 18)
            for ar in ((True,) if two else (False, True)):
                if refused:
                    with pytest.raises(abi.LmazeError) as e:
                        abi.describe_foveal_rollout(p, 1000, 16, ar, two, obs_every=3)
                    assert e.value.code == M.E_GRID, (variant, G)
                else:
                    text = abi.describe_foveal_rollout(p, 1000, 16, ar, two, obs_every=3)
                    plain = abi.describe_foveal_rollout(p, 1000, 16, ar, two)
                    assert ", obs_t>" in text and text.replace(", obs_t>", ">") == plain, (text, plain)
                for k in (0, -1):
                    with pytest.raises(abi.LmazeError) as e:
                        abi.describe_foveal_rollout(p, 1000, 16, ar, two, obs_every=k)
                    assert e.value.code == M.E_COUNT, (variant, G, k)
                assert abi.describe_foveal_rollout(p, 0, 16, ar, two, obs_every=3) == ""     # nothing to do: no launch
    assert "lmaze_describe_foveal_rollout_obs" in abi.SYMBOLS


def test_the_table_is_cheap_and_ragged(abi):
    """every row: a small T and an observation within 512 MiB; N ragged against the envs per workgroup the row gets; every
    kernel family has a row below one chunk and a row whose last workgroup takes fewer chunks than the first; the
    recordings leave trailing steps; the streaming sizes sit right past their thresholds"""
    below, short_last = set(), set()
    for r in M.ROWS:
        assert r.entry in M.ENTRIES and r.variant in M.VARIANTS and 1 <= r.T <= 9, r
        assert r.N * M.CHANNELS[r.variant] * 100 <= 512 << 20 and 5 <= r.G <= 64 and 1 <= r.n_layouts <= M.MAX_LAYOUTS, r
        assert (r.obs_every is not None) == (r.entry in M.RECORDING) and 0 <= r.hint < 0x400, r
        text = M.describe(abi, *r)
        epb, grid, chunks = (M.field(text, f) for f in ("envs_per_workgroup", "grid", "chunks"))
        assert r.N % epb, (r, text)
        family = text.split("<")[0]
        if r.N < epb:
            below.add(family)
        nchunks = -(-r.N // epb)
        if chunks > 1 and grid > 1 and nchunks % grid:
            short_last.add(family)
    assert below == short_last == {"foveal_kernel", "foveal_rollout_kernel"}
    rec = [r for r in M.ROWS if r.obs_every]
    assert any(r.T % r.obs_every for r in rec) and any(r.obs_every == 1 for r in rec)
    for v in M.VARIANTS:
        n = M.n_past_plain(v)
        assert n % 2 and M.nt_set(v, n) and not M.nt_set(v, n - 2), v
        assert any(r.variant == v and r.N == n and r.hint == 0 for r in M.ROWS), v
    assert M.N_PAST_FUSED * 400 > M.STREAM_BYTES >= (M.N_PAST_FUSED - 2) * 400
    # the ragged size at 256 envs x 4 chunks, as the launcher plans it.  Chunks are taken grid-stride (workgroup b takes
    # chunks b, b + grid, ...): one workgroup takes fewer chunks than the first, and the partial last chunk belongs to
    # another workgroup, not to the short one
    r = M.Row(M.STEP, "v1", 18, 1, M.N_RAGGED, 4, None, M.hint(0, 5, 4))
    assert r in M.ROWS
    text = M.describe(abi, *r)
    epb, grid, chunks = (M.field(text, f) for f in ("envs_per_workgroup", "grid", "chunks"))
    assert (epb, chunks) == (256, 4), text
    nchunks = -(-r.N // epb)
    taken = [len(range(b, nchunks, grid)) for b in range(grid)]
    assert sum(taken) == nchunks and max(taken) == chunks == taken[0] and min(taken) == chunks - 1, (text, taken)
    assert 0 < r.N % epb < 32 and taken[(nchunks - 1) % grid] == chunks, (text, taken)
    assert len(M.groups()) < 300


def test_the_table_holds_every_axis_value_the_launcher_branches_on():
    """the kernel_key coverage does not see these: they pick no other kernel, but the halving fallback, the cap's pad at
    large layout tables, the sizes below one chunk and the rollouts' default size switch are what they exercise.  A
    later trim of the table must keep a row for each."""
    steps, rolls = (M.STEP, M.STEP_RESET), (M.ROLLOUT, M.ROLLOUT_OBS)

    def have(**want):
        return any(all(getattr(r, f) in (v if isinstance(v, tuple) else (v,)) for f, v in want.items()) for r in M.ROWS)

    for v in ("v1", "v2", "v4", "v5"):
        for entry in steps:
            for G in M.STEP_GRIDS:
                assert have(entry=entry, variant=v, G=G, N=M.N_RAGGED), (entry, v, G)
            for N in (M.N_SMALL, M.N_ONE):
                assert have(entry=entry, variant=v, N=N), (entry, v, N)
            assert have(entry=entry, variant=v, N=M.n_past_plain(v), hint=0), (entry, v)
        for G in (M.ROLL_GT[v], 13, 33, 64):
            assert have(entry=M.ROLLOUT, variant=v, G=G, N=M.N_RAGGED), (v, G)
        for N in (M.N_SMALL, M.N_ONE, M.N_ROLL64, M.n_past_plain(v)):
            assert have(entry=M.ROLLOUT, variant=v, N=N, hint=0), (v, N)
        assert have(entry=M.ROLLOUT_OBS, variant=v, N=M.N_ROLL64) and have(entry=M.ROLLOUT_OBS, variant=v, G=13), v
        for k in (1, 3):
            assert have(entry=M.ROLLOUT_OBS, variant=v, G=M.ROLL_GT[v], obs_every=k), (v, k)
        if v != "v1":                                   # v1 has one layout
            for entry in steps + (M.ROLLOUT,):
                for G, L in ((18, 1), (18, M.MAX_LAYOUTS), (64, 1), (64, M.MAX_LAYOUTS)):
                    caps = {r.hint & 15 for r in M.ROWS if (r.entry, r.variant, r.G, r.n_layouts) == (entry, v, G, L)}
                    assert caps >= {0, 2, 5, 8, 12}, (entry, v, G, L, caps)
        if v in ("v2", "v4"):
            assert have(entry=M.STEP_RESET, variant=v, N=M.N_PAST_FUSED, hint=0), v
            assert have(entry=M.ROLLOUT_OBS, variant=v, G=64, n_layouts=M.MAX_LAYOUTS), v
    for entry in steps + rolls:
        assert have(entry=entry, variant="v6"), entry
        assert have(entry=entry, variant="v6", N=M.N_ROLL64 if entry in rolls else M.n_past_plain("v6")), entry
    for entries, codes, bad in ((steps, (2, 3, 4, 5), (1, 6)), (rolls, (2, 3, 4), (1, 5))):
        for entry in entries:
            for v in M.VARIANTS:
                rows = [r for r in M.ROWS if r.entry == entry and r.variant == v]
                assert {r.hint >> 4 & 15 for r in rows} >= set(codes) and {r.hint >> 4 & 15 for r in rows} & set(bad), (entry, v)
                assert {r.hint >> 8 for r in rows} == {0, 1, 2, 3}, (entry, v)
                assert {r.hint & 15 for r in rows} >= {0, 2, 5} and any(r.hint & 15 > 8 for r in rows), (entry, v)
            assert any(r.hint & 15 == 8 for r in M.ROWS if r.entry == entry), entry


@pytest.mark.parametrize("variant", ["v2", "v4"])
def test_the_three_rollout_families_describe_one_launch_where_no_table_is_staged(abi, variant):
    """The open loop, the epsilon-greedy and the sampling closed loop share one launcher (lmaze_foveal_launch.h): where the
    closed loops stage no table they plan the open loop's launch, and their lines differ from its line in the kernel's name
    and the " table=global" suffix alone.  G = 24 with 16 layouts: 9 216 B of greedy actions (rule: 8 192) and 884 736 B of
    thresholds (rule: 16 384), and v4's 18 816 + 272 envs = 53 632 B at 128 envs per workgroup is within the 64 KiB the
    launcher assumes without a device, so no size is halved."""
    G, L, T = 24, 16, 24
    assert L * G * G == 9216 > 8192 and L * G * G * 96 == 884736 > 16384
    fields = ("envs_per_workgroup", "chunks", "grid", "block", "lds", "workgroups_per_cu")
    sizes = set()
    for n in (333, 40000, 1 << 20):
        for h in (0, 0x20, 0x30, 0x40, 0x120, 0x25):
            for ar in (False, True):
                for every in (0, 3):
                    p = M.params(abi, variant, G, L, h)
                    o = abi.describe_foveal_rollout(p, n, T, ar, False, every or None)
                    assert o.startswith("foveal_rollout_kernel<"), o
                    lines = {"policy": abi.describe_foveal_rollout_policy(p, n, T, ar, every),
                             "sample": abi.describe_foveal_rollout_sample(p, n, T, ar, every)}
                    for family, c in lines.items():
                        assert [M.field(c, f) for f in fields] == [M.field(o, f) for f in fields], (o, c)
                        assert c.replace("foveal_rollout_%s_kernel<" % family, "foveal_rollout_kernel<").replace("> table=global ", "> ") == o, (o, c)
                    sizes.add(M.field(o, "envs_per_workgroup"))
    assert sizes == {32, 64, 128}
