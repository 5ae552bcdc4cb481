"""CPU: Q-learning inside the one-launch rollout (include/lmaze.h lmaze_env_rollout_qlearn / lmaze_describe_env_rollout_qlearn)
without a GPU -- the arithmetic of csrc/lmaze_learn.h run as a host program under the sanitizers against the numpy
restatement of tests/qlearn_ref.py, the symbols, every documented refusal in its order of precedence (answered before any
device call), the launch the describe call names, what the four new kernel forms need per wave, and the learning case of
tests/test_gpu_qlearn.py on the restatement alone."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import qlearn_ref as R
from closed_loop_ref import fields as _fields, grid_params as _params, perenv_lds as _perenv_lds, shared_lds as _shared_lds
from helpers import HIPCC, f32_bits, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_GRID, E_VARIANT, E_LAYOUT, E_COUNT, E_ALIGN = -1, -2, -3, -4, -5, -6
NAMES = ("lmaze_env_rollout_qlearn", "lmaze_describe_env_rollout_qlearn")


def _up16(x):
    return (x + 15) & ~15


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


# ------------------------------------------------------------- the arithmetic, as a host program under the sanitizers
@pytest.fixture(scope="module")
def qlearn_host(tmp_path_factory):
    """tests/csrc/qlearn_host.cpp: a stand-alone program around lmaze_learn.h, built with the address and undefined-behaviour
    sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("qlearn_host")
    exe = str(tmp / "qlearn_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "qlearn_host.cpp")])

    def run(mode, *arrays):
        src, dst = str(tmp / (mode + ".in")), str(tmp / (mode + ".out"))
        with open(src, "wb") as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        return open(dst, "rb").read()
    return run


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 100.0, -0.01, 1e-45, 3.4e38], np.float32)


def _rows():
    """Random rows, rows of a few values (ties everywhere), +-0.0 / +-inf / NaN in each position, and all-equal rows"""
    rs = np.random.RandomState(21)
    rows = [rs.randn(4000, 4).astype(np.float32), rs.choice(np.array([-1.0, 0.0, -0.0, 0.5, 0.5, 2.0], np.float32), (4000, 4)),
            rs.choice(SPECIAL, (4000, 4))]
    for pos in range(4):
        for v in SPECIAL:
            r = rs.randn(8, 4).astype(np.float32)
            r[:, pos] = v
            rows.append(r)
    rows.append(np.repeat(SPECIAL[:, None], 4, axis=1))
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)


def _first_max(qlearn_host, rows):
    raw = qlearn_host("max", np.array([len(rows)], np.int64), rows)
    return np.frombuffer(raw[:4 * len(rows)], np.float32), np.frombuffer(raw[4 * len(rows):], np.int32)


def test_host_first_max_is_the_strict_greater_chain(qlearn_host):
    rows = _rows()
    best, act = _first_max(qlearn_host, rows)
    want_best, want_act = R.first_max(rows)
    assert (act == want_act).all() and (f32_bits(best) == f32_bits(want_best)).all()
    # by hand: ties keep the first, -0.0 does not beat +0.0 nor the other way round, a NaN never wins, a NaN in q[0] stays
    nan = np.nan
    hand = np.array([[1, 1, 1, 1], [0, 1, 1, 0], [-0.0, 0.0, 0.0, -0.0], [0.0, -0.0, 1.0, 1.0], [nan, 5, 6, 7], [1, nan, 2, nan],
                     [-np.inf, nan, -np.inf, -np.inf], [3, 2, np.inf, np.inf], [nan, nan, nan, nan]], np.float32)
    best, act = _first_max(qlearn_host, hand)
    assert act.tolist() == [0, 1, 0, 2, 0, 2, 0, 2, 0]
    assert f32_bits(best)[2] == 0x80000000 and np.isnan(best[4]) and np.isnan(best[8]) and best[5] == 2.0 and best[6] == -np.inf


def _update(qlearn_host, alpha, gamma, q_sa, r, done, v_next):
    m = len(q_sa)
    raw = qlearn_host("update", np.array([m], np.int64), np.array([alpha, gamma], np.float32), q_sa.astype(np.float32),
                      r.astype(np.float32), done.astype(np.uint8), v_next.astype(np.float32))
    return np.frombuffer(raw, np.float32).reshape(3, m)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0, 0.1])
@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.0])
def test_host_target_and_update_are_the_numpy_roundings(qlearn_host, alpha, gamma):
    """10^5 random samples and the special values: rewards from the reference's literals and random ones, done 0 / 1"""
    rs = np.random.RandomState(22)
    m = 100000
    q_sa = (rs.randn(m) * np.exp2(rs.randint(-8, 8, m))).astype(np.float32)
    v_next = (rs.randn(m) * np.exp2(rs.randint(-8, 8, m))).astype(np.float32)
    r = np.where(rs.rand(m) < 0.5, rs.choice(np.array([-0.0, -0.01, -1.0, 100.0], np.float32), m), rs.randn(m)).astype(np.float32)
    done = (rs.rand(m) < 0.3).astype(np.uint8)
    k = 2000
    q_sa[:k], v_next[:k], r[:k] = rs.choice(SPECIAL, k), rs.choice(SPECIAL, k), rs.choice(SPECIAL, k)
    target, delta, q_new = _update(qlearn_host, alpha, gamma, q_sa, r, done, v_next)
    want_t = R.q_target(r, done, gamma, v_next)
    want_q, want_d = R.q_update(q_sa, alpha, want_t)

    def same(a, b):                                       # bit for bit; a NaN for a NaN (its payload is the platform's)
        return ((f32_bits(a) == f32_bits(b)) | (np.isnan(a) & np.isnan(b))).all()
    assert same(target, want_t) and same(delta, want_d) and same(q_new, want_q)
    fin = np.isfinite(q_sa) & np.isfinite(want_t)
    if alpha == 0.0:
        assert (f32_bits(q_new[fin] + np.float32(0.0)) == f32_bits(q_sa[fin] + np.float32(0.0))).all()   # q + 0 * delta
    # a done row is the reward itself: its bits, the sign of zero kept, no NaN from an infinite v_next
    assert (f32_bits(target[done != 0]) == f32_bits(r[done != 0])).all()


def test_host_target_is_never_fused(qlearn_host):
    """A case where fma(gamma, v, r) and the product rounded before the sum differ in the last bit, found by search: the
    host program and the restatement both give the unfused one."""
    rs = np.random.RandomState(23)
    g = np.float32(0.99)
    v = (rs.rand(200000).astype(np.float32) * np.float32(100.0)).astype(np.float32)
    r = np.full(len(v), -0.01, np.float32)
    unfused = ((g * v).astype(np.float32) + r).astype(np.float32)
    fused = (g.astype(np.float64) * v.astype(np.float64) + r.astype(np.float64)).astype(np.float32)   # the product is exact in double
    differ = np.flatnonzero(f32_bits(unfused) != f32_bits(fused))
    assert len(differ) > 100
    sel = differ[:1000]
    assert (np.abs(f32_bits(unfused[sel]).astype(np.int64) - f32_bits(fused[sel]).astype(np.int64)) == 1).all()
    target, _, _ = _update(qlearn_host, 0.5, 0.99, np.zeros(len(sel), np.float32), r[sel], np.zeros(len(sel), np.uint8), v[sel])
    assert (f32_bits(target) == f32_bits(unfused[sel])).all()
    assert (f32_bits(R.q_target(r[sel], np.zeros(len(sel)), 0.99, v[sel])) == f32_bits(unfused[sel])).all()
    # the same for alpha * delta + q
    a = np.float32(0.1)
    d = v[:200000]
    q0 = np.full(len(d), 1.0, np.float32)
    unf = ((a * d).astype(np.float32) + q0).astype(np.float32)
    fus = (a.astype(np.float64) * d.astype(np.float64) + q0.astype(np.float64)).astype(np.float32)
    sel = np.flatnonzero(f32_bits(unf) != f32_bits(fus))[:1000]
    assert len(sel) > 100
    # target = q + d exactly representable?  not in general: feed the delta through done rows, r = q + d rounded, and keep
    # the samples whose delta comes back as d
    tgt = (q0[sel] + d[sel]).astype(np.float32)
    back = (tgt - q0[sel]).astype(np.float32)
    keep = f32_bits(back) == f32_bits(d[sel])
    assert keep.sum() > 10
    sel = sel[keep]
    _, delta, q_new = _update(qlearn_host, 0.1, 0.99, q0[sel], tgt[keep], np.ones(len(sel), np.uint8), np.zeros(len(sel), np.float32))
    assert (f32_bits(delta) == f32_bits(d[sel])).all() and (f32_bits(q_new) == f32_bits(unf[sel])).all()


# ------------------------------------------------------------- symbols and refusals
def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in NAMES:
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
        assert not name.startswith(("lmaze_rollout", "lmaze_describe_rollout"))
    assert abi.lib.lmaze_abi_version() == 4
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("UPDATED IN PLACE", "FIRST maximum", "BEFORE this step's write", "never a fused multiply-add", "goal-free",
                   "qlearn=env, table=global", "v0:146-237", "v3:220-402", "v0:64-110", "n G^2 > INT32_MAX"):
        assert phrase in flat, phrase
    pkg = importlib.import_module("gym-lmaze_amd")
    doc = pkg.LmazeVecEnv.rollout_qlearn.__doc__
    for phrase in ("solve()", "rollout_policy(q=q, key=\"env\")", "state_keys(\"env\")", "table_stats", "UPDATED IN PLACE"):
        assert phrase in " ".join(doc.split()), phrase


def _call(abi, variant="v0", G=11, mode=None, T=6, n=100, q=64, obs_t=None, every=0, params=True, layout=64, ball=64, goal=None,
          obs=None, key_t=None, td_t=None):
    """Fabricated device addresses: every refusal is returned before anything is dereferenced or queued."""
    p = abi.make_params(abi.VARIANT_V3 if variant == "v3" else (abi.VARIANT_V0 if variant == "v0" else variant), G,
                        abi.LAYOUT_PER_ENV if mode is None else mode, 100, -1.0, -0.01, 100.0)
    return abi.lib.lmaze_env_rollout_qlearn(C.byref(p) if params else None, layout, q, 0.5, 0.99, 0, T, ball, goal, 64, 64, 64, None,
                                            obs, None, None, None, key_t, td_t, n, 1, 1, 0, 0, obs_t, every, None)


def test_refusals_in_order_of_precedence(abi):
    """lmaze_env_rollout_policy's refusals in its order, q in the place of policy: 16 bytes for q, 4 for td_t"""
    G64_OVER, G64_FITS = 1 << 19, (1 << 19) - 1          # n * 64 * 64 = 2^31, and the largest n below it
    # 1. the recording request, before anything else -- even NULL params or a bad count
    assert _call(abi, every=-1) == E_COUNT
    assert _call(abi, obs_t=4096, every=0) == E_COUNT
    assert _call(abi, obs_t=None, every=3) == E_NULL
    assert _call(abi, obs_t=4096 + 4, every=3) == E_ALIGN
    assert _call(abi, obs_t=None, every=3, n=-1, params=False) == E_NULL
    assert _call(abi, every=-1, q=None, G=64, n=G64_OVER) == E_COUNT
    # 2. params, variant, T -- before the row count
    assert _call(abi, params=False) == E_NULL
    assert _call(abi, G=2, n=1 << 30) == E_GRID
    assert _call(abi, G=65, n=1 << 30) == E_GRID
    assert _call(abi, mode=5, G=64, n=G64_OVER) == E_LAYOUT
    assert _call(abi, n=-1) == E_COUNT
    assert _call(abi, variant=2, G=64, n=G64_OVER) == E_VARIANT
    assert _call(abi, T=-1) == E_COUNT
    # 3. n * G^2 > INT32_MAX: before "nothing to do" and before the pointers, both layout modes
    for mode in (abi.LAYOUT_PER_ENV, abi.LAYOUT_SHARED):
        for variant, goal in (("v0", None), ("v3", 64)):
            m = dict(mode=mode, variant=variant, goal=goal)
            assert _call(abi, G=64, n=G64_OVER, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, T=0, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, q=None, layout=None, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_OVER, q=64 + 4, td_t=4097, **m) == E_COUNT
            assert _call(abi, G=64, n=G64_FITS, q=None, **m) == E_NULL
            assert _call(abi, G=64, n=G64_FITS, T=0, q=None, **m) == 0
    assert _call(abi, G=11, n=17747799) == E_COUNT
    assert _call(abi, G=11, n=17747798, q=None) == E_NULL
    # 4. pointers: q among them; then alignment, q's and td_t's among them
    assert _call(abi, q=None) == E_NULL
    assert _call(abi, variant="v3", goal=None) == E_NULL
    assert _call(abi, layout=None) == E_NULL
    assert _call(abi, q=None, ball=68) == E_NULL                    # NULL before alignment
    assert _call(abi, q=None, td_t=4097) == E_NULL
    assert _call(abi, layout=None, q=64 + 4) == E_NULL
    assert _call(abi, ball=68) == E_ALIGN
    assert _call(abi, obs=4096 + 8) == E_ALIGN
    assert _call(abi, layout=72) == E_ALIGN
    for mode in (abi.LAYOUT_PER_ENV, abi.LAYOUT_SHARED):
        for variant, goal in (("v0", None), ("v3", 64)):
            for off in (1, 4, 8, 12):
                assert _call(abi, q=4096 + off, mode=mode, variant=variant, goal=goal) == E_ALIGN
            for off in (1, 2, 3):
                assert _call(abi, td_t=4096 + off, mode=mode, variant=variant, goal=goal) == E_ALIGN


@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("T,n", [(0, 100), (6, 0), (0, 0)])
def test_nothing_to_do_reads_no_pointer_and_no_alignment(abi, variant, T, n):
    assert _call(abi, variant=variant, T=T, n=n, q=None, layout=None, ball=None) == 0
    assert _call(abi, variant=variant, T=T, n=n, q=4096 + 1, td_t=4097, layout=72, ball=68, obs=4096 + 8) == 0
    assert _call(abi, variant=variant, T=T, n=n, q=None, every=3 if T < 3 else 7) == 0
    assert _call(abi, variant=variant, T=-1, n=n, q=None) == E_COUNT


# ------------------------------------------------------------- describe lines
@pytest.mark.parametrize("variant", ["v0", "v3"])
@pytest.mark.parametrize("per_env", [True, False])
def test_describe_lines(abi, variant, per_env):
    """The name says the kernel, the form and that the table is in global memory; lds is the body's own arrays rounded up to
    16 -- the total of csrc/lmaze_rollout_lds.h under LMAZE_TAB_GLOBAL, nothing reserved for the table -- and the launch is
    that of the sampling form with a table per env, whatever launch_hint bits 12-14 select; bit 8 is not read."""
    mode = abi.LAYOUT_PER_ENV if per_env else abi.LAYOUT_SHARED
    kernel = "rollout_perenv_kernel" if per_env else "rollout_shared_kernel"
    own = _perenv_lds if per_env else _shared_lds
    for G in (8, 11, 18, 32, 64):
        for n in (777, 16384, 65536):
            for k in range(8):
                for T, every in ((16, 3), (16, 0), (1, 0)):
                    p = _params(abi, variant, G, mode, k << 12)
                    line = abi.describe_env_rollout_qlearn(p, n, T, obs_every=every)
                    head = "%s<v%s, qlearn=env, table=global%s> T=%d every=%d " % (kernel, variant[1], ", obs_t" if every else "", T, every)
                    assert line.startswith(head), line
                    f = _fields(line)
                    epb = f["envs_per_workgroup"]
                    assert epb % 4 == 0 and epb >= 4 and f["grid"] == -(-n // epb) and f["block"] == 256, line
                    assert f["lds"] == _up16(own(G, epb)) <= 160 << 10, line
                    twin = abi.describe_env_rollout(p, n, T, obs_every=every, form="sample")
                    assert line == twin.replace("sample=env", "qlearn=env"), (line, twin)
                    assert abi.describe_env_rollout_qlearn(_params(abi, variant, G, mode, (k << 12) | 0x100), n, T,
                                                           obs_every=every) == line
    p = _params(abi, variant, 11, mode, 1 << 15)
    assert ", obs_t, nt> " in abi.describe_env_rollout_qlearn(p, 4099, 8, obs_every=2)
    assert ", nt" not in abi.describe_env_rollout_qlearn(p, 4099, 8, obs_every=0)
    assert "obs_t" not in abi.describe_env_rollout_qlearn(p, 4099, 8, with_obs=False)


def test_describe_refusals_and_empty_lines(abi):
    p = _params(abi, "v0", 11, abi.LAYOUT_PER_ENV)
    buf = C.create_string_buffer(256)
    d = abi.lib.lmaze_describe_env_rollout_qlearn
    assert d(C.byref(p), 100, 6, 1, 1, -1, buf, 256) == E_COUNT
    assert d(C.byref(p), 100, 6, 1, 2, 0, buf, 256) == E_COUNT        # no narrow planes
    assert d(C.byref(p), 100, 6, 1, 1, 0, None, 256) == E_NULL
    assert d(None, 100, 6, 1, 1, 0, buf, 256) == E_NULL
    assert d(C.byref(p), 100, -1, 1, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(_params(abi, "v0", 64, abi.LAYOUT_PER_ENV)), 1 << 19, 6, 1, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(_params(abi, "v0", 64, abi.LAYOUT_PER_ENV)), 1 << 19, 0, 1, 1, 0, buf, 256) == E_COUNT
    assert d(C.byref(_params(abi, "v0", 2, abi.LAYOUT_PER_ENV)), 100, 6, 1, 1, 0, buf, 256) == E_GRID
    assert abi.describe_env_rollout_qlearn(p, 0, 6) == "" and abi.describe_env_rollout_qlearn(p, 100, 0) == ""
    # the describe entry of the other per-env forms keeps its two forms
    assert abi.lib.lmaze_describe_env_rollout(C.byref(p), 100, 6, 1, 1, 0, 2, buf, 256) == E_COUNT
    assert abi.ENV_ROLLOUT_FORMS == {"policy": 0, "sample": 1}
    lds_h = open(os.path.join(CSRC, "lmaze_rollout_lds.h")).read()
    assert "LMAZE_TAB_GLOBAL = 3, LMAZE_TAB_ENV_BYTES = 4 }" in lds_h          # no new table kind


# ------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_qlearn_kernels_no_scratch():
    """Exactly four new instantiations (two kernels x v0 / v3), none with scratch -- the condition.  Their registers and waves
    per SIMD beside the sampling sibling's with a table per env are printed."""
    kernels = kernel_usage("lmaze_step.hip")
    new = {k: v for k, v in kernels.items() if "RolloutEnvQArgs" in k}
    assert len(new) == 4, sorted(new)
    for frag in ("21rollout_shared_kernelILi0E", "21rollout_shared_kernelILi3E", "21rollout_perenv_kernelILi0E",
                 "21rollout_perenv_kernelILi3E"):
        assert sum(frag in k and "15RolloutEnvQArgs" in k for k in new) == 1, frag
    for name, v in sorted(new.items()):
        twin = name.replace("15RolloutEnvQArgs", "18RolloutEnvRowsArgs")
        assert twin in kernels and twin != name, name
        print("%s: VGPRs %d, waves per SIMD %d (sibling: %d, %d)" % (name, v["VGPRs"], v["Occupancy"], kernels[twin]["VGPRs"],
                                                                   kernels[twin]["Occupancy"]))
        assert v.get("ScratchSize", 0) == 0, (name, v)
    for old in ("11RolloutArgs", "14RolloutObsArgs", "RolloutPolicyArgs", "RolloutSampleArgs", "RolloutEnvBytesArgs", "RolloutEnvRowsArgs"):
        assert not any(old in k for k in new), old


# ------------------------------------------------------------- the restatement: pocket recurrence, and it learns
def test_restatement_in_a_pocket_is_the_scalar_recurrence():
    """A ball walled in on all four sides, epsilon = 0: every step bumps, c' == c, and q[c, a] follows one scalar
    recurrence -- q <- q + alpha * ((r_wall + gamma * max q[c]) - q), the maximum taken before the write."""
    N, G, T = 9, 8, 40
    lay, cell = R.pocket_layouts(N, G)
    st = R.learn_start(N)
    st["ball_xy"][:], st["done"][:] = cell, 0
    q = R.random_table(N, G, 3)
    q0 = q.copy()
    out = R.learn("v0", G, "per_env", lay, st, q, T, 0.5, 0.99, 0, False, 5, 9, 0, step_limit=1000)
    assert (st["ball_xy"] == cell).all() and not out["rows"]["done"].any()
    c = cell[:, 0] * G + cell[:, 1]
    assert (out["rows"]["key"] == np.arange(N) * G * G + c).all()
    for i in range(N):
        row = q0[i, c[i]].copy()
        for t in range(T):
            a = 0
            for j in (1, 2, 3):
                if row[j] > row[a]:
                    a = j
            target = np.float32(np.float32(-1.0) + np.float32(np.float32(0.99) * row[a]))
            delta = np.float32(target - row[a])
            assert out["rows"]["act"][t, i] == a and f32_bits(out["rows"]["td"][t, i]) == f32_bits(delta)
            row[a] = np.float32(row[a] + np.float32(np.float32(0.5) * delta))
        assert (f32_bits(q[i, c[i]]) == f32_bits(row)).all()
        other = np.arange(G * G) != c[i]
        assert (f32_bits(q[i, other]) == f32_bits(q0[i, other])).all()
    assert len(set(map(tuple, out["rows"]["act"].T.tolist()))) > 1 and (out["rows"]["act"].max(0) > out["rows"]["act"].min(0)).any()


def test_the_learning_case_meets_its_condition_on_the_restatement():
    """The condition tests/test_gpu_qlearn.py sets on its inputs, checked before any GPU run: after 64 x 64 steps from a zero
    table the greedy walk of the restatement's own table arrives in the fewest steps from at least 0.90 of the cells that
    can reach 'X' (measured when the seed was chosen: 532 of 559, 0.952)."""
    case = R.learn_case()
    print("greedy walks at the fewest steps: %d of %d" % (case["good"], case["total"]))
    assert case["total"] == 559 and case["good"] / case["total"] >= 0.90
