"""CPU: the learner-side entry points (lmaze_advantages, lmaze_advantages_table, lmaze_table_stats,
lmaze_describe_table_stats) without a GPU -- the symbols and the header's statement of the rules, every documented refusal
in its order of precedence (answered before any device call), the launch the describe call names, the per-element
arithmetic of lmaze_learn.h compiled for the host under the address and undefined-behaviour sanitizers and compared bit for
bit with its numpy restatement (tabular_ref.py), and what the new kernels need per wave."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tabular_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_NULL, E_COUNT, E_ALIGN = -1, -5, -6
NAMES = ("lmaze_advantages", "lmaze_advantages_table", "lmaze_table_stats", "lmaze_describe_table_stats")
MAX_ENVS = 1 << 30


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def test_symbols_exported_and_declared(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in NAMES:
        assert name in abi.SYMBOLS and hasattr(abi.lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    pkg = importlib.import_module("gym-lmaze_amd")
    for name in ("gae", "table_stats", "table_means"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.LmazeVecEnv.state_keys)
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("never a fused multiply-add", "ties to even", "skipped entirely", "adds onto", "4096 bins",
                   "adv_t may be reward_t", "target_t may be value_t", "step limit is treated as terminal",
                   "one unsigned compare", "below 2^39", "it never faults", "keys actions > 2^28"):
        assert phrase in flat, phrase


# ------------------------------------------------------------- refusals
def test_advantages_refusals_and_nothing_to_do(abi):
    """NULL for a required pointer, then the counts; T == 0 or n == 0 returns 0 on fabricated, misaligned pointers: nothing is
    read or queued.  tail and target_t are optional."""
    f = abi.lib.lmaze_advantages
    ok = dict(reward=64, done=64, value=64, tail=None, adv=64, target=None)

    def call(T=5, n=10, **kw):
        a = dict(ok, **kw)
        return f(a["reward"], a["done"], a["value"], a["tail"], 0.99, 0.95, a["adv"], a["target"], T, n, None)
    for name in ("reward", "done", "value", "adv"):
        assert call(**{name: None}) == E_NULL, name
        assert call(T=-1, n=-1, **{name: None}) == E_NULL, name        # NULL before the counts
        assert call(T=0, **{name: None}) == E_NULL, name               # ... and before "nothing to do"
    assert call(T=-1) == E_COUNT
    assert call(n=-1) == E_COUNT
    assert call(n=MAX_ENVS + 1, tail=64, target=64) == E_COUNT
    assert call(T=-1, n=0) == E_COUNT                                  # a bad count is refused with nothing to do, too
    assert call(T=0, n=-1) == E_COUNT
    for T, n in ((0, 10), (5, 0), (0, 0), (0, MAX_ENVS)):
        assert call(T=T, n=n) == 0
        assert call(T=T, n=n, reward=65, done=67, value=66, tail=70, adv=73, target=74) == 0


def test_advantages_table_refusals_and_nothing_to_do(abi):
    """The table form: key_t and values are required, key_tail and target_t are not; keys < 1 joins the counts."""
    f = abi.lib.lmaze_advantages_table
    ok = dict(reward=64, done=64, key=64, key_tail=None, values=64, adv=64, target=None)

    def call(T=5, n=10, keys=121, **kw):
        a = dict(ok, **kw)
        return f(a["reward"], a["done"], a["key"], a["key_tail"], a["values"], keys, 0.99, 0.95, a["adv"], a["target"], T, n, None)
    for name in ("reward", "done", "key", "values", "adv"):
        assert call(**{name: None}) == E_NULL, name
        assert call(T=-1, keys=0, **{name: None}) == E_NULL, name
        assert call(n=0, **{name: None}) == E_NULL, name
    assert call(T=-1) == E_COUNT
    assert call(n=-1) == E_COUNT
    assert call(n=MAX_ENVS + 1) == E_COUNT
    for keys in (0, -1, -(1 << 40)):
        assert call(keys=keys) == E_COUNT
        assert call(keys=keys, T=0) == E_COUNT                         # before "nothing to do"
        assert call(keys=keys, n=0) == E_COUNT
    for T, n in ((0, 10), (5, 0), (0, 0), (0, MAX_ENVS)):
        for keys in (1, 121, 1 << 40):
            assert call(T=T, n=n, keys=keys) == 0
            assert call(T=T, n=n, keys=keys, reward=65, done=67, key=66, key_tail=70, values=69, adv=73, target=74) == 0


def test_table_stats_refusals_and_nothing_to_do(abi):
    f = abi.lib.lmaze_table_stats

    def call(key=64, act=64, w=64, m=100, keys=121, actions=4, count=64, total=64):
        return f(key, act, w, m, keys, actions, count, total, None)
    # 1. key_t or count missing
    assert call(key=None) == E_NULL
    assert call(count=None) == E_NULL
    assert call(key=None, w=None, m=-1, keys=0) == E_NULL              # before the pair and before the counts
    assert call(count=None, total=None, actions=0) == E_NULL
    # 2. exactly one of weight_t / total_q24
    assert call(w=None) == E_NULL
    assert call(total=None) == E_NULL
    assert call(w=None, m=-1) == E_NULL                                # before the counts
    assert call(total=None, m=0) == E_NULL                             # ... and before "nothing to do"
    # 3. the counts
    assert call(m=-1) == E_COUNT
    assert call(keys=0) == E_COUNT
    assert call(keys=-5) == E_COUNT
    for actions in (0, -1, 256, 1 << 20):
        assert call(actions=actions) == E_COUNT
    assert call(keys=(1 << 28) // 4 + 1, actions=4) == E_COUNT
    assert call(keys=(1 << 28) + 1, actions=1, act=None) == E_COUNT
    assert call(keys=1 << 62, actions=255) == E_COUNT                  # the product does not wrap into range
    assert call(act=None, actions=4) == E_COUNT
    assert call(act=None, actions=2, m=0) == E_COUNT                   # before "nothing to do"
    assert call(m=0, keys=0) == E_COUNT
    # m == 0: nothing read, whatever the addresses; the largest tables are accepted
    for kw in (dict(), dict(w=None, total=None), dict(act=None, actions=1), dict(keys=(1 << 28) // 4), dict(keys=1 << 28, actions=1),
               dict(keys=1, actions=255)):
        assert call(m=0, **kw) == 0, kw
        assert call(m=0, **dict(dict(key=65, count=67), **kw)) == 0, kw
    assert call(m=0, key=65, act=66, w=67, count=69, total=70) == 0
    # rows off a 4-byte and tables off an 8-byte boundary, once there is something to do
    assert call(key=66) == E_ALIGN and call(act=65) == E_ALIGN and call(w=67) == E_ALIGN
    assert call(count=68) == E_ALIGN and call(total=68) == E_ALIGN


# ------------------------------------------------------------- describe
def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


def test_describe_table_stats(abi):
    """Where the table lives is a rule: up to 4096 bins in LDS, 16 bytes per bin and sized to the table; above that, global
    atomics and no LDS.  One launch for any m: the grid is capped."""
    for keys, actions in ((121, 4), (1024, 4), (4096, 1), (1024, 1), (1, 1), (17, 255 // 17)):
        bins = keys * actions
        for m in (1, 13 * 777, 64 * 4099, 16 << 20, 1 << 34):
            line = abi.describe_table_stats(m, keys, actions)
            assert line.startswith("table_stats_kernel<lds> grid="), line
            f = _fields(line)
            assert f["lds"] == 16 * bins <= 64 << 10 and f["bins"] == bins and f["block"] == 256, line
            assert f["grid"] == min(-(-m // 1024), 1024), line             # four samples per lane and turn, capped
    for keys, actions in ((4097, 1), (14641, 4), (1025, 4), (1 << 28, 1), ((1 << 28) // 255, 255)):
        for m in (1, 64 * 4099, 16 << 20, 1 << 34):
            line = abi.describe_table_stats(m, keys, actions)
            assert line.startswith("table_stats_kernel<global> grid="), line
            f = _fields(line)
            assert f["lds"] == 0 and f["bins"] == keys * actions and f["block"] == 256, line
            assert f["grid"] == min(-(-m // 1024), 2048), line
    assert _fields(abi.describe_table_stats(16 << 20, 121, 4))["grid"] == _fields(abi.describe_table_stats(1 << 34, 121, 4))["grid"]
    assert abi.describe_table_stats(0, 121, 4) == "" and abi.describe_table_stats(0, 14641, 4) == ""


def test_describe_table_stats_refusals(abi):
    d = abi.lib.lmaze_describe_table_stats
    buf = C.create_string_buffer(256)
    assert d(100, 121, 4, None, 256) == E_NULL
    assert d(100, 121, 4, buf, 0) == E_NULL
    assert d(-1, 0, 0, None, 256) == E_NULL                            # before the counts
    assert d(-1, 121, 4, buf, 256) == E_COUNT
    assert d(100, 0, 4, buf, 256) == E_COUNT
    assert d(100, 121, 0, buf, 256) == E_COUNT
    assert d(100, 121, 256, buf, 256) == E_COUNT
    assert d(100, (1 << 28) // 4 + 1, 4, buf, 256) == E_COUNT
    assert d(0, 0, 4, buf, 256) == E_COUNT                             # before the empty line
    buf.value = b"stale"
    assert d(0, 121, 4, buf, 256) == 0 and buf.value == b""
    assert d(100, 121, 4, buf, 8) == 0 and buf.value == b"table_s"     # truncated to len, always terminated


# ------------------------------------------------------------- lmaze_learn.h on the host
@pytest.fixture(scope="module")
def learn_host(tmp_path_factory):
    """tests/csrc/learn_host.cpp: a stand-alone program around lmaze_learn.h, built with the address and undefined-behaviour
    sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("learn")
    exe = str(tmp / "learn_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "learn_host.cpp")])

    def run(mode, *arrays):
        src, dst = str(tmp / (mode + ".in")), str(tmp / (mode + ".out"))
        with open(src, "wb") as fh:
            for a in arrays:
                fh.write(np.ascontiguousarray(a).tobytes())
        out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        return open(dst, "rb").read()
    return run


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("gamma,lam", [(0.0, 0.0), (0.99, 0.95), (1.0, 1.0)])
def test_host_gae_step_is_the_numpy_loop(learn_host, gamma, lam):
    """10^5 random samples (T = 25 rows of 4000 envs): rewards from the reference's literals -0.0, -0.01, -1, 100 and random
    ones, a tenth of the rows done, values of both signs -- advantage and target bit for bit."""
    rs = np.random.RandomState(11)
    T, n = 25, 4000
    reward = rs.choice(np.array([-0.0, -0.01, -1.0, 100.0, 0.37], np.float32), (T, n))
    other = rs.rand(T, n) < 0.2
    reward[other] = (rs.randn(int(other.sum())) * 5).astype(np.float32)
    done = (rs.rand(T, n) < 0.1).astype(np.uint8)
    value = (rs.randn(T + 1, n) * 30).astype(np.float32)
    value[rs.rand(T + 1, n) < 0.1] = 0.0
    raw = learn_host("gae", np.array([T, n], np.int32), np.array([gamma, lam], np.float32), reward, done, value)
    got = np.frombuffer(raw, np.uint32).reshape(2, T, n)
    adv, tgt = R.gae_numpy(reward, done, value[:T], value[T], gamma, lam)
    assert (got[0] == _bits(adv)).all() and (got[1] == _bits(tgt)).all()
    assert len(np.unique(got[0])) > 1000                              # not a constant


def test_host_gae_done_row_keeps_the_sign_of_zero(learn_host):
    """reward -0.0, value +0.0 on a done row: -0.0 - 0.0 = -0.0, which "+ gamma * 0" would turn into +0.0."""
    reward = np.array([[-0.0, -0.0, 100.0]], np.float32)
    done = np.array([[1, 0, 1]], np.uint8)
    value = np.zeros((2, 3), np.float32)
    raw = learn_host("gae", np.array([1, 3], np.int32), np.array([0.99, 0.95], np.float32), reward, done, value)
    got = np.frombuffer(raw, np.uint32).reshape(2, 1, 3)
    assert got[0, 0].tolist() == [0x80000000, 0x00000000, 0x42C80000]
    adv, _ = R.gae_numpy(reward, done, value[:1], value[1], 0.99, 0.95)
    assert (got[0] == _bits(adv)).all()


def _q24(learn_host, w):
    w = np.ascontiguousarray(w, dtype=np.float32)
    raw = learn_host("q24", np.array([len(w)], np.int64), w)
    return np.frombuffer(raw[:len(w)], np.uint8).astype(bool), np.frombuffer(raw[len(w):], np.int64)


def test_host_q24_special_weights(learn_host):
    t = 2.0 ** -25
    w = np.array([t, -t, 3 * t, -0.0, 2.0 ** 31, np.nan, np.inf, -np.inf, -(2.0 ** 31), 1.0, -1.0, 0.5 + t, 1.5 * 2.0 ** -24,
                  2.5 * 2.0 ** -24, -2.5 * 2.0 ** -24, np.float32(2.0 ** 31) - 128.0, 1e-45, -1e-45, 1.17549435e-38],
                 np.float32)
    ok, q = _q24(learn_host, w)
    assert ok.tolist() == [True, True, True, True, False, False, False, False, False] + [True] * 10
    assert q.tolist() == [0, 0, 2, 0, 0, 0, 0, 0, 0, 1 << 24, -(1 << 24), 1 << 23, 2, 2, -2, (1 << 55) - (1 << 31), 0, 0, 0]
    assert (ok == R.q24_ok(w)).all() and (q == R.q24(w)).all()


def test_host_q24_is_rint_of_the_double_product(learn_host):
    """10^5 random weights over every magnitude up to 2^31 and beyond, halves of 2^-24 (the ties) among them."""
    rs = np.random.RandomState(12)
    w = (rs.randn(100000) * np.exp2(rs.randint(-40, 34, 100000))).astype(np.float32)
    w[:20000] = ((rs.randint(-(1 << 20), 1 << 20, 20000) * 2 + 1) * 2.0 ** -25).astype(np.float32)     # odd multiples of 2^-25
    w[20000:20100] = rs.choice(np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, -(2.0 ** 31), 3e9], np.float32), 100)
    ok, q = _q24(learn_host, w)
    assert (ok == R.q24_ok(w)).all() and (q == R.q24(w)).all()
    assert 0.5 < ok.mean() < 1.0


def test_host_table_bin(learn_host):
    rs = np.random.RandomState(13)
    for keys, actions in ((121, 4), (4097, 1), (14641, 4), ((1 << 28) // 255, 255)):
        key = rs.randint(-3, keys + 3, 20000).astype(np.int32)
        act = rs.randint(-1, actions + 2, 20000).astype(np.int32)
        key[:4] = (-1, keys, np.iinfo(np.int32).max, np.iinfo(np.int32).min)
        act[4:8] = (-1, actions, np.iinfo(np.int32).max, np.iinfo(np.int32).min)
        raw = learn_host("bin", np.array([len(key)], np.int64), np.array([keys, actions], np.uint32), key, act)
        got = np.frombuffer(raw, np.int32)
        good = (key >= 0) & (key < keys) & (act >= 0) & (act < actions)
        want = np.where(good, key.astype(np.int64) * actions + act, -1)
        assert (got == want).all() and 0.2 < good.mean() < 1.0


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_no_scratch_full_occupancy_and_no_fma(tmp_path):
    """lmaze_aux.hip for gfx950: both forms of advantages_kernel and of table_stats_kernel without scratch at 8 waves per
    SIMD; the GAE chain holds no fused multiply-add; the LDS form accumulates with LDS atomics, the global form with global
    ones."""
    asm = str(tmp_path / "aux.s")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "lmaze_aux.hip"), "-o", asm],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    mine = {k: v for k, v in kernels.items() if "advantages_kernel" in k or "table_stats_kernel" in k}
    assert len(mine) == 4 and sum("advantages" in k for k in mine) == 2, sorted(kernels)
    for name, v in mine.items():
        assert v.get("ScratchSize", 0) == 0 and v["Occupancy"] >= 8, (name, v)
    text = open(asm).read()

    def ops(name):
        body = text.split("\n%s:" % name, 1)[1].split(".Lfunc_end", 1)[0]
        return re.findall(r"^\s+([a-z][a-z_0-9]+)", body, re.M)
    for name in mine:
        got = ops(name)
        if "advantages" in name:
            fused = [o for o in got if re.search(r"(fma|mac|mad)\w*_(f16|f32|f64|legacy)", o)]      # integer mads index the rows
            assert not fused and sum(o.startswith("v_mul_f32") for o in got) >= 16, (name, fused)
            assert sum(o.startswith("global_store") for o in got) >= 16, name      # eight rows, two outputs
        elif "ILb1E" in name:
            assert any(o.startswith("ds_add_u64") for o in got) and any(o.startswith("global_atomic_add_x2") for o in got), name
        else:
            assert any(o.startswith("global_atomic_add_x2") for o in got) and not any(o.startswith("ds_") for o in got), name
