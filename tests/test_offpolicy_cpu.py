"""CPU: the off-policy entry points (lmaze_action_probs, lmaze_vtrace, lmaze_vtrace_table) without a GPU -- the arithmetic of
lmaze_offpolicy.h compiled for the host and compared bit for bit with its numpy restatement (offpolicy_ref.py); the
restatement against the pinned action laws (policy_law.py), against GAE (tabular_ref.py), against V-trace's closed form and
against one sweep of evaluate_ref; every documented refusal in its order, answered before any device call; and what the
kernels need per wave."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import evaluate_ref as E
import helpers as H
import offpolicy_ref as R
import policy_law as L
import solve_ref as SR
import tabular_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-lmaze_amd", "csrc")
E_NULL, E_COUNT, E_ALIGN = -1, -5, -6
MAX_ENVS = 1 << 30
F = np.float32
U = 2.0 ** -24                       # the unit roundoff of float32
INF = float("inf")


@pytest.fixture(scope="module")
def abi():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return importlib.import_module("gym-lmaze_amd._abi")


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


# ------------------------------------------------------------- lmaze_offpolicy.h on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/csrc/offpolicy_host.cpp: a stand-alone program around lmaze_offpolicy.h, built with the address and
    undefined-behaviour sanitizers and run as a program (it is never loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("offpolicy")
    exe = str(tmp / "offpolicy_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "offpolicy_host.cpp")])

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


def host_weights(host, kind, table, eps32, key, act):
    m = len(key)
    raw = host("weights", np.array([m, len(table)], np.int64), np.array([R.FORMS[kind]], np.int32), np.array([eps32], np.uint32),
               table, key, act)
    return np.frombuffer(raw[:8 * m], np.uint64).astype(np.int64), np.frombuffer(raw[8 * m:], np.uint32)


@pytest.mark.parametrize("keys", [1, 121, 14641])
def test_host_weights_and_probs_are_the_restatement(host, keys):
    tables = R.special_tables(keys, keys)
    key, act = R.special_samples(keys, 20000, keys + 1)
    seen = set()
    for kind, table in tables.items():
        for e in (R.EPSILONS if kind != "thresholds" else (0,)):
            w, p = host_weights(host, kind, table, e, key, act)
            want = R.weights(kind, table, key, act, e)
            assert (w == want).all(), (kind, e)
            assert (p == _bits(R.probs(want))).all(), (kind, e)
            assert (want >= 0).all() and (want <= 1 << 34).all()
            inside = (key >= 0) & (key < keys)
            assert (want[~inside] == 0).all() and (want[inside] > 0).any()
            seen.update(np.unique(p).tolist())
    assert 0 in seen and len(seen) >= 3


def test_host_ratios_are_the_restatement(host):
    rs = np.random.RandomState(5)
    m = 50000
    wt = rs.randint(0, (1 << 34) + 1, m, dtype=np.int64)
    wb = rs.randint(0, (1 << 34) + 1, m, dtype=np.int64)
    wb[:1000] = 0
    wt[500:2000] = 0
    wb[2000:3000] = wt[2000:3000]
    wt[3000:3010] = 1 << 34
    wb[3000:3005] = 1
    wt[3010:3020] = (1 << 25) + 1 + 2 * np.arange(10)                  # halfway cases of the conversion: ties go to even
    raw = host("ratio", np.array([m], np.int64), wt.astype(np.uint64), wb.astype(np.uint64))
    got = np.frombuffer(raw, np.uint32)
    want = R.ratios(wt, wb)
    assert (got == _bits(want)).all()
    assert (want[:1000] == 0).all() and (want[2000:3000][wb[2000:3000] != 0] == 1).all()
    assert want[3000] == F(2.0 ** 34)


@pytest.mark.parametrize("rho_bar,c_bar", [(1.0, 1.0), (INF, INF), (2.0, 0.5)])
@pytest.mark.parametrize("gamma,lam", [(0.0, 0.0), (0.99, 0.95), (1.0, 1.0)])
def test_host_vtrace_walk_is_the_numpy_loop(host, gamma, lam, rho_bar, c_bar):
    T, n = 25, 2000
    reward, done, value, tail, ratio = R.special_rows(T, n, 0.1, 21)
    raw = host("vtrace", np.array([T, n], np.int32), np.array([gamma, lam, rho_bar, c_bar], F), reward, done,
               np.concatenate([value, tail[None]]), ratio)
    got = np.frombuffer(raw, np.uint32).reshape(2, T, n)
    vs, pg = R.vtrace_numpy(reward, done, value, tail, ratio, gamma, lam, rho_bar, c_bar)
    assert (got[0] == _bits(vs)).all() and (got[1] == _bits(pg)).all()
    assert len(np.unique(got[0])) > 1000
    # the done row with r = -0.0 and v = 0 keeps its sign: acc = 1 * (-0.0 - 0.0) = -0.0, vs = -0.0 + 0.0 = +0.0, pg = -0.0
    assert got[1, 0, 0] == 0x80000000 and got[0, 0, 0] == 0


# ------------------------------------------------------------- the law is the pinned one
def test_threshold_weights_are_the_sampling_law():
    rs = np.random.RandomState(31)
    rows = rs.randint(0, 1 << 32, (4000, 4), dtype=np.int64).astype(np.uint32)
    rows[:9] = R.special_tables(9, 0)["thresholds"]
    rows[1000:2000, :3] = np.sort(rows[1000:2000, :3], axis=1)
    law = L.sampling_law(rows)
    key = np.repeat(np.arange(len(rows)), 4)
    act = np.tile(np.arange(4), len(rows))
    w = R.weights("thresholds", rows, key, act).reshape(-1, 4)
    assert (w == 4 * law).all()
    for a in (-1, 4, 5, 255):
        assert (R.weights("thresholds", rows, np.arange(len(rows)), np.full(len(rows), a)) == 0).all()


@pytest.mark.parametrize("eps32", R.EPSILONS)
def test_policy_weights_are_the_epsilon_greedy_law(eps32):
    """every byte 0 .. 255: the four moves, and the byte itself when it is above 3 -- column 4 of the law"""
    entries = np.arange(256, dtype=np.uint8)
    law = L.epsilon_greedy_law(entries, eps32)
    key = np.repeat(np.arange(256), 4)
    w = R.weights("policy", entries, key, np.tile(np.arange(4), 256), eps32).reshape(256, 4)
    assert (w == law[:, :4]).all()
    own = R.weights("policy", entries, np.arange(256), np.arange(256), eps32)
    assert (own[4:] == law[4:, 4]).all() and (own[:4] == law[np.arange(4), np.arange(4)]).all()
    assert (w.sum(1)[:4] == 1 << 34).all() and ((w.sum(1) + own)[4:] == 1 << 34).all()
    # q: the same rule through the first maximum
    q = R.special_tables(10, 0)["q"]
    greedy = E.first_max(q)
    kq = np.repeat(np.arange(len(q)), 4)
    wq = R.weights("q", q, kq, np.tile(np.arange(4), len(q)), eps32).reshape(-1, 4)
    assert (wq == L.epsilon_greedy_law(greedy, eps32)[:, :4]).all()


# ------------------------------------------------------------- on-policy is GAE
@pytest.mark.parametrize("rho_bar,c_bar", [(1.0, 1.0), (INF, INF)])
@pytest.mark.parametrize("gamma,lam", [(0.0, 0.0), (0.99, 0.95), (1.0, 1.0)])
@pytest.mark.parametrize("T,N", [(1, 1), (9, 257), (13, 777)])
def test_on_policy_vtrace_is_gae(T, N, gamma, lam, rho_bar, c_bar):
    reward, done, value, tail, _ = R.special_rows(T, N, 0.1, T + N)
    adv, tgt = TR.gae_numpy(reward, done, value, tail, gamma, lam)
    for ratio in (None, np.ones((T, N), F)):
        vs, _ = R.vtrace_numpy(reward, done, value, tail, ratio, gamma, lam, rho_bar, c_bar)
        assert (_bits(vs) == _bits(tgt)).all() and (_bits(vs) == _bits(adv + value)).all()


# ------------------------------------------------------------- the reference is V-trace
def test_restatement_is_the_closed_form_of_vtrace():
    """vs - v = sum_k gamma^k (prod_{i<k} c_(t+i)) delta_(t+k), cut at done rows, delta = rho (r + gamma v' - v), in float64
    from the float32 rows.  The bound: a step makes 8 roundings (c, boot, tg, td, delta, gc, trace, acc), each of relative size
    U on a quantity no larger than MAG = T rho_bar (|r| + gamma |v| + |v|)_max, the bound on |acc|; an error made at row t + k
    reaches row t scaled by prod gamma c <= 1 here (gamma lambda c_bar < 1), so at most T steps' errors add up, and vs = acc + v
    rounds once more: (8 T + 1) U MAG."""
    T, N, gamma, lam, rho_bar, c_bar = 12, 64, 0.99, 0.95, 2.0, 0.5
    reward, done, value, tail, ratio = R.special_rows(T, N, 0.1, 77)
    ratio = np.where(np.isfinite(ratio), ratio, F(3.5)).astype(F)
    vs, _ = R.vtrace_numpy(reward, done, value, tail, ratio, gamma, lam, rho_bar, c_bar)
    g, lm = float(F(gamma)), float(F(lam))
    r64, v64, x64 = reward.astype(np.float64), np.concatenate([value, tail[None]]).astype(np.float64), ratio.astype(np.float64)
    rho, c = np.minimum(x64, rho_bar), lm * np.minimum(x64, c_bar)
    td = np.where(done != 0, r64 - v64[:T], r64 + g * v64[1:] - v64[:T])
    delta = rho * td
    want = np.zeros((T, N))
    for t in range(T):
        coef, live = np.ones(N), np.ones(N, bool)          # gamma^k prod c, and whether no done row lies in t .. t + k - 1
        for k in range(T - t):
            want[t] += np.where(live, coef * delta[t + k], 0.0)
            live &= done[t + k] == 0
            coef = coef * g * c[t + k]
    mag = T * rho_bar * float((np.abs(r64) + g * np.abs(v64[1:]) + np.abs(v64[:T])).max())
    bound = (8 * T + 1) * U * mag
    err = np.abs((vs.astype(np.float64) - v64[:T]) - want).max()
    print("closed form: err %.3g bound %.3g" % (err, bound))
    assert err <= bound
    # the recursion with c and rho swapped: delta weighed by c, the trace by rho
    swapped = np.zeros((T + 1, N))
    for t in range(T - 1, -1, -1):
        swapped[t] = c[t] * td[t] + np.where(done[t] != 0, 0.0, g * rho[t] * swapped[t + 1])
    miss = np.abs(swapped[:T] - want).max()
    print("swapped: miss %.3g" % miss)
    assert miss > 100 * bound


# ------------------------------------------------------------- ties to evaluate(), deterministic
def test_expected_vtrace_target_is_one_sweep_of_evaluate():
    """Every (non-wall cell, action) pair of a v3 maze once, as a row of T = 1 with the model's reward, done and next key:
    with rho_bar = inf, sum_a mu(a|s) vs(s, a) = sum_a pi(a|s) (r + gamma v') - v + v = (T^pi v)(s), one evaluate_ref sweep of
    the target table from v.  The bound, with MAG = rho_max (|r| + gamma |v'| + |v|)_max: the vtrace side makes 3 roundings
    in the ratio (two conversions, one division; relative, on a product no larger than MAG) and 5 more (boot, tg, td, delta,
    vs), each no larger than U MAG, and the average over mu (weights that sum to 1) keeps that; the sweep makes 3 roundings
    in each probability, 2 in r + gamma v', 1 in each product and 3 in the sum: 8 + 9 = 17 roundings, (17 U MAG)."""
    G, gamma = 11, 0.9
    lay = H.bordered_random_layouts(1, G, 5)[0]
    goal = (G - 2, G - 3)
    model = SR.extract_model("v3", lay, goal)
    assert not model.sticky.any()
    S = G * G
    cells = np.flatnonzero(~model.wall)
    key = np.repeat(cells, 4).astype(np.int32)[None]
    act = np.tile(np.arange(4), len(cells)).astype(np.int32)[None]
    reward = model.r[key[0], act[0]][None].astype(F)
    done = model.terminal[key[0], act[0]][None].astype(np.uint8)
    nxt = model.nxt[key[0], act[0]]
    assert done.any() and not done.all()
    v = (np.random.RandomState(3).randn(S) * 10).astype(F)
    v[model.wall] = 0.0
    behaviour, target = R.min_law_table(S, 1), R.min_law_table(S, 2)
    wb, wt = R.weights("thresholds", behaviour, key, act), R.weights("thresholds", target, key, act)
    assert (wb >= 4 * R.MIN_LAW).all() and (wt >= 4 * R.MIN_LAW).all()
    ratio = R.ratios(wt, wb)
    _, want = E.sweep(model, gamma, E.probabilities(E.weights(thresholds=target), model.sticky, model.wall), v)
    mu = (wb[0] / float(1 << 34)).reshape(-1, 4)
    mag = float(ratio.max()) * float((np.abs(reward[0]) + gamma * np.abs(v[nxt]) + np.abs(v[key[0]])).max())
    bound = 17 * U * mag

    def expected(x):
        vs, _ = R.vtrace_numpy(reward, done, TR.table_values(v, key), TR.table_values(v, nxt), x, gamma, 0.0, INF, 1.0)
        return (mu * vs[0].astype(np.float64).reshape(-1, 4)).sum(1)
    err = np.abs(expected(ratio) - want[cells]).max()
    print("evaluate tie: err %.3g bound %.3g" % (err, bound))
    assert err <= bound
    with np.errstate(all="ignore"):
        for what, x in (("no ratio", None), ("inverted", (F(1) / ratio).astype(F))):
            miss = np.abs(expected(x) - want[cells]).max()
            print(what, "miss %.3g" % miss)
            assert miss > 100 * bound, what


# ------------------------------------------------------------- refusals
def test_action_probs_refusals_and_nothing_to_do(abi):
    f = abi.lib.lmaze_action_probs

    def call(key=64, act=64, m=100, policy=None, q=None, eps=0, thresholds=64, keys=121, prob=64):
        return f(key, act, m, policy, q, eps, thresholds, keys, prob, None)
    for name in ("key", "act", "prob"):
        assert call(**{name: None}) == E_NULL, name
        assert call(m=-1, keys=0, thresholds=None, **{name: None}) == E_NULL, name
    # exactly one table, before the counts
    assert call(thresholds=None) == E_NULL
    assert call(policy=64) == E_NULL and call(q=64) == E_NULL and call(policy=64, q=64, thresholds=None) == E_NULL
    assert call(thresholds=None, m=-1) == E_NULL and call(policy=64, keys=0, m=0) == E_NULL
    # the counts, before the alignments and before "nothing to do"
    assert call(m=-1) == E_COUNT and call(keys=0) == E_COUNT and call(keys=-3, m=0) == E_COUNT
    assert call(m=-1, thresholds=72) == E_COUNT
    # the alignments, before "nothing to do"
    assert call(thresholds=72) == E_ALIGN and call(thresholds=None, q=72) == E_ALIGN
    assert call(key=66) == E_ALIGN and call(act=65) == E_ALIGN and call(prob=67) == E_ALIGN
    assert call(m=0, thresholds=72) == E_ALIGN and call(m=0, key=66) == E_ALIGN
    assert call(thresholds=None, policy=65, m=0) == 0                  # a byte table has no alignment
    for kw in (dict(), dict(thresholds=None, q=64), dict(thresholds=None, policy=63, eps=7), dict(keys=1 << 40)):
        assert call(m=0, **kw) == 0, kw


def test_vtrace_refusals_and_nothing_to_do(abi):
    f = abi.lib.lmaze_vtrace
    ok = dict(reward=64, done=64, value=64, tail=None, rho=None, vs=64, pg=None)

    def call(T=5, n=10, **kw):
        a = dict(ok, **kw)
        return f(a["reward"], a["done"], a["value"], a["tail"], a["rho"], 0.99, 0.95, 1.0, 1.0, a["vs"], a["pg"], T, n, None)
    for name in ("reward", "done", "value", "vs"):
        assert call(**{name: None}) == E_NULL, name
        assert call(T=-1, n=-1, **{name: None}) == E_NULL, name
        assert call(T=0, **{name: None}) == E_NULL, name
    assert call(T=0, vs=None, pg=64) == 0                              # one output is enough
    assert call(T=-1) == E_COUNT and call(n=-1) == E_COUNT and call(n=MAX_ENVS + 1) == E_COUNT
    assert call(T=-1, n=0) == E_COUNT and call(T=0, n=-1) == E_COUNT and call(T=-1, reward=66) == E_COUNT
    for name in ("reward", "value", "tail", "rho", "vs", "pg"):
        assert call(**{name: 66}) == E_ALIGN, name
        assert call(T=0, **{name: 66}) == E_ALIGN, name               # before "nothing to do"
    assert call(T=0, done=65) == 0                                     # bytes have no alignment
    for T, n in ((0, 10), (5, 0), (0, 0), (0, MAX_ENVS)):
        assert call(T=T, n=n) == 0 and call(T=T, n=n, tail=64, rho=64, pg=64) == 0


def test_vtrace_table_refusals_and_nothing_to_do(abi):
    f = abi.lib.lmaze_vtrace_table
    ok = dict(reward=64, done=64, key=64, act=64, key_tail=None, values=64, b_policy=None, b_q=None, b_th=64, t_policy=None,
              t_q=64, t_th=None, vs=64, pg=None, rho_out=None)

    def call(T=5, n=10, keys=121, **kw):
        a = dict(ok, **kw)
        return f(a["reward"], a["done"], a["key"], a["act"], a["key_tail"], a["values"], keys, a["b_policy"], a["b_q"], 0,
                 a["b_th"], a["t_policy"], a["t_q"], 7, a["t_th"], 0.99, 0.95, 1.0, 1.0, a["vs"], a["pg"], a["rho_out"], T, n, None)
    for name in ("reward", "done", "key", "act", "values", "vs"):
        assert call(**{name: None}) == E_NULL, name
        assert call(T=-1, keys=0, b_th=None, **{name: None}) == E_NULL, name
        assert call(n=0, **{name: None}) == E_NULL, name
    assert call(T=0, vs=None, pg=64) == 0 and call(T=0, vs=None, rho_out=64) == E_NULL
    # exactly one form per table: the behaviour table first, then the target, both before the counts
    assert call(b_th=None) == E_NULL and call(b_policy=64) == E_NULL and call(b_q=64) == E_NULL
    assert call(t_q=None) == E_NULL and call(t_th=64) == E_NULL and call(t_policy=64) == E_NULL
    assert call(b_th=None, T=-1) == E_NULL and call(t_q=None, keys=0, n=0) == E_NULL
    assert call(T=-1) == E_COUNT and call(n=-1) == E_COUNT and call(n=MAX_ENVS + 1) == E_COUNT
    for keys in (0, -1, -(1 << 40)):
        assert call(keys=keys) == E_COUNT and call(keys=keys, T=0) == E_COUNT and call(keys=keys, n=0) == E_COUNT
    assert call(T=-1, b_th=72) == E_COUNT                             # the counts before the alignments
    assert call(b_th=72) == E_ALIGN and call(t_q=72) == E_ALIGN and call(T=0, b_th=72) == E_ALIGN
    for name in ("reward", "key", "act", "key_tail", "values", "vs", "pg", "rho_out"):
        assert call(**{name: 66}) == E_ALIGN, name
        assert call(n=0, **{name: 66}) == E_ALIGN, name
    for T, n in ((0, 10), (5, 0), (0, 0), (0, MAX_ENVS)):
        for keys in (1, 121, 1 << 40):
            assert call(T=T, n=n, keys=keys) == 0
            assert call(T=T, n=n, keys=keys, b_th=None, b_policy=63, t_q=None, t_policy=61, key_tail=64, pg=64, rho_out=64) == 0


def test_symbols_and_python_surface(abi):
    header = open(os.path.join(ROOT, "include", "lmaze.h")).read()
    for name in ("lmaze_action_probs", "lmaze_vtrace", "lmaze_vtrace_table"):
        assert name in abi.SYMBOLS and hasattr(abi.lib, name) and name + "(" in header
    assert abi.lib.lmaze_abi_version() == 4 == abi.ABI_VERSION
    pkg = importlib.import_module("gym-lmaze_amd")
    for name in ("table_policy", "action_probs", "vtrace"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("no exclusion and no renormalisation", "carries its greedy share", "one correctly rounded division",
                   "Equal tables give exactly 1", "A NaN ratio is clipped to the bars"):
        assert phrase in flat, phrase


def test_table_policy_records():
    """the record is built by the rules the rollouts convert by, host side: no GPU needed"""
    import torch
    pkg = importlib.import_module("gym-lmaze_amd")
    ABI = importlib.import_module("gym-lmaze_amd._abi")
    probs = torch.rand(121, 4, dtype=torch.float64) + 0.01
    rec = pkg.table_policy(probs=probs)
    assert rec.kind == "thresholds" and rec.keys == 121 and rec.epsilon_u32 == 0
    assert torch.equal(rec.table.view(torch.int32), ABI.sampling_thresholds(probs).view(torch.int32))
    logits = torch.randn(121, 4)
    rec = pkg.table_policy(logits=logits, temperature=0.5, keys=121)
    assert torch.equal(rec.table.view(torch.int32),
                       ABI.sampling_thresholds(torch.softmax(logits.double() / 0.5, -1)).view(torch.int32))
    th = rec.table
    assert pkg.table_policy(thresholds=th).table is th                 # the caller's memory, never a copy
    by = torch.randint(0, 6, (121,), dtype=torch.uint8)
    rec = pkg.table_policy(policy=by, epsilon=0.1)
    assert rec.kind == "policy" and rec.table is by and rec.epsilon_u32 == ABI.epsilon_u32(0.1)
    q = torch.randn(121, 4)
    rec = pkg.table_policy(q=q, epsilon=1.0)
    assert rec.kind == "q" and rec.table is q and rec.epsilon_u32 == (1 << 32) - 1
    with pytest.raises(AttributeError):
        rec.table = by
    for kw in (dict(), dict(policy=by, q=q), dict(probs=probs, epsilon=0.1), dict(thresholds=th, epsilon=0.5), dict(policy=by, keys=120),
               dict(q=q.double()), dict(q=q[:, :3]), dict(policy=by.view(11, 11)), dict(logits=logits, temperature=0.0),
               dict(policy=by, epsilon=1.5), dict(thresholds=th[:, :3]), dict(probs=-probs)):
        with pytest.raises(ValueError):
            pkg.table_policy(**kw)


# ------------------------------------------------------------- what the kernels need per wave
@pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not installed")
def test_offpolicy_kernels_use_no_scratch():
    usage = H.kernel_usage("lmaze_offpolicy.hip")
    probs = [k for k in usage if "action_probs_kernel" in k]
    walks = [k for k in usage if "vtrace_kernel" in k]
    assert len(probs) == 3 and len(walks) == 10 and len(usage) == 13, sorted(usage)     # one per form; rows + 3 x 3 forms
    for name, v in usage.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
