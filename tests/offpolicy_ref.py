"""numpy restatements of include/lmaze.h's off-policy rules (lmaze_action_probs, lmaze_vtrace, lmaze_vtrace_table), shared by
test_offpolicy_cpu.py (against the host build of lmaze_offpolicy.h) and test_gpu_offpolicy.py (against the kernels).  The
weights are exact integers in units of 2^-34; every float32 numpy operation is one rounding, in the header's order."""
import numpy as np

F = np.float32
TWO32 = 1 << 32
FORMS = {"thresholds": 0, "policy": 1, "q": 2}          # lmaze_offpolicy.h's LMAZE_LAW_*


def q_first_max(q):
    """The first maximum of every row of q[n, 4] by a strict '>' from a = 0 on: a NaN never wins, nothing beats a NaN in word 0."""
    q = np.asarray(q, dtype=F).reshape(-1, 4)
    best, act = q[:, 0].copy(), np.zeros(len(q), np.int64)
    with np.errstate(invalid="ignore"):
        for a in range(1, 4):
            better = q[:, a] > best
            best = np.where(better, q[:, a], best)
            act = np.where(better, a, act)
    return act


def weights(kind, table, key, action, eps32=0):
    """int64, shaped like key: the weight in units of 2^-34 with which the table rule records `action` at `key`.  kind
    "thresholds" (uint32 or int32 bits [S, 4]), "policy" (uint8[S]) or "q" (float32[S, 4]), the last two with eps32."""
    key, action = np.asarray(key, dtype=np.int64), np.asarray(action, dtype=np.int64)
    S = len(table)
    inside = (key >= 0) & (key < S)
    at = np.where(inside, key, 0).reshape(-1)
    a = action.reshape(-1)
    move = (a >= 0) & (a <= 3)
    if kind == "thresholds":
        rows = np.ascontiguousarray(table).reshape(-1, 4).view(np.uint32)[at]
        s = np.sort(rows[:, :3].astype(np.int64), axis=1)
        edges = np.concatenate([np.zeros((len(at), 1), np.int64), s, np.full((len(at), 1), TWO32, np.int64)], axis=1)
        ai = np.where(move, a, 0)
        who = np.arange(len(at))
        w = np.where(move, 4 * (edges[who, ai + 1] - edges[who, ai]), 0)
    else:
        greedy = (np.asarray(table, dtype=np.uint8).reshape(-1).astype(np.int64)[at] if kind == "policy"
                  else q_first_max(np.asarray(table, dtype=F).reshape(-1, 4)[at]))
        e = int(eps32)
        w = np.where(move, e, 0) + np.where(a == greedy, 4 * (TWO32 - e), 0)
    return np.where(inside.reshape(-1), w, 0).astype(np.int64).reshape(key.shape)


def probs(w):
    """p = fl(w) * 2^-34: the conversion rounds to nearest even, the scaling is exact."""
    return (np.asarray(w, dtype=np.int64).astype(F) * F(2.0 ** -34)).astype(F)


def ratios(w_target, w_behaviour):
    """fl(fl(wt) / fl(wb)), 0 where wb == 0."""
    wt, wb = np.asarray(w_target, dtype=np.int64), np.asarray(w_behaviour, dtype=np.int64)
    with np.errstate(all="ignore"):
        return np.where(wb != 0, wt.astype(F) / np.where(wb != 0, wb, 1).astype(F), F(0)).astype(F)


def vtrace_numpy(reward, done, value, v_tail, ratio, gamma, lam, rho_bar, c_bar):
    """V-trace in float32, every numpy operation one rounding: (vs[T, n], pg[T, n]).  value[T, n] the values of the rows,
    v_tail[n] the value behind the last row (None: 0), ratio[T, n] the unclipped ratios (None: 1)."""
    reward, value = np.asarray(reward, dtype=F), np.asarray(value, dtype=F)
    T, n = reward.shape
    ratio = np.ones((T, n), F) if ratio is None else np.asarray(ratio, dtype=F)
    g, lm, rb, cb = F(gamma), F(lam), F(rho_bar), F(c_bar)
    v_next = np.zeros(n, F) if v_tail is None else np.asarray(v_tail, dtype=F)
    vs_next, acc_next = v_next, np.zeros(n, F)
    vs_t, pg_t = np.empty((T, n), F), np.empty((T, n), F)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            r, v, d = reward[t], value[t], np.asarray(done[t]) != 0
            rho = np.where(ratio[t] < rb, ratio[t], rb).astype(F)
            cc = np.where(ratio[t] < cb, ratio[t], cb).astype(F)
            c = lm * cc
            td_done = r - v
            boot = g * v_next
            tg = r + boot
            td = tg - v
            delta = rho * td
            gc = g * c
            trace = gc * acc_next
            acc = np.where(d, rho * td_done, delta + trace).astype(F)
            vs = acc + v
            qb = g * vs_next
            qv = np.where(d, r, r + qb).astype(F)
            qa = qv - v
            vs_t[t], pg_t[t] = vs, rho * qa
            v_next, vs_next, acc_next = v, vs, acc
    return vs_t, pg_t


# ------------------------------------------------------------- the inputs both suites share
INF = float("inf")


def special_tables(keys, seed):
    """{kind: table} of `keys` rows each, the special rows first (as many as fit): threshold rows out of order, with a word 0
    and a word 2^32 - 1, with equal words; bytes above 3; q rows with ties, a NaN in word 0 and elsewhere, +-inf."""
    rs = np.random.RandomState(seed)
    top = (1 << 32) - 1
    th = rs.randint(0, 1 << 32, (keys, 4), dtype=np.int64)
    th[::2, :3] = np.sort(th[::2, :3], axis=1)                        # every second row monotone, the others as they fell
    head = np.array([[0, 0, 0, 7], [top, top, top, 0], [0, 1 << 31, top, 1], [top, 0, 1 << 31, 2], [1 << 31, top, 0, 3],
                     [5, 5, 9, 4], [9, 5, 5, 5], [1 << 30, 1 << 31, 3 << 30, top], [3 << 30, 1 << 30, 1 << 31, 0]], np.int64)
    th[:min(keys, len(head))] = head[:keys]
    by = rs.randint(0, 4, keys).astype(np.uint8)
    hb = np.array([0, 1, 2, 3, 4, 5, 7, 255, 128], np.uint8)
    by[:min(keys, len(hb))] = hb[:keys]
    q = (rs.randn(keys, 4) * 3).astype(F)
    nan = np.nan
    hq = np.array([[1, 1, 1, 1], [0, 2, 2, 1], [nan, 5, 6, 7], [1, nan, 0, 0], [1, 2, nan, 3], [-INF, -INF, -INF, -INF],
                   [0, INF, INF, 1], [-0.0, 0.0, -1, -1], [3, 2, nan, INF], [nan, nan, nan, nan]], F)
    q[:min(keys, len(hq))] = hq[:keys]
    return {"thresholds": th.astype(np.uint32), "policy": by, "q": q}


def special_samples(keys, m, seed):
    """(key, action) int32[m]: keys -1, `keys` and the int32 extremes among those in range, actions -1 .. 5 and the extremes;
    every special row of special_tables() meets every action -1 .. 5."""
    rs = np.random.RandomState(seed)
    key = rs.randint(0, keys, m).astype(np.int32)
    act = rs.randint(-1, 6, m).astype(np.int32)
    grid = [(k, a) for k in range(min(keys, 10)) for a in range(-1, 6)]
    grid += [(k, a) for k in (-1, keys, keys + 7, np.iinfo(np.int32).max, np.iinfo(np.int32).min) for a in (0, 3)]
    grid += [(0, a) for a in (np.iinfo(np.int32).max, np.iinfo(np.int32).min, 255, 256 + 3, 4)]
    grid = grid[:m]
    key[:len(grid)] = [g[0] for g in grid]
    act[:len(grid)] = [g[1] for g in grid]
    return key, act


EPSILONS = (0, min(int(0.1 * 4294967296.0), 4294967295), (1 << 32) - 1)


def special_rows(T, N, done_rate, seed):
    """reward (the reference's literals -0.0, -0.01, -1, 100 and random ones), done, value rows with exact zeros, tail, and
    ratios in [0, 4] with 0, inf and NaN among them; a done row with r = -0.0 and v = 0 first."""
    rs = np.random.RandomState(seed)
    reward = rs.choice(np.array([-0.0, -0.01, -1.0, 100.0], F), (T, N))
    other = rs.rand(T, N) < 0.25
    reward[other] = (rs.randn(int(other.sum())) * 3).astype(F)
    done = (rs.rand(T, N) < done_rate).astype(np.uint8)
    value = (rs.randn(T, N) * 20).astype(F)
    value[rs.rand(T, N) < 0.2] = 0.0
    tail = (rs.randn(N) * 20).astype(F)
    ratio = (rs.rand(T, N) * 4).astype(F)
    odd = rs.rand(T, N) < 0.1
    ratio[odd] = rs.choice(np.array([0.0, 1.0, INF, np.nan], F), int(odd.sum()))
    reward.flat[0], done.flat[0], value.flat[0], ratio.flat[0] = -0.0, 1, 0.0, 1.0
    return reward, done, value, tail, ratio


MIN_LAW = 1 << 27                    # every action has probability >= 2^-5 in every row


def min_law_table(entries, seed):
    """uint32[entries, 4]: four gaps of 2^27 and a random split of the rest, the words of every second row out of order"""
    rs = np.random.RandomState(seed)
    rest = (1 << 32) - 4 * MIN_LAW
    c = np.sort(rs.randint(0, rest + 1, (entries, 3), dtype=np.int64), axis=1) + MIN_LAW * np.arange(1, 4)
    c[::2] = c[::2][:, [2, 0, 1]]
    rows = np.zeros((entries, 4), np.int64)
    rows[:, :3] = c
    rows[:, 3] = rs.randint(0, 1 << 32, entries, dtype=np.int64)
    return rows.astype(np.uint32)
