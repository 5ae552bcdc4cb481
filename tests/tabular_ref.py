"""numpy restatements of include/lmaze.h's learner-side rules (lmaze_advantages, lmaze_table_stats), shared by
test_tabular_cpu.py (against the host build of lmaze_learn.h) and test_gpu_tabular.py (against the kernels)."""
import numpy as np

F = np.float32
Q_ONE = 1 << 24


def table_values(values, keys):
    """values[key] where 0 <= key < len(values), 0 elsewhere (float32)."""
    keys = np.asarray(keys, dtype=np.int64)
    ok = (keys >= 0) & (keys < len(values))
    return np.where(ok, np.asarray(values, dtype=F)[np.where(ok, keys, 0)], F(0)).astype(F)


def gae_numpy(reward, done, value, v_tail, gamma, lam):
    """GAE(lambda) in float32, every numpy operation one rounding: (adv[T, n], target[T, n]).  value[T, n] the values of
    the rows, v_tail[n] the value behind the last row (None: 0)."""
    reward, value = np.asarray(reward, dtype=F), np.asarray(value, dtype=F)
    T, n = reward.shape
    g = F(gamma)
    gl = F(g * F(lam))
    v_next = np.zeros(n, F) if v_tail is None else np.asarray(v_tail, dtype=F)
    adv = np.zeros(n, F)
    out, tgt = np.empty((T, n), F), np.empty((T, n), F)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            v = value[t]
            boot = g * v_next
            target = reward[t] + boot
            delta = target - v
            trace = gl * adv
            adv = np.where(np.asarray(done[t]) != 0, reward[t] - v, delta + trace).astype(F)
            out[t] = adv
            tgt[t] = adv + v
            v_next = v
    return out, tgt


def q24_ok(w):
    w = np.asarray(w, dtype=F)
    with np.errstate(all="ignore"):
        return np.isfinite(w) & (np.abs(w.astype(np.float64)) < 2.0 ** 31)


def q24(w):
    """rint(float64(w) * 2^24) as int64 where q24_ok(w), 0 elsewhere."""
    w = np.asarray(w, dtype=F)
    ok = q24_ok(w)
    return np.rint(np.where(ok, w, F(0)).astype(np.float64) * float(Q_ONE)).astype(np.int64)


def table_stats_numpy(key, action, weight, keys, actions, count=None, total=None):
    """(count, total, kept): int64[keys, actions] tables with np.add.at, and the mask of the samples that were not skipped."""
    key = np.asarray(key, dtype=np.int64).ravel()
    action = np.zeros_like(key) if action is None else np.asarray(action, dtype=np.int64).ravel()
    kept = (key >= 0) & (key < keys) & (action >= 0) & (action < actions)
    if weight is not None:
        weight = np.asarray(weight, dtype=F).ravel()
        kept &= q24_ok(weight)
    bins = (key * actions + action)[kept]
    count = np.zeros((keys, actions), np.int64) if count is None else count.copy()
    np.add.at(count.reshape(-1), bins, 1)
    if weight is not None:
        total = np.zeros((keys, actions), np.int64) if total is None else total.copy()
        np.add.at(total.reshape(-1), bins, q24(weight)[kept])
    return count, total, kept
