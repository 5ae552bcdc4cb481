"""The learner-side kernels (gae: lmaze_advantages / lmaze_advantages_table; table_stats: lmaze_table_stats) against what a
user writes in torch without them, interleaved rounds in one process, HIP events after warm-up, medians.  Per shape of rows
[T, N] and per table (an 11x11 ball-keyed one, 121 keys: table_stats in LDS; a goal-keyed one, 14 641 keys: global atomics):
    gae rows    gae(reward_t, done_t, gamma, lam, value_t=, tail=)   against the torch reverse loop over value rows
    gae table   gae(..., values=, key_t=, key_tail=)                 against the same loop behind V[key_t.long()]
    stats       table_stats(key_t, actions_t, weight_t, ...)         against torch.bincount(bin) and bincount(bin, weights=)
                                                                     (float64 sums: not reproducible bit for bit)
    count       table_stats(key_t, actions_t, ...)                   against torch.bincount(bin)
Each kernel figure is also given as bytes moved / the box's own copy ceiling (lmaze_bandwidth_probe, 512 MiB copy: read +
write bytes per second), the bytes being the rows read and written once.

    python tools/bench_tabular.py --out profiles/tabular/bench_tabular.json [--rounds 5]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = importlib.import_module("gym-lmaze_amd")

ROWS = ((64, 65536), (16, 1 << 20))
TABLES = (("ball 11x11", 121), ("goal 11x11", 14641))
GAMMA, LAM, ACTIONS = 0.99, 0.95, 4


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def _rounds(fns, rounds):
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):         # interleaved
        for k, f in fns.items():
            times[k].append(_timed(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {k: {"us": round(med[k], 3), "spread": [round(min(v), 3), round(max(v), 3)]} for k, v in times.items()}


def copy_ceiling(dev, rounds):
    """bytes per second (read + write) of the library's own copy probe over 512 MiB."""
    nbytes = 512 << 20
    src, dst = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def probe():
        PKG._abi.check("lmaze_bandwidth_probe", PKG._abi.lib.lmaze_bandwidth_probe(src.data_ptr(), dst.data_ptr(), nbytes, stream))
    med, _ = _rounds({"copy": probe}, max(rounds, 5))
    return 2 * nbytes / (med["copy"] * 1e-6)


def _torch_gae(reward, done, value, tail):
    T = reward.shape[0]
    adv_t, tgt_t = torch.empty_like(reward), torch.empty_like(reward)
    adv, v_next = torch.zeros_like(tail), tail
    for t in range(T - 1, -1, -1):
        v = value[t]
        adv = torch.where(done[t], reward[t] - v, reward[t] + GAMMA * v_next - v + (GAMMA * LAM) * adv)
        adv_t[t] = adv
        tgt_t[t] = adv + v
        v_next = v
    return adv_t, tgt_t


def bench(T, n, name, keys, rounds, ceiling, dev):
    g = torch.Generator(device=dev).manual_seed(n + keys)
    reward = torch.randn((T, n), device=dev, generator=g)
    done = torch.rand((T, n), device=dev, generator=g) < 0.05
    value_t = torch.randn((T, n), device=dev, generator=g)
    tail = torch.randn(n, device=dev, generator=g)
    values = torch.randn(keys, device=dev, generator=g)
    key_t = torch.randint(0, keys, (T, n), dtype=torch.int32, device=dev, generator=g)
    key_tail = torch.randint(0, keys, (n,), dtype=torch.int32, device=dev, generator=g)
    act_t = torch.randint(0, ACTIONS, (T, n), dtype=torch.int32, device=dev, generator=g)
    adv, tgt = torch.empty_like(reward), torch.empty_like(reward)
    count = torch.zeros((keys, ACTIONS), dtype=torch.int64, device=dev)
    total = torch.zeros((keys, ACTIONS), dtype=torch.int64, device=dev)
    bins = keys * ACTIONS

    def torch_bins():
        return (key_t.long() * ACTIONS + act_t.long()).reshape(-1)

    fns = {
        "gae_rows": lambda: PKG.gae(reward, done, GAMMA, LAM, value_t=value_t, tail=tail, out=adv, targets=tgt),
        "gae_rows_torch": lambda: _torch_gae(reward, done, value_t, tail),
        "gae_table": lambda: PKG.gae(reward, done, GAMMA, LAM, values=values, key_t=key_t, key_tail=key_tail, out=adv, targets=tgt),
        "gae_table_torch": lambda: _torch_gae(reward, done, values[key_t.long()], values[key_tail.long()]),
        "stats": lambda: PKG.table_stats(key_t, act_t, reward, keys=keys, actions=ACTIONS, count=count, total=total),
        "stats_torch": lambda: (torch.bincount(torch_bins(), minlength=bins),
                                torch.bincount(torch_bins(), weights=reward.reshape(-1).double(), minlength=bins)),
        "count": lambda: PKG.table_stats(key_t, act_t, keys=keys, actions=ACTIONS, count=count),
        "count_torch": lambda: torch.bincount(torch_bins(), minlength=bins),
    }
    med, out = _rounds(fns, rounds)
    m = T * n
    moved = {"gae_rows": 17 * m + 4 * n, "gae_table": 17 * m + 4 * n, "stats": 12 * m, "count": 8 * m}    # rows read + written once
    return {"rows": "%dx%d" % (T, n), "T": T, "n": n, "table": name, "keys": keys, "actions": ACTIONS,
            "stats_launch": PKG._abi.describe_table_stats(m, keys, ACTIONS), "us_per_call": out,
            "bytes": moved,
            "fraction_of_copy_ceiling": {k: round(b / (med[k] * 1e-6) / ceiling, 3) for k, b in moved.items()},
            "torch_over_kernel": {k: round(med[k + "_torch"] / med[k], 1) for k in moved}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ceiling = copy_ceiling(dev, args.rounds)
    print(json.dumps({"copy_ceiling_TB_per_s": round(ceiling / 1e12, 3)}), flush=True)
    res = []
    for T, n in ROWS:
        for name, keys in TABLES:
            r = bench(T, n, name, keys, args.rounds, ceiling, dev)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "copy_ceiling_bytes_per_s": ceiling, "rounds": args.rounds,
                       "results": res}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
