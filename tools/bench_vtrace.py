"""The off-policy kernels (action_probs: lmaze_action_probs; vtrace: lmaze_vtrace / lmaze_vtrace_table) against the torch
composition they replace and against gae() at the same shape in the same run, interleaved rounds in one process, HIP events
after warm-up, medians.  Per shape of rows [T, N], per table size (an 11x11 ball-keyed one, 121 keys; a goal-keyed one,
14 641 keys) and per pairing of table forms (behaviour/target: thresholds/thresholds, policy/q):
    probs         action_probs(key_t, actions_t, behaviour)
    vtrace_rows   vtrace(..., value_t=, tail=, rho_t=)              against the torch reverse loop over value and ratio rows
    vtrace_table  vtrace(..., values=, key_t=, actions_t=, behaviour=, target=)
                                                                    against the gathers V[key], P[key, action] of two
                                                                    probability tables, a division and the same loop
    gae_rows, gae_table   gae() on the same rows: the same scan with fewer streams, the yardstick
The torch compositions are asserted to give the kernels' bits before anything is timed.  Each kernel figure is also given as
bytes moved / the box's own copy ceiling (lmaze_bandwidth_probe, 512 MiB copy: read + write bytes per second), the bytes
being the rows read and written once; the table gathers (4 bytes of value and one row of each table per sample, from tables
that stay in L2) are listed beside them and not counted.

    python tools/bench_vtrace.py --out profiles/vtrace/bench_vtrace.json [--rounds 5]"""
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

ROWS = ((64, 65536), (64, 1 << 20))
TABLES = (("ball 11x11", 121), ("goal 11x11", 14641))
FORMS = (("thresholds", "thresholds"), ("policy", "q"))
GAMMA, LAM, RHO_BAR, C_BAR = 0.99, 0.95, 1.0, 1.0
ROW_BYTES = {"thresholds": 16, "q": 16, "policy": 1}


def _timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def _rounds(fns, rounds, reps):
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):         # interleaved
        for k, f in fns.items():
            times[k].append(_timed(f, 1 if k.endswith("_torch") else reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {k: {"us": round(med[k], 3), "spread": [round(min(v), 3), round(max(v), 3)]} for k, v in times.items()}


def copy_ceiling(dev, rounds):
    """bytes per second (read + write) of the library's own copy probe over 512 MiB."""
    nbytes = 512 << 20
    src, dst = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def probe():
        PKG._abi.check("lmaze_bandwidth_probe", PKG._abi.lib.lmaze_bandwidth_probe(src.data_ptr(), dst.data_ptr(), nbytes, stream))
    med, _ = _rounds({"copy": probe}, max(rounds, 5), 1)
    return 2 * nbytes / (med["copy"] * 1e-6)


def _torch_vtrace(reward, done, value, tail, ratio):
    """the T-step reverse loop of elementwise ops, each rounded on its own like the kernel's"""
    T = reward.shape[0]
    vs_t, pg_t = torch.empty_like(reward), torch.empty_like(reward)
    v_next, vs_next, acc = tail, tail, torch.zeros_like(tail)
    for t in range(T - 1, -1, -1):
        r, v, x = reward[t], value[t], ratio[t]
        rho = torch.clamp(x, max=RHO_BAR)
        c = LAM * torch.clamp(x, max=C_BAR)
        acc = torch.where(done[t], rho * (r - v), rho * ((r + GAMMA * v_next) - v) + (GAMMA * c) * acc)
        vs = acc + v
        pg_t[t] = rho * (torch.where(done[t], r, r + GAMMA * vs_next) - v)
        vs_t[t] = vs
        v_next, vs_next = v, vs
    return vs_t, pg_t


def _table(kind, keys, dev, g):
    if kind == "thresholds":
        return PKG.table_policy(probs=torch.rand((keys, 4), device=dev, generator=g) + 0.05)
    if kind == "policy":
        return PKG.table_policy(policy=torch.randint(0, 4, (keys,), dtype=torch.uint8, device=dev, generator=g), epsilon=0.1)
    return PKG.table_policy(q=torch.randn((keys, 4), device=dev, generator=g), epsilon=0.05)


def _prob_table(table, dev):
    """float32[keys, 4]: action_probs() over every (key, action) pair -- what the torch composition gathers from"""
    key = torch.arange(table.keys, dtype=torch.int32, device=dev).repeat_interleave(4).contiguous()
    act = torch.arange(4, dtype=torch.int32, device=dev).repeat(table.keys).contiguous()
    return PKG.action_probs(key, act, table).view(table.keys, 4)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def bench(T, n, name, keys, forms, rounds, reps, ceiling, dev):
    g = torch.Generator(device=dev).manual_seed(n + keys)
    reward = torch.randn((T, n), device=dev, generator=g)
    done = torch.rand((T, n), device=dev, generator=g) < 0.05
    value_t = torch.randn((T, n), device=dev, generator=g)
    rho_t = torch.rand((T, n), device=dev, generator=g) * 2
    tail = torch.randn(n, device=dev, generator=g)
    values = torch.randn(keys, device=dev, generator=g)
    key_t = torch.randint(0, keys, (T, n), dtype=torch.int32, device=dev, generator=g)
    key_tail = torch.randint(0, keys, (n,), dtype=torch.int32, device=dev, generator=g)
    act_t = torch.randint(0, 4, (T, n), dtype=torch.int32, device=dev, generator=g)
    behaviour, target = _table(forms[0], keys, dev, g), _table(forms[1], keys, dev, g)
    pb, pt = _prob_table(behaviour, dev), _prob_table(target, dev)
    vs, pg, adv, tgt, prob = (torch.empty_like(reward) for _ in range(5))
    clips = dict(rho_bar=RHO_BAR, c_bar=C_BAR)

    def torch_table():
        k, a = key_t.long(), act_t.long()
        b = pb[k, a]
        ratio = torch.where(b == 0, torch.zeros_like(b), pt[k, a] / b)
        return _torch_vtrace(reward, done, values[k], values[key_tail.long()], ratio)

    fns = {
        "probs": lambda: PKG.action_probs(key_t, act_t, behaviour, out=prob),
        "vtrace_rows": lambda: PKG.vtrace(reward, done, GAMMA, LAM, value_t=value_t, tail=tail, rho_t=rho_t, out=vs, pg=pg, **clips),
        "vtrace_rows_torch": lambda: _torch_vtrace(reward, done, value_t, tail, rho_t),
        "vtrace_table": lambda: PKG.vtrace(reward, done, GAMMA, LAM, values=values, key_t=key_t, key_tail=key_tail, actions_t=act_t,
                                           behaviour=behaviour, target=target, out=vs, pg=pg, **clips),
        "vtrace_table_torch": torch_table,
        "gae_rows": lambda: PKG.gae(reward, done, GAMMA, LAM, value_t=value_t, tail=tail, out=adv, targets=tgt),
        "gae_table": lambda: PKG.gae(reward, done, GAMMA, LAM, values=values, key_t=key_t, key_tail=key_tail, out=adv, targets=tgt),
    }
    for form in ("rows", "table"):  # the composition gives the kernel's bits
        want = fns["vtrace_%s_torch" % form]()
        fns["vtrace_%s" % form]()
        assert _same(vs, want[0]) and _same(pg, want[1]), "the torch composition and vtrace (%s form) differ" % form
        del want
    med, out = _rounds(fns, rounds, reps)
    m = T * n
    moved = {"probs": 12 * m, "vtrace_rows": 21 * m + 4 * n, "vtrace_table": 21 * m + 4 * n, "gae_rows": 17 * m + 4 * n,
             "gae_table": 17 * m + 4 * n}                                   # rows read + written once
    gathered = {"probs": ROW_BYTES[forms[0]], "vtrace_table": 4 + ROW_BYTES[forms[0]] + ROW_BYTES[forms[1]], "gae_table": 4}
    return {"rows": "%dx%d" % (T, n), "T": T, "n": n, "table": name, "keys": keys, "behaviour": forms[0], "target": forms[1],
            "us_per_call": out, "bytes": moved, "bytes_per_sample": {k: round(b / m, 2) for k, b in moved.items()},
            "gathered_bytes_per_sample": gathered,
            "fraction_of_copy_ceiling": {k: round(b / (med[k] * 1e-6) / ceiling, 3) for k, b in moved.items()},
            "torch_over_kernel": {k: round(med[k + "_torch"] / med[k], 1) for k in ("vtrace_rows", "vtrace_table")},
            "vtrace_over_gae": {"rows": round(med["vtrace_rows"] / med["gae_rows"], 3),
                                "table": round(med["vtrace_table"] / med["gae_table"], 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="kernel calls per timed window (the torch loops are timed one by one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ceiling = copy_ceiling(dev, args.rounds)
    print(json.dumps({"copy_ceiling_TB_per_s": round(ceiling / 1e12, 3)}), flush=True)
    res = []
    for T, n in ROWS:
        for name, keys in TABLES:
            for forms in FORMS:
                r = bench(T, n, name, keys, forms, args.rounds, args.reps, ceiling, dev)
                print(json.dumps(r), flush=True)
                res.append(r)
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "copy_ceiling_bytes_per_s": ceiling, "rounds": args.rounds,
                       "reps": args.reps, "results": res}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
