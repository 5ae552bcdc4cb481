"""Sampling closed-loop one-launch foveal rollouts (LmazeFovealVecEnv.rollout_sample: a categorical table policy inside the
kernel) against the loop they replace and against the epsilon-greedy closed loop, interleaved rounds in one process, HIP
events after warm-up.  Per shape (v1 / v2 / v4, fused reset, T steps, trajectory rows on):
    (s) rollout_sample(T, thresholds, trajectory=True)            one launch: per env-step the key's row of thresholds (16 B
                                                                  for v1; 96 B, six reads, for v2/v4) and a Philox draw
    (a) T x (gather thresholds[key] + compare a draw + step(auto_reset=True) + row copies)
                                                                  the same loop on the per-step API: several launches a step
    (p) rollout_policy(T, policy, epsilon=0.1, trajectory=True)   the epsilon-greedy closed loop on the same envs: a 1-byte read
Each method steps an env of its own (same layouts, same seed).  Reported per method: us per step, median over the rounds and
the spread; and the ratios a / s and s / p.

    python tools/bench_foveal_rollout_sample.py --out profiles/foveal_rollout_sample/bench_foveal_rollout_sample.json
        [--steps 64] [--rounds 5] [--variants v1,v2,v4] [--envs 16384,65536,1048576]

Exit status 1 when at some shape the sampling rollout is not faster than (a): that is the feature's reason to exist."""
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

EPS = 0.1


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def _rounds(fns, rounds, per):
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):         # interleaved
        for k, f in fns.items():
            times[k].append(_timed(f) / per)
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {k: {"us": round(med[k], 3), "spread": [round(min(v), 3), round(max(v), 3)]} for k, v in times.items()}


def bench(variant, n, T, rounds, dev):
    sample, loop, greedy = (PKG.LmazeFovealVecEnv(n, variant=variant, device=dev, seed=3) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(n + T)
    A = 4 if variant == "v1" else 25
    S = sample.n_layouts * sample.grid * sample.grid
    thresholds = PKG._abi.sampling_thresholds(torch.rand((S, A), device=dev, generator=g) ** 4, actions=A)
    # the torch loop compares as int64: uint32 has no ordering kernels
    cut = thresholds.view(torch.int32)[:, :A - 1].to(torch.int64) & 0xFFFFFFFF
    table = torch.randint(0, A, (S,), dtype=torch.uint8, device=dev, generator=g)
    streams = 2 if variant == "v1" else 1
    rows = [torch.empty((T, n), dtype=dt, device=dev) for _ in range(streams) for dt in (torch.float32, torch.bool)]
    act_t = torch.empty((T, n), dtype=torch.int32, device=dev)
    key_t = torch.empty((T, n), dtype=torch.int32, device=dev)

    def s():
        sample.rollout_sample(T, thresholds=thresholds, auto_reset=True, trajectory=True, actions_t=act_t, key_t=key_t)

    def a():
        for t in range(T):
            k = loop.state_keys()
            r = torch.randint(0, 1 << 32, (n, 1), dtype=torch.int64, device=dev)
            act = (r >= cut[k.long()]).sum(dim=1).to(torch.int32)
            loop.step(act, auto_reset=True)
            act_t[t].copy_(act)
            key_t[t].copy_(k)
            for row, src in zip(rows, (loop.reward, loop.done, loop.foveal_reward, loop.foveal_done)):
                row[t].copy_(src)

    def p():
        greedy.rollout_policy(T, policy=table, epsilon=EPS, auto_reset=True, trajectory=True, actions_t=act_t, key_t=key_t)

    med, out = _rounds({"s": s, "a": a, "p": p}, rounds, T)
    return {"variant": variant, "G": sample.grid, "layouts": sample.n_layouts, "n": n, "T": T, "fused_reset": True,
            "table_bytes": int(thresholds.numel() * 4), "env_steps_per_s": round(n / (med["s"] * 1e-6), 1),
            "sample_launch": PKG._abi.describe_foveal_rollout_sample(sample.params, n, T, True, 0),
            "policy_launch": PKG._abi.describe_foveal_rollout_policy(greedy.params, n, T, True, 0),
            "us_per_step": out, "a_over_s": round(med["a"] / med["s"], 2), "s_over_p": round(med["s"] / med["p"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="v1,v2,v4")
    ap.add_argument("--envs", default="16384,65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = []
    for variant in args.variants.split(","):
        for n in (int(x) for x in args.envs.split(",")):
            r = bench(variant, n, args.steps, args.rounds, dev)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)
    slow = [r for r in res if not r["us_per_step"]["s"]["us"] < r["us_per_step"]["a"]["us"]]
    for r in slow:
        print("FAIL: %s x %d: the sampling rollout (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (r["variant"], r["n"], r["us_per_step"]["s"]["us"], r["us_per_step"]["a"]["us"]), file=sys.stderr)
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
