"""Closed-loop one-launch foveal rollouts (LmazeFovealVecEnv.rollout_policy: a tabular epsilon-greedy policy inside the
kernel) against the loop they replace and against the open-loop rollout, interleaved rounds in one process, HIP events after
warm-up.  Per shape (v1 / v2 / v4, fused reset, T steps, trajectory rows on, epsilon = 0.1):
    (p) rollout_policy(T, policy, epsilon=0.1, trajectory=True)   one launch: per env-step a 1-byte table read and a Philox draw
    (a) T x (gather policy[key] + epsilon mix + step(auto_reset=True) + row copies)
                                                                  the same loop on the per-step API: several launches a step
    (b) rollout(actions, auto_reset=True, trajectory=True)        the open-loop rollout over a pre-generated int32[T,N] tensor
Each method steps an env of its own (same layouts, same seed).  Reported per method: us per step, median over the rounds and
the spread; and the ratios a / p and p / b.

    python tools/bench_foveal_rollout_policy.py --out profiles/foveal_rollout_policy/bench_foveal_rollout_policy.json
        [--steps 64] [--rounds 5] [--variants v1,v2,v4] [--envs 16384,65536,1048576]

Exit status 1 when at some shape the closed loop is not faster than (a): that is the feature's reason to exist."""
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
    closed, loop, open_ = (PKG.LmazeFovealVecEnv(n, variant=variant, device=dev, seed=3) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(n + T)
    A = 4 if variant == "v1" else 25
    S = closed.n_layouts * closed.grid * closed.grid
    table = torch.randint(0, A, (S,), dtype=torch.uint8, device=dev, generator=g)
    actions = torch.randint(0, A, (T, n), dtype=torch.int32, device=dev, generator=g)
    streams = 2 if variant == "v1" else 1
    rows = [torch.empty((T, n), dtype=dt, device=dev) for _ in range(streams) for dt in (torch.float32, torch.bool)]
    act_t = torch.empty((T, n), dtype=torch.int32, device=dev)
    key_t = torch.empty((T, n), dtype=torch.int32, device=dev)

    def p():
        closed.rollout_policy(T, policy=table, epsilon=EPS, auto_reset=True, trajectory=True, actions_t=act_t, key_t=key_t)

    def a():
        for t in range(T):
            k = loop.state_keys()
            act = table[k.long()].to(torch.int32)
            explore = torch.rand(n, device=dev) < EPS
            act = torch.where(explore, torch.randint(0, A, (n,), dtype=torch.int32, device=dev), act)
            loop.step(act, auto_reset=True)
            act_t[t].copy_(act)
            key_t[t].copy_(k)
            for r, src in zip(rows, (loop.reward, loop.done, loop.foveal_reward, loop.foveal_done)):
                r[t].copy_(src)

    def b():
        open_.rollout(actions, auto_reset=True, trajectory=True)

    med, out = _rounds({"p": p, "a": a, "b": b}, rounds, T)
    return {"variant": variant, "G": closed.grid, "layouts": closed.n_layouts, "n": n, "T": T, "epsilon": EPS, "fused_reset": True,
            "env_steps_per_s": round(n / (med["p"] * 1e-6), 1),
            "closed_loop_launch": PKG._abi.describe_foveal_rollout_policy(closed.params, n, T, True, 0),
            "open_loop_launch": PKG._abi.describe_foveal_rollout(open_.params, n, T, auto_reset=True),
            "us_per_step": out, "a_over_p": round(med["a"] / med["p"], 2), "p_over_b": round(med["p"] / med["b"], 3)}


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
    slow = [r for r in res if not r["us_per_step"]["p"]["us"] < r["us_per_step"]["a"]["us"]]
    for r in slow:
        print("FAIL: %s x %d: the closed loop (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (r["variant"], r["n"], r["us_per_step"]["p"]["us"], r["us_per_step"]["a"]["us"]), file=sys.stderr)
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
