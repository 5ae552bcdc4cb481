"""One-launch foveal rollout (LmazeFovealVecEnv.rollout -> lmaze_foveal_rollout) against a Python loop of T step launches
(step_raw / hier_step_raw) on the same seeded inputs, interleaved A/B rounds in one process, HIP events after warm-up.

    python tools/bench_foveal_rollout.py --out profiles/foveal_rollout/bench.json [--sizes 4096,16384] [--steps 64,256]

Per line: us per step (median over rounds, and the spread min..max), env-steps/s, the bytes one env-step moves as counted
here -- observation (C*25*4) + action (4) + the trajectory rows + the per-env state once per rollout (state bytes / T) --
and the launch lmaze_describe_foveal_rollout names."""
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

WORKLOADS = (("v1", False), ("v1", True), ("v2", False), ("v2", True), ("v4", False), ("v4", True), ("v5", True))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def bench(variant, fused, n, T, rounds, dev):
    env = PKG.LmazeFovealVecEnv(n, variant=variant, device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(n + T)
    hi = 4 if variant in ("v1", "v5") else 25
    acts = torch.randint(0, hi, (T, n), dtype=torch.int32, device=dev, generator=g)
    goals = torch.randint(0, 25, (T, n), dtype=torch.int32, device=dev, generator=g) if variant == "v5" else None
    two = goals is not None
    stride = n * 4

    def one():
        env.rollout(acts, goals=goals, auto_reset=fused and not two, trajectory=True)

    def loop():
        for t in range(T):
            if two:
                env.hier_step_raw(acts.data_ptr() + t * stride, goals.data_ptr() + t * stride)
            else:
                env.step_raw(acts.data_ptr() + t * stride, auto_reset=fused)

    for _ in range(2):
        one()
        loop()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(_timed(one) / T)
        b.append(_timed(loop) / T)
    C = env.channels
    state = env._state.numel() // n + (4 if env._has_visit else 0)
    rows = 5 * (2 if variant in ("v1", "v5") else 1)
    per = C * 25 * 4 + 4 + (4 if two else 0) + rows + (100 * 4 if two else 0)
    med_a, med_b = statistics.median(a), statistics.median(b)
    return {"variant": variant, "workload": "two-level" if two else ("fused-reset" if fused else "plain"), "n": n, "T": T,
            "one_launch_us_per_step": round(med_a, 3), "one_launch_spread": [round(min(a), 3), round(max(a), 3)],
            "step_loop_us_per_step": round(med_b, 3), "step_loop_spread": [round(min(b), 3), round(max(b), 3)],
            "speedup": round(med_b / med_a, 3), "env_steps_per_s_one_launch": round(n / med_a * 1e6),
            "env_steps_per_s_step_loop": round(n / med_b * 1e6),
            "bytes_per_env_step": round(per + state / T, 1),
            "bytes_counted": "obs %d + action%s + rows %d + state %d / T%s" % (C * 100, " + goal" if two else "", rows, state,
                                                                             " + obs_local 400" if two else ""),
            "launch": PKG._abi.describe_foveal_rollout(env.params, n, T, fused and not two, two)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536,1048576")
    ap.add_argument("--steps", default="64,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl = WORKLOADS if args.workloads == "all" else [w for w in WORKLOADS if "%s%s" % (w[0], "f" if w[1] else "") in args.workloads.split(",")]
    res = []
    for n in [int(x) for x in args.sizes.split(",")]:
        for T in [int(x) for x in args.steps.split(",")]:
            for variant, fused in wl:
                r = bench(variant, fused, n, T, args.rounds, dev)
                print(json.dumps(r), flush=True)
                res.append(r)
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
