"""Sampling closed-loop one-launch two-level rollouts of v5/v6 (LmazeFovealVecEnv.rollout_hier_sample: a categorical planner and
a categorical controller inside the kernel) against the loop they replace and against the epsilon-greedy closed loop,
interleaved rounds in one process, HIP events after warm-up.  Per shape (v5, T steps, trajectory rows on):
    (s) rollout_hier_sample(T, controller_thresholds, planner_thresholds, ..., trajectory=True)
                                                     one launch: per env-step one 16-byte controller row, one Philox draw and,
                                                     for the envs that plan, six 16-byte reads of the planner row
    (a) T x (gather planner rows [state_keys()] + compare-sum on a torch-drawn uniform, gather controller rows
             [controller_keys()] + compare-sum, hier_step(actions, goals) + row copies)    the same loop on the per-step API
    (p) rollout_hier_policy(T, controller, planner, epsilon = planner_epsilon = 0.1, ..., trajectory=True)
                                                     the epsilon-greedy closed loop: two 1-byte table reads per env-step
Each method steps an env of its own (same layouts, same seed).  (a) looks its controller key up BEFORE the plannerStep of
the same launch -- the per-step API has no key in between -- and compares every env's planner row, planning or not, as a
batched loop does: a timing stand-in, not the same policy.  Its tables are the thresholds with the top bit flipped, int32, so
that torch's signed compare is the unsigned one.  Reported per method: us per step, median over the rounds and the spread;
and the ratios a / s and s / p.  No ratio is required: the exit status is 0 whenever the run completes.

    python tools/bench_hier_rollout_sample.py --out profiles/hier_rollout_sample/bench_hier_rollout_sample.json
        [--steps 64] [--rounds 5] [--keys offset,cell] [--envs 16384,65536,1048576]"""
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


def bench(ckey, n, T, rounds, dev):
    sampled, loop, greedy = (PKG.LmazeFovealVecEnv(n, variant="v5", device=dev, seed=3) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(n + T)
    cells = sampled.n_layouts * sampled.grid * sampled.grid
    ckeys = 100 * cells if ckey == "cell" else 100
    # Boltzmann tables at temperature 0.5 over random values
    cth = PKG._abi.sampling_thresholds(torch.softmax(torch.randn(ckeys, 4, device=dev, generator=g).double() / 0.5, -1), actions=4)
    pth = PKG._abi.sampling_thresholds(torch.softmax(torch.randn(cells, 25, device=dev, generator=g).double() / 0.5, -1), actions=25)
    flip = torch.tensor(-2 ** 31, dtype=torch.int32, device=dev)
    cth_s, pth_s = cth.view(torch.int32)[:, :3] ^ flip, pth.view(torch.int32) ^ flip      # signed order = unsigned order
    controller = torch.randint(0, 4, (ckeys,), dtype=torch.uint8, device=dev, generator=g)
    planner = torch.randint(0, 25, (cells,), dtype=torch.uint8, device=dev, generator=g)
    rows = [torch.empty((T, n), dtype=dt, device=dev) for _ in range(2) for dt in (torch.float32, torch.bool)]
    ints = [torch.empty((T, n), dtype=torch.int32, device=dev) for _ in range(4)]
    act_t, key_t, goals_t, goal_key_t = ints

    def s():
        sampled.rollout_hier_sample(T, controller_thresholds=cth, planner_thresholds=pth, controller_key=ckey, trajectory=True,
                                    actions_t=act_t, key_t=key_t, goals_t=goals_t, goal_key_t=goal_key_t)

    def a():
        for t in range(T):
            kp = loop.state_keys()
            r = torch.randint(-2 ** 31, 2 ** 31, (n, 1), dtype=torch.int32, device=dev)
            goal = (r >= pth_s[kp.long()]).sum(dim=1, dtype=torch.int32)
            kc = loop.controller_keys(ckey)
            r = torch.randint(-2 ** 31, 2 ** 31, (n, 1), dtype=torch.int32, device=dev)
            act = (r >= cth_s[kc.long()]).sum(dim=1, dtype=torch.int32)
            loop.hier_step(act, goal)
            for dst, src in zip(ints, (act, kc, goal, kp)):
                dst[t].copy_(src)
            for dst, src in zip(rows, (loop.reward, loop.done, loop.foveal_reward, loop.foveal_done)):
                dst[t].copy_(src)

    def p():
        greedy.rollout_hier_policy(T, controller=controller, planner=planner, epsilon=EPS, planner_epsilon=EPS, controller_key=ckey,
                                   trajectory=True, actions_t=act_t, key_t=key_t, goals_t=goals_t, goal_key_t=goal_key_t)

    med, out = _rounds({"s": s, "a": a, "p": p}, rounds, T)
    return {"variant": "v5", "G": sampled.grid, "layouts": sampled.n_layouts, "n": n, "T": T, "controller_key": ckey,
            "greedy_epsilon": EPS, "greedy_planner_epsilon": EPS, "env_steps_per_s": round(n / (med["s"] * 1e-6), 1),
            "sampled_launch": PKG._abi.describe_v5_rollout_sample(sampled.params, n, T, ckey, 0),
            "greedy_launch": PKG._abi.describe_v5_rollout_policy(greedy.params, n, T, ckey, 0),
            "us_per_step": out, "a_over_s": round(med["a"] / med["s"], 2), "s_over_p": round(med["s"] / med["p"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--keys", default="offset,cell")
    ap.add_argument("--envs", default="16384,65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = []
    for ckey in args.keys.split(","):
        for n in (int(x) for x in args.envs.split(",")):
            r = bench(ckey, n, args.steps, args.rounds, dev)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
