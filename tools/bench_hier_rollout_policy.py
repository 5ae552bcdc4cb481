"""Closed-loop one-launch two-level rollouts of v5/v6 (LmazeFovealVecEnv.rollout_hier_policy: a tabular planner and a tabular
controller inside the kernel) against the loop they replace and against the open-loop rollout, interleaved rounds in one
process, HIP events after warm-up.  Per shape (v5, T steps, trajectory rows on, epsilon = planner epsilon = 0.1):
    (p) rollout_hier_policy(T, controller, planner, ..., trajectory=True)   one launch: per env-step two 1-byte table reads and
                                                                            one Philox draw
    (a) T x (gather planner[state_keys()] + epsilon mix, gather controller[controller_keys()] + epsilon mix,
             hier_step(actions, goals) + row copies)                        the same loop on the per-step API
    (b) rollout(actions, goals=goals, trajectory=True)                      the open-loop rollout over pre-generated int32[T,N] tensors
Each method steps an env of its own (same layouts, same seed).  (a) looks its controller key up BEFORE the plannerStep of
the same launch -- the per-step API has no key in between -- so it is a timing stand-in, not the same policy.  Reported per
method: us per step, median over the rounds and the spread; and the ratios a / p and p / b.

    python tools/bench_hier_rollout_policy.py --out profiles/hier_rollout_policy/bench_hier_rollout_policy.json
        [--steps 64] [--rounds 5] [--keys offset,cell] [--envs 16384,65536,1048576]

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


def bench(ckey, n, T, rounds, dev):
    closed, loop, open_ = (PKG.LmazeFovealVecEnv(n, variant="v5", device=dev, seed=3) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(n + T)
    cells = closed.n_layouts * closed.grid * closed.grid
    controller = torch.randint(0, 4, (100 * cells if ckey == "cell" else 100,), dtype=torch.uint8, device=dev, generator=g)
    planner = torch.randint(0, 25, (cells,), dtype=torch.uint8, device=dev, generator=g)
    actions = torch.randint(0, 4, (T, n), dtype=torch.int32, device=dev, generator=g)
    goals = torch.randint(0, 25, (T, n), dtype=torch.int32, device=dev, generator=g)
    rows = [torch.empty((T, n), dtype=dt, device=dev) for _ in range(2) for dt in (torch.float32, torch.bool)]
    ints = [torch.empty((T, n), dtype=torch.int32, device=dev) for _ in range(4)]
    act_t, key_t, goals_t, goal_key_t = ints

    def p():
        closed.rollout_hier_policy(T, controller=controller, planner=planner, epsilon=EPS, planner_epsilon=EPS, controller_key=ckey,
                                   trajectory=True, actions_t=act_t, key_t=key_t, goals_t=goals_t, goal_key_t=goal_key_t)

    def a():
        for t in range(T):
            kp = loop.state_keys()
            goal = planner[kp.long()].to(torch.int32)
            goal = torch.where(torch.rand(n, device=dev) < EPS, torch.randint(0, 25, (n,), dtype=torch.int32, device=dev), goal)
            kc = loop.controller_keys(ckey)
            act = controller[kc.long()].to(torch.int32)
            act = torch.where(torch.rand(n, device=dev) < EPS, torch.randint(0, 4, (n,), dtype=torch.int32, device=dev), act)
            loop.hier_step(act, goal)
            for r, src in zip(ints, (act, kc, goal, kp)):
                r[t].copy_(src)
            for r, src in zip(rows, (loop.reward, loop.done, loop.foveal_reward, loop.foveal_done)):
                r[t].copy_(src)

    def b():
        open_.rollout(actions, goals=goals, trajectory=True)

    med, out = _rounds({"p": p, "a": a, "b": b}, rounds, T)
    return {"variant": "v5", "G": closed.grid, "layouts": closed.n_layouts, "n": n, "T": T, "controller_key": ckey, "epsilon": EPS,
            "planner_epsilon": EPS, "env_steps_per_s": round(n / (med["p"] * 1e-6), 1),
            "closed_loop_launch": PKG._abi.describe_v5_rollout_policy(closed.params, n, T, ckey, 0),
            "open_loop_launch": PKG._abi.describe_foveal_rollout(open_.params, n, T, auto_reset=True, two_level=True),
            "us_per_step": out, "a_over_p": round(med["a"] / med["p"], 2), "p_over_b": round(med["p"] / med["b"], 3)}


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
    slow = [r for r in res if not r["us_per_step"]["p"]["us"] < r["us_per_step"]["a"]["us"]]
    for r in slow:
        print("FAIL: %s x %d: the closed loop (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (r["controller_key"], r["n"], r["us_per_step"]["p"]["us"], r["us_per_step"]["a"]["us"]), file=sys.stderr)
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
