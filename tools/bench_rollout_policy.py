"""Closed-loop one-launch rollouts (rollout_policy: a tabular epsilon-greedy policy inside the kernel) against what a user
writes without them and against the open-loop ceiling, interleaved rounds in one process, HIP events after warm-up.
Per shape (fused reset, T steps, epsilon 0.1, the final planes only):
    (p) rollout_policy(T, policy, epsilon)              one launch, with the trajectory rows (reward, done, action, key)
    (a) T x (torch gather of policy[ball_x * G + ball_y] + torch epsilon mix + step(auto_reset=True))
                                                         the same loop on the per-step API: three or more launches a step;
                                                         step() renders the planes every step, as that loop does by default, so
                                                         a / p is launches AND dead plane stores saved, not launch overhead alone
    (b) rollout(actions, obs_every=0, trajectory=True)  the open-loop one-launch rollout over pre-generated actions: the
                                                         ceiling -- (p) drops its 4-byte action load and adds a table lookup
                                                         and a Philox draw
Each method steps an env of its own (same layout, same seed).  Reported per method: us per step, median over the rounds and
the spread; and the ratios a / p and p / b.  The 8x8 shape is the one where (b) runs the wave-autonomous kernel and (p),
which has no such form, the general shared one.

    python tools/bench_rollout_policy.py --out profiles/rollout_policy/bench_rollout_policy.json [--steps 64] [--rounds 5]

Exit status 1 when at 65 536 x 11x11 the closed loop is not faster than (a): that is the feature's reason to exist."""
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

# (name, G, envs, per-env layouts, obs dtype)
SHAPES = (("65536x11x11", 11, 65536, False, "int32"), ("1Mx11x11", 11, 1 << 20, False, "int32"),
          ("16384x12x12", 12, 16384, False, "int32"), ("16384x11x11 per-env", 11, 16384, True, "int32"),
          ("65536x11x11 u8", 11, 65536, False, "u8"), ("65536x8x8", 8, 65536, False, "int32"))
GATE = "65536x11x11"
EPS = 0.1


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def _make(variant, G, n, per_env, dtype, dev):
    if per_env:
        lays = PKG.layouts.random_walled(n, G, dev, seed=7 + G)
        return PKG.LmazeVecEnv(n, variant=variant, per_env_layouts=lays, device=dev, seed=3)
    return PKG.LmazeVecEnv(n, variant=variant, layout=PKG.layouts.open_room(G, (G // 2, G // 2)), device=dev, seed=3, obs_dtype=dtype)


def bench(variant, name, G, n, per_env, dtype, T, rounds, dev):
    closed, loop, open_ = (_make(variant, G, n, per_env, dtype, dev) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(n + T)
    table = torch.randint(0, 4, (G * G,), dtype=torch.uint8, device=dev, generator=g)
    table_i32 = table.to(torch.int32)
    acts = torch.randint(0, 4, (T, n), dtype=torch.int32, device=dev, generator=g)

    def p():
        closed.rollout_policy(T, policy=table, epsilon=EPS, trajectory=True)

    def a():
        for _ in range(T):
            ball = loop.ball_xy
            greedy = table_i32[(ball[:, 0] * G + ball[:, 1]).long()]
            explore = torch.rand(n, device=dev) < EPS
            loop.step(torch.where(explore, torch.randint(0, 4, (n,), dtype=torch.int32, device=dev), greedy), auto_reset=True)

    def b():
        open_.rollout(acts, obs_every=0, trajectory=True)

    fns = {"p": p, "a": a, "b": b}
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):         # interleaved
        for k, f in fns.items():
            times[k].append(_timed(f) / T)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {k: {"us_per_step": round(med[k], 3), "spread": [round(min(v), 3), round(max(v), 3)]} for k, v in times.items()}
    return {"shape": name, "variant": variant, "G": G, "n": n, "per_env_layouts": per_env, "obs": dtype, "T": T, "epsilon": EPS,
            "fused_reset": True, "env_steps_per_s": round(n / (med["p"] * 1e-6), 1),
            "closed_loop_launch": PKG._abi.describe_rollout_policy(closed.params, n, T, with_obs="u8" if dtype == "u8" else True),
            "open_loop_launch": PKG._abi.describe_rollout(open_.params, n, T, auto_reset=True,
                                                          with_obs="u8" if dtype == "u8" else True, obs_every=0),
            "results": out, "a_over_p": round(med["a"] / med["p"], 2), "p_over_b": round(med["p"] / med["b"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variant", default="v0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = []
    for name, G, n, per_env, dtype in SHAPES:
        r = bench(args.variant, name, G, n, per_env, dtype, args.steps, args.rounds, dev)
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)
    gate = next(r for r in res if r["shape"] == GATE)
    if not gate["results"]["p"]["us_per_step"] < gate["results"]["a"]["us_per_step"]:
        print("FAIL: at %s the closed loop (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (GATE, gate["results"]["p"]["us_per_step"], gate["results"]["a"]["us_per_step"]), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
