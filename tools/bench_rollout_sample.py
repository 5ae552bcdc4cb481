"""Sampling closed-loop one-launch rollouts (rollout_sample: a categorical table policy inside the kernel) against what a
user writes without them and against the nearest existing kernel, interleaved rounds in one process, HIP events after
warm-up.  Per shape (fused reset, T steps, the final planes only, trajectory rows on):
    (s) rollout_sample(T, thresholds=...)               one launch: per env-step a 16-byte table read, a Philox draw, three compares
    (a) T x (gather probs[key] + torch.multinomial + step(auto_reset=True))
                                                         the same loop on the per-step API: several launches a step; step()
                                                         renders the planes every step, as that loop does by default
    (e) rollout_policy(T, policy, epsilon=0.1)          the epsilon-greedy closed loop: a 1-byte table read and the same draw
Each method steps an env of its own (same layout, same seed).  Reported per method: us per step, median over the rounds and
the spread; and the ratios a / s and s / e.  32x32 is the largest table staged in LDS (16 KiB), 64x64 reads it from global
memory, and so does the goal-keyed v3 shape.

Then lmaze_returns: discounted_returns(reward_t, done_t, gamma) on [T, N] rows against the torch reverse loop (T dependent
steps of a few launches each), us per call.

    python tools/bench_rollout_sample.py --out profiles/rollout_sample/bench_rollout_sample.json [--steps 64] [--rounds 5]

Exit status 1 when at 65 536 x 11x11 the sampling rollout is not faster than (a): that is the feature's reason to exist."""
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

# (name, variant, key, G, envs, per-env layouts, obs dtype)
SHAPES = (("65536x11x11", "v0", "ball", 11, 65536, False, "int32"), ("1Mx11x11", "v0", "ball", 11, 1 << 20, False, "int32"),
          ("16384x12x12", "v0", "ball", 12, 16384, False, "int32"), ("16384x11x11 per-env", "v0", "ball", 11, 16384, True, "int32"),
          ("65536x11x11 u8", "v0", "ball", 11, 65536, False, "u8"), ("65536x32x32", "v0", "ball", 32, 65536, False, "int32"),
          ("16384x64x64", "v0", "ball", 64, 16384, False, "int32"), ("65536x11x11 v3 goal-keyed", "v3", "goal", 11, 65536, False, "int32"))
RETURNS = ((64, 65536), (64, 1 << 20))
GATE = "65536x11x11"
EPS, GAMMA = 0.1, 0.99


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


def bench(name, variant, key, G, n, per_env, dtype, T, rounds, dev):
    sample, loop, greedy = (_make(variant, G, n, per_env, dtype, dev) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(n + T)
    S = G ** 4 if key == "goal" else G * G
    probs = torch.rand((S, 4), device=dev, generator=g) + 0.05
    probs /= probs.sum(dim=1, keepdim=True)
    thresholds = PKG._abi.sampling_thresholds(probs)
    table = torch.randint(0, 4, (S,), dtype=torch.uint8, device=dev, generator=g)

    def s():
        sample.rollout_sample(T, thresholds=thresholds, key=key, trajectory=True)

    def a():
        for _ in range(T):
            ball = loop.ball_xy
            k = ball[:, 0] * G + ball[:, 1]
            if key == "goal":
                k = (loop.goal_xy[:, 0] * G + loop.goal_xy[:, 1]) * (G * G) + k
            act = torch.multinomial(probs[k.long()], 1).reshape(-1).to(torch.int32)
            loop.step(act, auto_reset=True)

    def e():
        greedy.rollout_policy(T, policy=table, epsilon=EPS, key=key, trajectory=True)

    med, out = _rounds({"s": s, "a": a, "e": e}, rounds, T)
    with_obs = "u8" if dtype == "u8" else True
    return {"shape": name, "variant": variant, "key": key, "G": G, "n": n, "per_env_layouts": per_env, "obs": dtype, "T": T,
            "fused_reset": True, "env_steps_per_s": round(n / (med["s"] * 1e-6), 1),
            "sampling_launch": PKG._abi.describe_rollout_sample(sample.params, n, T, with_obs=with_obs, key=key),
            "eps_greedy_launch": PKG._abi.describe_rollout_policy(greedy.params, n, T, with_obs=with_obs, key=key),
            "us_per_step": out, "a_over_s": round(med["a"] / med["s"], 2), "s_over_e": round(med["s"] / med["e"], 3)}


def bench_returns(T, n, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    reward = torch.randn((T, n), device=dev, generator=g)
    done = torch.rand((T, n), device=dev, generator=g) < 0.05
    out = torch.empty_like(reward)

    def kernel():
        PKG.discounted_returns(reward, done, GAMMA, out=out)

    def torch_loop():
        ret = torch.zeros(n, device=dev)
        res = torch.empty_like(reward)
        for t in range(T - 1, -1, -1):
            ret = torch.where(done[t], reward[t], reward[t] + GAMMA * ret)
            res[t] = ret

    med, res = _rounds({"kernel": kernel, "torch_loop": torch_loop}, rounds, 1)
    return {"returns": "%dx%d" % (T, n), "T": T, "n": n, "gamma": GAMMA, "us_per_call": res,
            "bytes": 13 * T * n, "kernel_TB_per_s": round(13 * T * n / (med["kernel"] * 1e-6) / 1e12, 3),
            "loop_over_kernel": round(med["torch_loop"] / med["kernel"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res, ret = [], []
    for shape in SHAPES:
        r = bench(*shape, args.steps, args.rounds, dev)
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    for T, n in RETURNS:
        r = bench_returns(T, n, args.rounds, dev)
        print(json.dumps(r), flush=True)
        ret.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res, "returns": ret}, f, indent=1)
    gate = next(r for r in res if r["shape"] == GATE)
    if not gate["us_per_step"]["s"]["us"] < gate["us_per_step"]["a"]["us"]:
        print("FAIL: at %s the sampling rollout (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (GATE, gate["us_per_step"]["s"]["us"], gate["us_per_step"]["a"]["us"]), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
