"""Closed-loop one-launch rollouts with a table PER ENV (rollout_policy(key="env") / rollout_sample(key="env")) against
what a user writes without them and against their floor, the same rollout with ONE table for the batch; interleaved rounds
in one process, HIP events after warm-up.  Per shape (fused reset, T steps, epsilon 0.1, the final planes only, trajectory
rows), for the epsilon-greedy form:
    (e) rollout_policy(T, policy[N, G*G], epsilon, key="env")   one launch
    (a) T x (torch gather of policy[i, ball_x * G + ball_y] + torch epsilon mix + step(auto_reset=True))
                                                                 the same loop on the per-step API: three or more launches
                                                                 a step, and step() renders the planes every step
    (p) rollout_policy(T, policy[G*G], epsilon, key="ball")     one shared table on the same env: the floor -- e / p is what
                                                                 a table per env costs over a table per batch
and for the sampling form the same three, "s_e", "s_a" (gather of probs[i, cell] + torch.multinomial + step()) and "s_p".
Each method steps an env of its own (same layouts, same seed).  Reported per method: us per step, median over the rounds
and the spread; and the ratios a / e and e / p of both forms.

    python tools/bench_rollout_env_table.py --out profiles/rollout_env_table/bench_rollout_env_table.json [--steps 64] [--rounds 5]

Exit status 1 when at 16 384 x 11x11 per-env (e) is not faster than (a): that is the feature's reason to exist."""
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

# (name, G, envs, per-env layouts)
SHAPES = (("16384x11x11 per-env", 11, 16384, True), ("65536x11x11 per-env", 11, 65536, True),
          ("16384x32x32 per-env", 32, 16384, True), ("65536x11x11 shared", 11, 65536, False))
GATE = "16384x11x11 per-env"
EPS = 0.1


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def _make(variant, G, n, per_env, dev):
    if per_env:
        lays = PKG.layouts.random_walled(n, G, dev, seed=7 + G)
        return PKG.LmazeVecEnv(n, variant=variant, per_env_layouts=lays, device=dev, seed=3)
    return PKG.LmazeVecEnv(n, variant=variant, layout=PKG.layouts.open_room(G, (G // 2, G // 2)), device=dev, seed=3)


def bench(variant, name, G, n, per_env, T, rounds, dev):
    envs = {k: _make(variant, G, n, per_env, dev) for k in ("e", "a", "p", "s_e", "s_a", "s_p")}
    S = G * G
    g = torch.Generator(device=dev).manual_seed(n + T)
    tables = torch.randint(0, 4, (n, S), dtype=torch.uint8, device=dev, generator=g)
    tables_i32 = tables.reshape(-1).to(torch.int32)
    probs = torch.rand((n, S, 4), device=dev, generator=g) + 0.05
    thresholds = PKG._abi.sampling_thresholds(probs.reshape(-1, 4))
    one_table, one_thresholds = tables[0].contiguous(), thresholds.view(torch.int32)[:S].clone()     # int32: the same bits
    row0 = torch.arange(n, device=dev, dtype=torch.int64) * S

    def rows(env):
        ball = env.ball_xy
        return row0 + (ball[:, 0] * G + ball[:, 1]).long()

    def e():
        envs["e"].rollout_policy(T, policy=tables, epsilon=EPS, key="env", trajectory=True)

    def a():
        env = envs["a"]
        for _ in range(T):
            greedy = tables_i32[rows(env)]
            explore = torch.rand(n, device=dev) < EPS
            env.step(torch.where(explore, torch.randint(0, 4, (n,), dtype=torch.int32, device=dev), greedy), auto_reset=True)

    def p():
        envs["p"].rollout_policy(T, policy=one_table, epsilon=EPS, key="ball", trajectory=True)

    def s_e():
        envs["s_e"].rollout_sample(T, thresholds=thresholds, key="env", trajectory=True)

    def s_a():
        env = envs["s_a"]
        flat = probs.reshape(-1, 4)
        for _ in range(T):
            env.step(torch.multinomial(flat[rows(env)], 1).reshape(n).to(torch.int32), auto_reset=True)

    def s_p():
        envs["s_p"].rollout_sample(T, thresholds=one_thresholds, key="ball", trajectory=True)

    fns = {"e": e, "a": a, "p": p, "s_e": s_e, "s_a": s_a, "s_p": s_p}
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):         # interleaved
        for k, f in fns.items():
            times[k].append(_timed(f) / T)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {k: {"us_per_step": round(med[k], 3), "spread": [round(min(v), 3), round(max(v), 3)]} for k, v in times.items()}
    d = PKG._abi
    return {"shape": name, "variant": variant, "G": G, "n": n, "per_env_layouts": per_env, "T": T, "epsilon": EPS, "fused_reset": True,
            "env_steps_per_s": round(n / (med["e"] * 1e-6), 1),
            "launches": {"e": d.describe_env_rollout(envs["e"].params, n, T, form="policy"),
                         "p": d.describe_rollout_policy(envs["p"].params, n, T),
                         "s_e": d.describe_env_rollout(envs["s_e"].params, n, T, form="sample"),
                         "s_p": d.describe_rollout_sample(envs["s_p"].params, n, T)},
            "results": out, "a_over_e": round(med["a"] / med["e"], 2), "e_over_p": round(med["e"] / med["p"], 3),
            "sample_a_over_e": round(med["s_a"] / med["s_e"], 2), "sample_e_over_p": round(med["s_e"] / med["s_p"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variant", default="v0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = []
    for name, G, n, per_env in SHAPES:
        r = bench(args.variant, name, G, n, per_env, args.steps, args.rounds, dev)
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)
    gate = next(r for r in res if r["shape"] == GATE)
    if not gate["results"]["e"]["us_per_step"] < gate["results"]["a"]["us_per_step"]:
        print("FAIL: at %s the closed loop (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (GATE, gate["results"]["e"]["us_per_step"], gate["results"]["a"]["us_per_step"]), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
