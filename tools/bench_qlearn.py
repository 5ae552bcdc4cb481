"""Q-learning inside the one-launch rollout (rollout_qlearn()) against the torch loop it replaces and against its floor, the
acting-only rollout on the same tables; interleaved rounds in one process, HIP events after warm-up.  Per shape (fused reset,
T steps, epsilon 0.1, alpha 0.1, gamma 0.99, the final planes only, trajectory rows):
    (l) rollout_qlearn(T, q[N, G*G, 4], ...)                      one launch: act, step, learn
    (a) T x (gather q[i, cell] + first maximum + torch epsilon mix + step(auto_reset=True) + gather q[i, cell'] + max +
             indexed update)                                       the same learner on the per-step API
    (p) rollout_policy(T, q=q, epsilon, key="env")                 acting only, a table per env: l / p is the cost of learning
        (its greedy_table(q) reduction is part of the call: a user who acts on a Q table pays it)
    (b) rollout_policy(T, policy=greedy bytes, epsilon, key="env") acting only on a byte table reduced beforehand
Each method steps an env of its own (same layouts, same seed) and, where it learns, a table of its own.  Reported per method:
us per step, median over the rounds and the spread; and the ratios a / l, l / p and l / b.

    python tools/bench_qlearn.py --out profiles/qlearn/bench_qlearn.json [--steps 64] [--rounds 5]

Exit status 1 when at 16 384 x 11x11 per-env (l) is not faster than (a): that is the feature's reason to exist."""
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
EPS, ALPHA, GAMMA = 0.1, 0.1, 0.99


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
    envs = {k: _make(variant, G, n, per_env, dev) for k in ("l", "a", "p", "b")}
    S = G * G
    g = torch.Generator(device=dev).manual_seed(n + T)
    q0 = torch.rand((n, S, 4), device=dev, generator=g)
    q_l, q_a, q_p = q0.clone(), q0.clone().reshape(n * S, 4), q0.clone()
    bytes_b = PKG.LmazeVecEnv.greedy_table(q0.reshape(n * S, 4))
    row0 = torch.arange(n, device=dev, dtype=torch.int64) * S

    def rows(env):
        ball = env.ball_xy
        return row0 + (ball[:, 0] * G + ball[:, 1]).long()

    def l():  # noqa: E743
        envs["l"].rollout_qlearn(T, q_l, alpha=ALPHA, gamma=GAMMA, epsilon=EPS)

    def a():
        env = envs["a"]
        for _ in range(T):
            r = rows(env)
            greedy = PKG.LmazeVecEnv.greedy_table(q_a[r]).to(torch.int32)
            explore = torch.rand(n, device=dev) < EPS
            act = torch.where(explore, torch.randint(0, 4, (n,), dtype=torch.int32, device=dev), greedy)
            _, rew, done, _ = env.step(act, auto_reset=True)
            v_next = q_a[rows(env)].max(-1).values
            target = torch.where(done.bool(), rew, rew + GAMMA * v_next)
            al = act.long()
            q_a[r, al] = q_a[r, al] + ALPHA * (target - q_a[r, al])

    def p():
        envs["p"].rollout_policy(T, q=q_p, epsilon=EPS, key="env", trajectory=True)

    def b():
        envs["b"].rollout_policy(T, policy=bytes_b, epsilon=EPS, key="env", trajectory=True)

    fns = {"l": l, "a": a, "p": p, "b": b}
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
    return {"shape": name, "variant": variant, "G": G, "n": n, "per_env_layouts": per_env, "T": T, "epsilon": EPS, "alpha": ALPHA,
            "gamma": GAMMA, "fused_reset": True, "env_steps_per_s": round(n / (med["l"] * 1e-6), 1),
            "launches": {"l": d.describe_env_rollout_qlearn(envs["l"].params, n, T),
                         "p": d.describe_env_rollout(envs["p"].params, n, T, form="policy")},
            "results": out, "a_over_l": round(med["a"] / med["l"], 2), "l_over_p": round(med["l"] / med["p"], 3),
            "l_over_b": round(med["l"] / med["b"], 3)}


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
    if not gate["results"]["l"]["us_per_step"] < gate["results"]["a"]["us_per_step"]:
        print("FAIL: at %s the learner in the rollout (%.3f us per step) is not faster than the per-step loop (%.3f)"
              % (GATE, gate["results"]["l"]["us_per_step"], gate["results"]["a"]["us_per_step"]), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
