"""Rollouts that record observations, against what a caller does without them, interleaved rounds in one process, HIP
events after warm-up.  Per shape:
    (a) rollout(obs_t, obs_every=1)              one launch, every step's observation into the caller's slots
    (b) T x (step() + copy of obs into its slot)  the caller's loop without the feature
    (c) rollout()                                today's one launch, planes rewritten every step
    (d) rollout(obs_every=0)                     grid only: the final planes only

    python tools/bench_rollout_obs.py --out profiles/rollout_obs/bench_rollout_obs.json [--steps 16] [--rounds 5]
    python tools/bench_rollout_obs.py --sweep      (a) and (d) under launch_hint bits 12-14 (envs per workgroup) and 15
                                                   (the other slot store policy), grid shapes

Per line: us per step (median over rounds, and the spread min..max), the bytes one env-step moves as counted here --
action 4 B + rows 5 B (trajectory=True) + per-env state / T, and for (a) / (b) the recorded observation (4 G^2, or
100 C (+400 local)) -- and that rate against the 8 TB/s peak."""
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
PEAK = 8.0e12

GRID = (("v0", 11, 65536, "shared", False), ("v0", 8, 65536, "shared", False), ("v0", 11, 1 << 20, "shared", False),
        ("v0", 11, 1 << 20, "shared", True), ("v0", 11, 16384, "per_env", False), ("v0", 32, 262144, "per_env", False))
FOVEAL = (("v1", 16384), ("v2", 16384), ("v4", 16384), ("v5", 16384), ("v1", 1 << 20), ("v2", 1 << 20), ("v4", 1 << 20),
          ("v5", 1 << 20))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def _run(fns, T, rounds):
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(_timed(f) / T)
    return times


def _line(times, n, per_bytes):
    out = {}
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = {"us_per_step": round(med, 3), "spread": [round(min(v), 3), round(max(v), 3)],
                  "bytes_per_env_step": round(per_bytes[k], 1),
                  "frac_of_8TBs": round(n * per_bytes[k] / (med * 1e-6) / PEAK, 3)}
    return out


def bench_grid(variant, G, n, kind, fused, T, rounds, dev, hints=(0,)):
    if kind == "per_env":
        env = PKG.LmazeVecEnv(n, variant=variant, per_env_layouts=PKG.layouts.random_walled(n, G, dev, seed=1), device=dev)
    else:
        env = PKG.LmazeVecEnv(n, variant=variant, layout=PKG.layouts.open_room(G, (G // 2, G // 2)), device=dev)
    g = torch.Generator(device=dev).manual_seed(n + T)
    acts = torch.randint(0, 4, (T, n), dtype=torch.int32, device=dev, generator=g)
    obs_t = torch.empty((T, n, G, G), dtype=torch.int32, device=dev)
    stride = n * 4
    fns = {}
    for h in hints:
        def a(h=h):
            env.params.launch_hint = h
            env.rollout(acts, auto_reset=fused, trajectory=True, obs_t=obs_t, obs_every=1)
            env.params.launch_hint = 0

        def d(h=h):
            env.params.launch_hint = h
            env.rollout(acts, auto_reset=fused, trajectory=True, obs_every=0)
            env.params.launch_hint = 0
        fns["a" if h == 0 else "a_hint_%#x" % h] = a
        fns["d" if h == 0 else "d_hint_%#x" % h] = d

    if hints == (0,):
        rew_t = torch.empty((T, n), dtype=torch.float32, device=dev)
        done_t = torch.empty((T, n), dtype=torch.bool, device=dev)

        def b():
            for t in range(T):
                env.step_raw(acts.data_ptr() + t * stride, auto_reset=fused)
                obs_t[t].copy_(env.obs)
                rew_t[t].copy_(env.reward)
                done_t[t].copy_(env.done)
        fns["b"] = b
        fns["c"] = lambda: env.rollout(acts, auto_reset=fused, trajectory=True)
    times = _run(fns, T, rounds)
    state = env._state.numel() / n
    base = 4 + 5 + state / T
    per = {k: base + (4 * G * G if k[0] in "ab" else 0) for k in times}
    return {"family": "grid", "variant": variant, "G": G, "n": n, "layout": kind, "fused_reset": fused, "T": T,
            "bytes_counted": "action 4 + rows 5 + state %d / T (+ obs 4 G^2 = %d for a, b)" % (state, 4 * G * G),
            "results": _line(times, n, per)}


def bench_foveal(variant, n, T, rounds, dev):
    env = PKG.LmazeFovealVecEnv(n, variant=variant, device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(n + T)
    two = variant == "v5"
    acts = torch.randint(0, 4 if variant in ("v1", "v5") else 25, (T, n), dtype=torch.int32, device=dev, generator=g)
    goals = torch.randint(0, 25, (T, n), dtype=torch.int32, device=dev, generator=g) if two else None
    fused = not two
    obs_t = torch.empty((T,) + tuple(env.obs.shape), dtype=torch.float32, device=dev)
    loc_t = torch.empty((T,) + tuple(env.obs_local.shape), dtype=torch.float32, device=dev) if two else None
    stride = n * 4

    def a():
        env.rollout(acts, goals=goals, auto_reset=fused, trajectory=True, obs_t=obs_t, obs_local_t=loc_t, obs_every=1)

    rows = [torch.empty((T, n), dtype=x.dtype, device=dev) for x in (env.reward, env.done)]

    def b():
        for t in range(T):
            if two:
                env.hier_step_raw(acts.data_ptr() + t * stride, goals.data_ptr() + t * stride)
                loc_t[t].copy_(env.obs_local)
            else:
                env.step_raw(acts.data_ptr() + t * stride, auto_reset=fused)
            obs_t[t].copy_(env.obs)
            rows[0][t].copy_(env.reward)
            rows[1][t].copy_(env.done)

    def c():
        env.rollout(acts, goals=goals, auto_reset=fused, trajectory=True)

    times = _run({"a": a, "b": b, "c": c}, T, rounds)
    C = env.channels
    state = env._state.numel() / n
    rb = 10 if variant in ("v1", "v5") else 5
    base = 4 + (4 if two else 0) + rb + state / T
    obs = 100 * C + (400 if two else 0)
    per = {k: base + (obs if k in "ab" else 0) for k in times}
    return {"family": "foveal", "variant": variant, "n": n, "workload": "two-level" if two else "fused-reset", "T": T,
            "bytes_counted": "action 4%s + rows %d + state %d / T (+ obs %d for a, b)" % (" + goal 4" if two else "", rb,
                                                                                        state, obs),
            "results": _line(times, n, per)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = []
    if args.sweep:
        hints = (0,) + tuple(k << 12 for k in (2, 3, 4, 5)) + (0x8000,)
        for variant, G, n, kind, fused in GRID:
            if G == 8 and kind == "shared":
                continue                          # the wave-autonomous kernel has no envs-per-workgroup knob
            r = bench_grid(variant, G, n, kind, fused, args.steps, args.rounds, dev, hints=hints)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
    else:
        for variant, G, n, kind, fused in GRID:
            r = bench_grid(variant, G, n, kind, fused, args.steps, args.rounds, dev)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
        for variant, n in FOVEAL:
            r = bench_foveal(variant, n, args.steps, args.rounds, dev)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
