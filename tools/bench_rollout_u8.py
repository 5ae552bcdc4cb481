"""One-launch rollouts of the u8 env against what it did before (T step launches) and against the int32 env, interleaved
rounds in one process, HIP events after warm-up.  Per shape (fused reset, T steps):
    (a) u8 rollout()                                one launch of rollout_shared_u8_kernel
    (b) T x u8 step()                               the u8 env's rollout before the kernel existed
    (c) int32 rollout()                             the int32 env's one launch, same shape
    (d) u8 rollout(obs_t, obs_every=1)              one launch, every step's planes into the caller's uint8 slots
    (e) T x (u8 step() + copy of obs into its slot)  the same without the recording rollout

    python tools/bench_rollout_u8.py --out profiles/rollout_u8/bench_rollout_u8.json [--steps 16] [--rounds 5]
    python tools/bench_rollout_u8.py --sweep --out ...   (a) and (d) under launch_hint bits 12-14 = 3..7 (16..256 envs
                                                         per workgroup), where the launcher's default comes from

Per line: us per step (median over rounds, and the spread min..max), the bytes one env-step moves as counted here --
action 4 B + per-env state / T + the planes (G^2 for the u8 forms, 4 G^2 for (c); (d) and (e) the slot) -- and that
rate against the 8 TB/s peak."""
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

SHAPES = ((8, 65536), (11, 65536), (12, 16384), (11, 262144), (11, 1 << 20))


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


def bench(variant, G, n, T, rounds, dev, hints=None):
    lay = PKG.layouts.open_room(G, (G // 2, G // 2))
    env = PKG.LmazeVecEnv(n, variant=variant, layout=lay, device=dev, obs_dtype="u8")
    g = torch.Generator(device=dev).manual_seed(n + T)
    acts = torch.randint(0, 4, (T, n), dtype=torch.int32, device=dev, generator=g)
    obs_t = torch.empty((T, n, G, G), dtype=torch.uint8, device=dev)
    stride = n * 4
    fns = {}
    if hints:
        for h in hints:
            def a(h=h):
                env.params.launch_hint = h
                env.rollout(acts)
                env.params.launch_hint = 0

            def d(h=h):
                env.params.launch_hint = h
                env.rollout(acts, obs_t=obs_t, obs_every=1)
                env.params.launch_hint = 0
            fns["a_hint_%#x" % h] = a
            fns["d_hint_%#x" % h] = d
        wide = None
    else:
        wide = PKG.LmazeVecEnv(n, variant=variant, layout=lay, device=dev)

        def b():
            for t in range(T):
                env.step_raw(acts.data_ptr() + t * stride, auto_reset=True)

        def e():
            for t in range(T):
                env.step_raw(acts.data_ptr() + t * stride, auto_reset=True)
                obs_t[t].copy_(env.obs)
        fns = {"a": lambda: env.rollout(acts), "b": b, "c": lambda: wide.rollout(acts),
               "d": lambda: env.rollout(acts, obs_t=obs_t, obs_every=1), "e": e}
    times = _run(fns, T, rounds)
    state = env._state.numel() / n
    base = 4 + state / T
    per = {k: base + (4 * G * G if k == "c" else (2 * G * G if k == "e" else G * G)) for k in times}
    out = {}
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = {"us_per_step": round(med, 3), "spread": [round(min(v), 3), round(max(v), 3)],
                  "bytes_per_env_step": round(per[k], 1), "frac_of_8TBs": round(n * per[k] / (med * 1e-6) / PEAK, 3)}
    kern = PKG._abi.describe_rollout(env.params, n, T, auto_reset=True, with_obs="u8")
    del wide
    return {"variant": variant, "G": G, "n": n, "fused_reset": True, "T": T, "u8_rollout_launch": kern,
            "bytes_counted": "action 4 + state %d / T + planes (G^2 u8, 4 G^2 int32; e: the step's G^2 + the copy's G^2)"
                             % state, "results": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variant", default="v0")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hints = tuple(k << 12 for k in (3, 4, 5, 6, 7)) if args.sweep else None
    res = []
    for G, n in SHAPES:
        r = bench(args.variant, G, n, args.steps, args.rounds, dev, hints=hints)
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
