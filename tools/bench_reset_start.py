"""reset(thresholds=...) (lmaze_reset_start: the ball from a start law, one placement launch and the masked render) against
    a  reset() as it is, at the same shape: the floor -- the same bookkeeping and render, no table;
    b  the torch composition it replaces: gather the row, torch.searchsorted on the draw, set_state, zero the counters,
       observe() -- given the SAME 31-bit draws u as a tensor (a sampler of its own would pay for its draw as well), the table
       already widened to int64 outside the timed region (searchsorted has no uint32), and checked here: it must place every
       ball on the cell the kernel chose or the tool exits 1;
    c  the placement launch alone (the ABI call without planes), for the bytes it must read;
alternating within one process, HIP events around each call after warm-up, medians of --rounds calls each (21).
    1  65 536 x 11x11     shared layout, key="ball"      2  1 048 576 x 11x11  shared layout, key="ball"
    3  16 384 x 32x32     per-env layouts, key="env"     4  65 536 x 11x11     per-env layouts, key="env"
    5  65 536 x V3_GRID_18 shared, key="goal", keep_goal=True (both sides read the goals as they are)

    python tools/bench_reset_start.py --out profiles/reset_start/bench_reset_start.json [--rounds 21]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = importlib.import_module("gym-lmaze_amd")
from bench_solve import _rounds   # noqa: E402  (the same timing loop)

HBM_PEAK = 8.0e12                  # bytes per second, the MI355X's nominal figure
M32 = np.uint64(0xFFFFFFFF)


def reset_draw_u(seed, epoch, n, env_base=0):
    """u int64[n] = r.y >> 1 of the reset draw (include/lmaze.h lmaze_reset_start): Philox4x32-10, counter (env, epoch), key seed"""
    e = np.arange(n, dtype=np.uint64) + np.uint64(env_base)
    c0, c1 = e & M32, e >> np.uint64(32)
    c2, c3 = np.full(n, epoch & 0xFFFFFFFF, np.uint64), np.full(n, epoch >> 32, np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return (c1 >> np.uint64(1)).astype(np.int64)


def bench(name, env, key, weights, rounds):
    dev, N, G = env.device, env.num_envs, env.grid
    S = G * G
    keep = key == "goal"
    thr = PKG.start_thresholds(weights)
    wide = thr.view(torch.int32).to(torch.int64) & 0xFFFFFFFF                  # what searchsorted can read

    def kernel():
        env.reset(thresholds=thr, key=key, keep_goal=keep, validate=False)

    def floor():
        env.reset()

    def placement():
        PKG._abi.check("lmaze_reset_start", PKG._abi.lib.lmaze_reset_start(
            env._pp, env._p_layout, None, thr.data_ptr(), PKG._abi.ROW_MODES[key], 1 if keep else 0, env.seed, env._epoch, env.env_base,
            env._p_ball, env._p_goal if env._is_v3 else None, env._p_step, env._p_reward, env._p_done, None, N, env._stream()))
        env._epoch += 1

    def composition(u):
        if key == "ball":
            k = torch.searchsorted(wide[0], u, right=True)
        else:
            rows = wide if key == "env" else wide[env.state_keys("goal").long() // S]
            k = torch.searchsorted(rows, u[:, None], right=True)[:, 0]
        env.set_state(ball_xy=torch.stack([k // G, k % G], 1))
        env.step_count.zero_()
        env.reward.fill_(-0.0)
        env.done.zero_()
        env.observe()
        return k

    epoch = env._epoch
    kernel()
    cells = env.state_keys("ball").long()
    u = torch.from_numpy(reset_draw_u(env.seed, epoch, N, env.env_base)).to(dev)
    same = bool((composition(u) == cells).all()) and bool((env.state_keys("ball").long() == cells).all())
    med, out = _rounds({"reset_start": kernel, "reset": floor, "torch": lambda: composition(u), "placement": placement}, rounds)
    params = env.params
    res = {"config": name, "variant": env.variant, "envs": N, "grid": G, "key": key, "launch": PKG._abi.describe_reset_start(params, N, key),
           "same_cells": same, "us": out, "torch_over_reset_start": round(med["torch"] / med["reset_start"], 2),
           "reset_start_over_reset": round(med["reset_start"] / med["reset"], 3)}
    if key == "env":
        must = N * S * 4 + N * 17                                              # the rows; ball, counters and flags written
        res.update(placement_bytes=must, placement_share_of_hbm_peak=round(must / (med["placement"] * 1e-6) / HBM_PEAK, 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=int, default=1, help="divide the env counts (rehearsals)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = PKG.layouts
    gen = torch.Generator(dev).manual_seed(1)

    def shared(n, variant, layout, key):
        env = PKG.LmazeVecEnv(n // args.scale, variant=variant, layout=layout, device=dev, seed=3)
        S = env.grid ** 2
        free = (env.layout.reshape(1, S) != ord("W")).float()
        rows = S if key == "goal" else 1
        return env, free * torch.rand((rows, S), device=dev, generator=gen)

    def per_env(n, G):
        lay = L.random_walled(n // args.scale, G, dev)
        env = PKG.LmazeVecEnv(n // args.scale, variant="v0", per_env_layouts=lay, device=dev, seed=3, validate=False)
        return env, PKG.reset_distribution(lay, "v0") * torch.rand((lay.shape[0], G * G), device=dev, generator=gen)

    configs = (("1 65536 x 11x11 shared", "ball", lambda: shared(65536, "v0", L.open_room(11, (5, 5)), "ball")),
               ("2 1048576 x 11x11 shared", "ball", lambda: shared(1 << 20, "v0", L.open_room(11, (5, 5)), "ball")),
               ("3 16384 x 32x32 per-env", "env", lambda: per_env(16384, 32)),
               ("4 65536 x 11x11 per-env", "env", lambda: per_env(65536, 11)),
               ("5 65536 x V3_GRID_18 shared", "goal", lambda: shared(65536, "v3", L.V3_GRID_18, "goal")))
    res, ok = [], True
    for name, key, build in configs:
        env, weights = build()
        r = bench(name, env, key, weights, args.rounds)
        print(json.dumps(r), flush=True)
        res.append(r)
        ok = ok and r["same_cells"]
        del env, weights
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": res}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
