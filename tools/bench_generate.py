"""lmaze_generate (layouts.mazes(): spanning-tree mazes, one launch, a maze in LDS from its draws to its bytes) against two
time yardsticks at the same shape, interleaved rounds in one process, HIP events around ten calls after warm-up, medians
of the per-call time:
    walled  layouts.random_walled -- what a user calls today for per-env layouts.  A different distribution (i.i.d. wall
            noise, free cells not connected), so it is a yardstick for the time only.
    fill    torch.empty(N, G, G, uint8).fill_() of the same bytes: the write floor.
All three write into memory allocated outside the timed region where the call allows it (mazes(out=), fill_);
random_walled allocates its own.  Before the timing the first mazes of every shape are checked: a full 'W' border, one 'X',
R*R - 1 opened walls between the rooms (the tool exits 1 otherwise).
    a  16 384 x 32x32      b  65 536 x 11x11      c  1 048 576 x 11x11      d  16 384 x 64x64

    python tools/bench_generate.py --out profiles/generate/bench_generate.json [--rounds 7]"""
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
SHAPES = (("a 16384 x 32x32", 16384, 32), ("b 65536 x 11x11", 65536, 11), ("c 1048576 x 11x11", 1 << 20, 11), ("d 16384 x 64x64", 16384, 64))


REPS = 10                           # calls inside one timed window: a single call is tens of microseconds


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / REPS


def _rounds(fns, rounds):
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):         # interleaved
        for k, f in fns.items():
            times[k].append(_timed(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {k: {"us": round(med[k], 1), "spread": [round(min(v), 1), round(max(v), 1)]} for k, v in times.items()}


def looks_like_mazes(lay):
    """The cheap properties of a perfect maze, on the device: border, one 'X', R*R rooms free, R*R - 1 walls opened."""
    n, G, _ = lay.shape
    R = (G - 1) // 2
    W = ord("W")
    border = (lay[:, 0, :] == W).all() & (lay[:, -1, :] == W).all() & (lay[:, :, 0] == W).all() & (lay[:, :, -1] == W).all()
    one_goal = ((lay == ord("X")).sum((1, 2)) == 1).all()
    rooms = (lay[:, 1:2 * R:2, 1:2 * R:2] != W).all()
    free = ((lay != W).sum((1, 2)) == 2 * R * R - 1).all()
    return bool(border & one_goal & rooms & free)


def bench(name, N, G, rounds):
    dev = torch.device("cuda", 0)
    L = PKG.layouts
    out = torch.empty((N, G, G), dtype=torch.uint8, device=dev)
    floor = torch.empty((N, G, G), dtype=torch.uint8, device=dev)
    L.mazes(N, G, dev, out=out)
    ok = looks_like_mazes(out[:4096])
    fns = {"generate": lambda: L.mazes(N, G, dev, out=out), "walled": lambda: L.random_walled(N, G, dev),
           "fill": lambda: floor.fill_(ord("W"))}
    med, res = _rounds(fns, rounds)
    nbytes = N * G * G
    return {"config": name, "mazes": N, "grid": G, "bytes": nbytes, "launch": PKG._abi.describe_generate(G, N), "mazes_ok": ok,
            "us": res, "generate_ns_per_maze": round(med["generate"] * 1000.0 / N, 2),
            "generate_GBps": round(nbytes / med["generate"] / 1000.0, 1), "fill_GBps": round(nbytes / med["fill"] / 1000.0, 1),
            "walled_over_generate": round(med["walled"] / med["generate"], 2), "generate_over_fill": round(med["generate"] / med["fill"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=int, default=1, help="divide the maze counts (rehearsals)")
    args = ap.parse_args()
    res, ok = [], True
    for name, N, G in SHAPES:
        r = bench(name, max(1, N // args.scale), G, args.rounds)
        print(json.dumps(r), flush=True)
        res.append(r)
        ok = ok and r["mazes_ok"]
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_window": REPS, "results": res}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
