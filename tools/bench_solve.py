"""lmaze_solve (solve_tables(): value iteration with the problem in LDS, one launch) against the same Jacobi sweep written in
torch on the device -- per sweep one gather of V at the successor, a multiply, an add, a select for the terminal pairs and a
max over the four actions -- interleaved rounds in one process, HIP events after warm-up, medians.  The torch side gets the
model as tensors built outside the timed region (its own restatement of the transition, checked here: both sides must
give the same V bit for bit or the tool exits 1) and runs exactly as many sweeps as the kernel's slowest problem did, with
no convergence test -- a user's loop would add a reduction and a host synchronise every few sweeps.
    a  16 384 x 32x32   per-env random mazes, v0, sweeps = 128      (solve_kernel<v0, workgroup, 4>)
    b  V3_GRID_18       every goal cell (key="goal"), sweeps = 1400  (solve_kernel<v3, workgroup, 2>, 324 problems)
    c  65 536 x 11x11   per-env random mazes, v0, sweeps = 128      (solve_kernel<v0, wave, 2>)

    python tools/bench_solve.py --out profiles/solve/bench_solve.json [--rounds 5]"""
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
GAMMA = 0.99
REWARDS = (-1.0, -0.01, 100.0)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


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


def torch_model(layouts, variant, goals):
    """(nxt int64[P, S, 4] flat into [P*S], r float32[P, S, 4], terminal, excluded bool[P, S, 4], wall bool[P, S]) of layouts
    uint8[P, G, G] (v3: goals int32[P, 2]); bordered layouts, so every target of a non-wall cell is on the grid."""
    P, G, _ = layouts.shape
    S, dev = G * G, layouts.device
    rw, rm, rg = (torch.tensor(x, dtype=torch.float32, device=dev) for x in REWARDS)
    flat = layouts.reshape(P, S)
    s = torch.arange(S, device=dev)
    x, y = s // G, s % G
    nxt, r, excluded = [], [], []
    for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        tx, ty = (x + ox).clamp(0, G - 1), (y + oy).clamp(0, G - 1)
        t = tx * G + ty
        c = flat[:, t]
        bump = c == ord("W")
        if variant == "v3":
            hit = ((tx + ox)[None, :] == goals[:, 0:1]) & ((ty + oy)[None, :] == goals[:, 1:2])
            ra = torch.where(bump, rw, torch.where(hit, rg, rm))
            ex = torch.zeros_like(bump)
        else:
            ra = torch.where(bump, rw, torch.where(c == ord("X"), rg, rm))
            ex = ~bump & (c != ord("B")) & (c != ord("X"))
        nxt.append(torch.where(bump | ex, s[None, :], t[None, :]))
        r.append(ra)
        excluded.append(ex)
    nxt, r, excluded = (torch.stack(v, dim=2) for v in (nxt, r, excluded))
    nxt = nxt + (torch.arange(P, device=dev) * S)[:, None, None]
    return nxt, r.contiguous(), (r == rg) & ~excluded, excluded, flat == ord("W")


def torch_solve(model, sweeps):
    nxt, r, terminal, excluded, wall = model
    P, S = wall.shape
    v = torch.zeros(P * S, dtype=torch.float32, device=r.device)
    dead = wall | excluded.all(dim=2)
    ninf = torch.tensor(float("-inf"), dtype=torch.float32, device=r.device)
    for _ in range(sweeps):
        q = torch.where(terminal, r, r + GAMMA * v[nxt])
        q = torch.where(excluded, ninf, q)
        v = torch.where(dead, 0.0, q.max(dim=2).values).reshape(-1)
    return v.reshape(P, S)


def bench(name, variant, layouts, goals, sweeps, rounds):
    dev = layouts.device
    per_env = layouts if layouts.dim() == 3 and goals is None else None
    P = layouts.shape[0] if per_env is not None else goals.shape[0]
    G = layouts.shape[-1]
    lay3 = layouts if layouts.dim() == 3 else layouts[None].expand(P, G, G).contiguous()
    model = torch_model(lay3, variant, goals)

    def kernel():
        return PKG.solve_tables(layouts, variant=variant, goals=goals, gamma=GAMMA, sweeps=sweeps, rewards=REWARDS, validate=False)
    got = kernel()
    torch.cuda.synchronize()
    longest = int(got.sweeps_run.max())
    same = bool(torch.equal(torch_solve(model, longest).view(torch.int32), got.v.view(torch.int32)))
    med, out = _rounds({"kernel": kernel, "torch": lambda: torch_solve(model, longest)}, rounds)
    params = PKG._abi.make_params(PKG.VARIANTS[variant]["id"], G, 1 if layouts.dim() == 3 else 0, 100, *REWARDS)
    run = got.sweeps_run.double()
    return {"config": name, "variant": variant, "problems": P, "grid": G, "sweeps": sweeps, "launch": PKG._abi.describe_solve(params, P),
            "sweeps_run": {"min": int(run.min()), "mean": round(float(run.mean()), 1), "max": longest},
            "torch_sweeps": longest, "same_bits": same, "us_per_solve": out, "torch_over_kernel": round(med["torch"] / med["kernel"], 1),
            "kernel_ns_per_problem_sweep": round(med["kernel"] * 1000.0 / float(run.sum()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem counts (rehearsals)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = PKG.layouts
    G18 = 18
    cells = torch.arange(G18 * G18, dtype=torch.int32, device=dev)
    goals = torch.stack([cells // G18, cells % G18], dim=1).to(torch.int32).contiguous()
    shared = torch.from_numpy(L.to_codes(L.V3_GRID_18).copy()).to(dev)
    configs = (("a 16384 x 32x32 per-env", "v0", L.random_walled(16384 // args.scale, 32, dev), None, 128),
               ("b V3_GRID_18 every goal", "v3", shared, goals, 1400),
               ("c 65536 x 11x11 per-env", "v0", L.random_walled(65536 // args.scale, 11, dev), None, 128))
    res, ok = [], True
    for name, variant, layouts, g, sweeps in configs:
        r = bench(name, variant, layouts, g, sweeps, args.rounds)
        print(json.dumps(r), flush=True)
        res.append(r)
        ok = ok and r["same_bits"]
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "gamma": GAMMA, "results": res}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
