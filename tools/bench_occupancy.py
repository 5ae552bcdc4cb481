"""lmaze_occupancy (occupancy_tables(): the exact discounted occupancy with the problem in LDS, one launch) against the same
Jacobi sweep written in torch on the device, and against lmaze_evaluate at the same shape with the same table -- interleaved
rounds in one process, HIP events after warm-up, medians.  The torch side gets the gather of every state as tensors built
outside the timed region (the four incoming weights and their source cells, the weight that stays, from bench_solve's model and
bench_evaluate's probabilities; checked here: both sides must give the same d and d_sa bit for bit or the tool exits 1) and
runs the same operations per sweep -- four gathers of D at the sources, a multiply and an add each, the term that stays, the
product with gamma and the sum with start -- with the same early stop: after every sweep it asks whether any bit of D changed,
which is one reduction and one host synchronise per sweep.  A problem that has settled stays where it is, so stopping all
problems together changes no value.  start is reset_distribution(), the law of the cell reset() places the ball on.
    a  16 384 x 32x32   per-env random mazes, v0, sweeps = 128      (occupancy_kernel<v0, workgroup, 4>)
    b  V3_GRID_18       every goal cell (key="goal"), sweeps = 1400  (occupancy_kernel<v3, workgroup, 2>, 324 problems)
    c  65 536 x 11x11   per-env random mazes, v0, sweeps = 128      (occupancy_kernel<v0, wave, 2>)
each with solve()'s policy at epsilon = 0.1 and with random thresholds.  No threshold is fixed: the yardstick is evaluate() per
executed problem-sweep in the same run.

    python tools/bench_occupancy.py --out profiles/occupancy/bench_occupancy.json [--rounds 5]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = importlib.import_module("gym-lmaze_amd")
from bench_evaluate import EPSILON, TWO32, torch_probs   # noqa: E402  (the same probabilities)
from bench_solve import GAMMA, REWARDS, _rounds, torch_model   # noqa: E402  (the same model tensors, the same timing loop)


def torch_gather(model, p):
    """(win float32[P, S, 4], src int64[P, S, 4] flat into [P*S], wself float32[P, S]): the transpose of the model, once"""
    nxt, _, terminal, excluded, wall = model
    P, S = wall.shape
    dev = wall.device
    cells = torch.arange(P * S, device=dev).reshape(P, S)
    flows = ~excluded & ~terminal & ~wall[..., None]
    moved = nxt != cells[..., None]
    win = torch.zeros(P * S, 4, dtype=torch.float32, device=dev)
    src = cells.reshape(-1, 1).repeat(1, 4)
    for a in range(4):
        go = flows[..., a] & moved[..., a]
        c = nxt[..., a][go]                              # one source per (c, a): no index twice
        win[c, a] = p[..., a][go]
        src[c, a] = cells[go]
    wself = torch.zeros(P, S, dtype=torch.float32, device=dev)
    first = torch.ones(P, S, dtype=torch.bool, device=dev)
    for a in range(4):
        use = flows[..., a] & ~moved[..., a]
        wself = torch.where(use, torch.where(first, p[..., a], wself + p[..., a]), wself)
        first = first & ~use
    return win.reshape(P, S, 4), src.reshape(P, S, 4), wself


def torch_occupancy(gather, wall, start, p, sweeps):
    win, src, wself = gather
    P, S = wall.shape
    d = torch.zeros(P * S, dtype=torch.float32, device=wall.device)
    use = [win[..., a] != 0 for a in range(4)]
    use_self = wself != 0
    for _ in range(sweeps):
        acc = torch.zeros(P, S, dtype=torch.float32, device=wall.device)
        for a in range(4):
            term = win[..., a] * d[src[..., a]]
            acc = torch.where(use[a], acc + term, acc)
        term = wself * d.reshape(P, S)
        acc = torch.where(use_self, acc + term, acc)
        new = torch.where(wall, 0.0, start + GAMMA * acc).reshape(-1)
        changed = bool((new.view(torch.int32) != d.view(torch.int32)).any())       # the early stop: a host synchronise
        d = new
        if not changed:
            break
    d = d.reshape(P, S)
    return d, d[..., None] * p


def bench(name, variant, layouts, goals, sweeps, kind, rounds):
    dev = layouts.device
    P = layouts.shape[0] if goals is None else goals.shape[0]
    G = layouts.shape[-1]
    S = G * G
    lay3 = layouts if layouts.dim() == 3 else layouts[None].expand(P, G, G).contiguous()
    model = torch_model(lay3, variant, goals)
    wall = model[4]
    common = dict(variant=variant, goals=goals, gamma=GAMMA, sweeps=sweeps, rewards=REWARDS, validate=False)
    solved = PKG.solve_tables(layouts, **common)
    if kind == "policy":
        table = dict(policy=solved.policy, epsilon=EPSILON)
        p = torch_probs(model, policy=solved.policy, epsilon_u32=PKG._abi.epsilon_u32(EPSILON))
    else:
        gen = torch.Generator(dev).manual_seed(P + G)
        c = torch.randint(0, TWO32, (P, S, 4), device=dev, generator=gen)
        c[..., :3] = c[..., :3].sort(dim=-1).values
        thr = torch.where(c >= TWO32 // 2, c - TWO32, c).to(torch.int32).contiguous()
        table = dict(thresholds=thr)
        p = torch_probs(model, thresholds=thr)
    start = PKG.reset_distribution(layouts, variant, goals)
    gather = torch_gather(model, p)

    def kernel():
        return PKG.occupancy_tables(layouts, start, **common, **table)

    def evaluate():
        return PKG.evaluate_tables(layouts, **common, **table)
    got, ev = kernel(), evaluate()
    torch.cuda.synchronize()
    td, tdsa = torch_occupancy(gather, wall, start, p, sweeps)
    same = bool(torch.equal(td.view(torch.int32), got.d.view(torch.int32)) and torch.equal(tdsa.view(torch.int32), got.d_sa.view(torch.int32)))
    med, out = _rounds({"occupancy": kernel, "torch": lambda: torch_occupancy(gather, wall, start, p, sweeps), "evaluate": evaluate}, rounds)
    params = PKG._abi.make_params(PKG.VARIANTS[variant]["id"], G, 1 if layouts.dim() == 3 else 0, 100, *REWARDS)
    run, erun = got.sweeps_run.double(), ev.sweeps_run.double()
    occ_ns = med["occupancy"] * 1000.0 / float(run.sum())
    ev_ns = med["evaluate"] * 1000.0 / float(erun.sum())
    return {"config": name, "policy": kind, "variant": variant, "problems": P, "grid": G, "sweeps": sweeps,
            "launch": PKG._abi.describe_occupancy(params, P),
            "sweeps_run": {"min": int(run.min()), "mean": round(float(run.mean()), 1), "max": int(run.max())},
            "evaluate_sweeps_run": {"min": int(erun.min()), "mean": round(float(erun.mean()), 1), "max": int(erun.max())},
            "same_bits": same, "us": out, "torch_over_occupancy": round(med["torch"] / med["occupancy"], 1),
            "occupancy_ns_per_problem_sweep": round(occ_ns, 2), "evaluate_ns_per_problem_sweep": round(ev_ns, 2),
            "occupancy_over_evaluate_per_problem_sweep": round(occ_ns / ev_ns, 3)}


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
        for kind in ("policy", "thresholds"):
            r = bench(name, variant, layouts, g, sweeps, kind, args.rounds)
            print(json.dumps(r), flush=True)
            res.append(r)
            ok = ok and r["same_bits"]
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "gamma": GAMMA, "epsilon": EPSILON, "results": res},
                      f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
