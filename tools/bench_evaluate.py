"""lmaze_evaluate (evaluate_tables(): exact policy evaluation with the problem in LDS, one launch) against the same Jacobi sweep
written in torch on the device, and against lmaze_solve at the same shape -- interleaved rounds in one process, HIP events
after warm-up, medians.  The torch side gets the model and the four probabilities of every state as tensors built outside the
timed region (its own restatement of the transition and of the weight rule, checked here: both sides must give the same V and
Q bit for bit or the tool exits 1) and runs the same operations per sweep -- a gather of V at the successor, a multiply, an
add, a select for the terminal pairs, then the four products and the sums in the header's order -- with the same early stop:
after every sweep it asks whether any bit of V changed, which is one reduction and one host synchronise per sweep.  A problem
that has settled stays where it is, so stopping all problems together changes no value.
    a  16 384 x 32x32   per-env random mazes, v0, sweeps = 128      (evaluate_kernel<v0, workgroup, 4>)
    b  V3_GRID_18       every goal cell (key="goal"), sweeps = 1400  (evaluate_kernel<v3, workgroup, 2>, 324 problems)
    c  65 536 x 11x11   per-env random mazes, v0, sweeps = 128      (evaluate_kernel<v0, wave, 2>)
each with solve()'s policy at epsilon = 0.1 and with random thresholds.

    python tools/bench_evaluate.py --out profiles/evaluate/bench_evaluate.json [--rounds 5]"""
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
from bench_solve import GAMMA, REWARDS, _rounds, torch_model   # noqa: E402  (the same model tensors, the same timing loop)

EPSILON = 0.1
TWO32 = 1 << 32


def torch_probs(model, policy=None, epsilon_u32=0, thresholds=None):
    """float32[P, S, 4]: the header's weight rule in int64, the weight on an excluded pair dropped, one division"""
    _, _, _, excluded, wall = model
    if thresholds is not None:
        c = (thresholds.to(torch.int64) & (TWO32 - 1))[..., :3].sort(dim=-1).values
        w = 4 * torch.stack([c[..., 0], c[..., 1] - c[..., 0], c[..., 2] - c[..., 1], TWO32 - c[..., 2]], dim=-1)
    else:
        hit = policy[..., None].to(torch.int64) == torch.arange(4, device=policy.device)
        w = epsilon_u32 + torch.where(hit, 4 * (TWO32 - epsilon_u32), 0)
    w = torch.where(excluded | wall[..., None], 0, w)
    W = w.sum(-1, keepdim=True)
    return torch.where(W == 0, 0.0, w.to(torch.float32) / W.clamp(min=1).to(torch.float32)).contiguous()


def torch_evaluate(model, p, sweeps):
    nxt, r, terminal, excluded, wall = model
    P, S = wall.shape
    v = torch.zeros(P * S, dtype=torch.float32, device=r.device)
    ninf = torch.tensor(float("-inf"), dtype=torch.float32, device=r.device)
    use = [p[..., a] != 0 for a in range(4)]
    first, seen = [], torch.zeros_like(use[0])
    for a in range(4):                                  # the action a state's sum starts from
        first.append(use[a] & ~seen)
        seen = seen | use[a]
    q = None
    for _ in range(sweeps):
        q = torch.where(terminal, r, r + GAMMA * v[nxt])
        q = torch.where(excluded, ninf, q)
        new = torch.zeros(P, S, dtype=torch.float32, device=r.device)
        for a in range(4):
            term = p[..., a] * q[..., a]
            new = torch.where(use[a], torch.where(first[a], term, new + term), new)
        new = new.reshape(-1)
        changed = bool((new.view(torch.int32) != v.view(torch.int32)).any())       # the early stop: a host synchronise
        v = new
        if not changed:
            break
    q = torch.where(wall[..., None], 0.0, q)
    return v.reshape(P, S), q


def bench(name, variant, layouts, goals, sweeps, kind, rounds):
    dev = layouts.device
    P = layouts.shape[0] if goals is None else goals.shape[0]
    G = layouts.shape[-1]
    S = G * G
    lay3 = layouts if layouts.dim() == 3 else layouts[None].expand(P, G, G).contiguous()
    model = torch_model(lay3, variant, goals)
    common = dict(variant=variant, goals=goals, gamma=GAMMA, sweeps=sweeps, rewards=REWARDS, validate=False)

    def solve():
        return PKG.solve_tables(layouts, **common)
    solved = solve()
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

    def kernel():
        return PKG.evaluate_tables(layouts, **common, **table)
    got = kernel()
    torch.cuda.synchronize()
    longest = int(got.sweeps_run.max())
    tv, tq = torch_evaluate(model, p, sweeps)
    same = bool(torch.equal(tv.view(torch.int32), got.v.view(torch.int32)) and torch.equal(tq.view(torch.int32), got.q.view(torch.int32)))
    med, out = _rounds({"evaluate": kernel, "torch": lambda: torch_evaluate(model, p, sweeps), "solve": solve}, rounds)
    params = PKG._abi.make_params(PKG.VARIANTS[variant]["id"], G, 1 if layouts.dim() == 3 else 0, 100, *REWARDS)
    run, srun = got.sweeps_run.double(), solved.sweeps_run.double()
    return {"config": name, "policy": kind, "variant": variant, "problems": P, "grid": G, "sweeps": sweeps,
            "launch": PKG._abi.describe_evaluate(params, P),
            "sweeps_run": {"min": int(run.min()), "mean": round(float(run.mean()), 1), "max": longest},
            "solve_sweeps_run": {"min": int(srun.min()), "mean": round(float(srun.mean()), 1), "max": int(srun.max())},
            "same_bits": same, "us": out, "torch_over_evaluate": round(med["torch"] / med["evaluate"], 1),
            "evaluate_ns_per_problem_sweep": round(med["evaluate"] * 1000.0 / float(run.sum()), 2),
            "solve_ns_per_problem_sweep": round(med["solve"] * 1000.0 / float(srun.sum()), 2)}


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
