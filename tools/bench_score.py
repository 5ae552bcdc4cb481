"""lmaze_score (score_tables(): distances and greedy walk lengths with the problem in LDS, one launch) against the same
computation written in torch on the device: gather-based min-plus sweeps over [P, S] tensors with the same early stop (a sweep
that changes nothing ends them, which costs the torch loop a reduction and a host synchronise per sweep), then gather-based
pointer doubling with the same trip count and the same early stop.  Interleaved rounds in one process, HIP events after
warm-up, medians.  The torch side gets the model as tensors built outside the timed region (bench_solve.py's restatement of
the transition); both sides must give the same integers or the tool exits 1.
    a  16 384 x 32x32   per-env generated mazes (loops 0.25), v0     (score_kernel<v0, workgroup, 4>)
    b  65 536 x 11x11   per-env generated mazes (loops 0.25), v0     (score_kernel<v0, wave, 2>)
    c  16 384 x 64x64   per-env generated mazes (loops 0.25), v0     (score_kernel<v0, workgroup, 16>)
each with solve()'s policy (every walk arrives: the doubling stops early) and with uniformly random bytes (cycles: every round
runs).

    python tools/bench_score.py --out profiles/score/bench_score.json [--rounds 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_solve import PKG, REWARDS, _rounds, torch_model  # noqa: E402

INF = 0x3FFFFFFF
ARRIVED, NEVER = -1, -2


def torch_score(model, policy):
    """(optimal int32[P, S], steps int32[P, S], sweeps run, rounds run)"""
    nxt, _, terminal, excluded, wall = model
    P, S = wall.shape
    dev = wall.device
    usable = ~excluded & ~wall[:, :, None]
    inf = torch.tensor(INF, dtype=torch.int32, device=dev)
    d = torch.where((terminal & usable).any(dim=2), 1, INF).to(torch.int32).reshape(-1)
    sweeps = 0
    for _ in range(S):
        sweeps += 1
        via = torch.where(terminal, 0, d[nxt]) + 1
        new = torch.where(usable, via, inf).min(dim=2).values.clamp(max=INF).reshape(-1)
        same = torch.equal(new, d)
        d = new
        if same:
            break
    optimal = torch.where(d >= INF, -1, d).reshape(P, S)
    a = policy.long()[:, :, None]
    to = nxt.gather(2, a)[:, :, 0].reshape(-1)
    term = terminal.gather(2, a)[:, :, 0].reshape(-1)
    excl = excluded.gather(2, a)[:, :, 0].reshape(-1)
    own = torch.arange(P * S, device=dev)
    never = wall.reshape(-1) | excl | (~term & (to == own))
    ptr = torch.where(term & ~never, ARRIVED, torch.where(never, NEVER, to))
    length = torch.ones(P * S, dtype=torch.int32, device=dev)
    rounds = 0
    for _ in range((S - 1).bit_length()):
        rounds += 1
        live = ptr >= 0
        at = torch.where(live, ptr, 0)
        p2, l2 = ptr[at], length[at]
        length = torch.where(live & (p2 != NEVER), length + l2, length)
        ptr = torch.where(live, p2, ptr)
        if not bool((ptr >= 0).any()):
            break
    steps = torch.where(ptr == ARRIVED, length, -1).reshape(P, S)
    return optimal, steps, sweeps, rounds


def bench(name, layouts, table, policy, rounds):
    P, G, _ = layouts.shape
    model = torch_model(layouts, "v0", None)

    def kernel():
        return PKG.score_tables(layouts, policy=policy, rewards=REWARDS, validate=False)
    got = kernel()
    optimal, steps, sweeps, dbl = torch_score(model, policy)
    same = bool(torch.equal(optimal, got.optimal)) and bool(torch.equal(steps, got.steps))
    med, out = _rounds({"kernel": kernel, "torch": lambda: torch_score(model, policy)}, rounds)
    params = PKG._abi.make_params(PKG.VARIANTS["v0"]["id"], G, 1, 100, *REWARDS)
    s = got.summary.double().sum(0)
    return {"config": name, "table": table, "problems": P, "grid": G, "launch": PKG._abi.describe_score(params, P),
            "torch_sweeps": sweeps, "torch_rounds": dbl, "longest_optimal": int(got.optimal.max()), "longest_walk": int(got.steps.max()),
            "share_arrived": round(float(s[1] / s[0]), 4), "share_shortest": round(float(s[2] / s[0]), 4), "same_integers": same,
            "us_per_score": out, "torch_over_kernel": round(med["torch"] / med["kernel"], 1),
            "kernel_ns_per_problem": round(med["kernel"] * 1000.0 / P, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem counts (rehearsals)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res, ok = [], True
    for name, P, G in (("a 16384 x 32x32 per-env", 16384, 32), ("b 65536 x 11x11 per-env", 65536, 11), ("c 16384 x 64x64 per-env", 16384, 64)):
        P //= args.scale
        layouts = PKG.layouts.mazes(P, G, dev, seed=7, loops=0.25)
        solved = PKG.solve_tables(layouts, gamma=0.99, rewards=REWARDS, outputs=("policy",), validate=False).policy
        gen = torch.Generator(device=dev).manual_seed(5)
        random = torch.randint(0, 4, (P, G * G), device=dev, generator=gen).to(torch.uint8)
        for table, policy in (("solve()", solved), ("random", random)):
            r = bench(name, layouts, table, policy, args.rounds)
            print(json.dumps(r), flush=True)
            res.append(r)
            ok = ok and r["same_integers"]
        del layouts, solved, random
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": res}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
