import importlib, sys, torch
sys.path.insert(0, ".")
PKG = importlib.import_module("gym-lmaze_amd")
dev = torch.device("cuda", 0)
for v, kw in (("v1", {"auto_reset": True}), ("v2", {"auto_reset": True}), ("v4", {}), ("v5", "goals")):
    env = PKG.LmazeFovealVecEnv(16384, variant=v, device=dev, seed=1)
    a = torch.randint(0, 4, (64, 16384), dtype=torch.int32, device=dev)
    g = torch.randint(0, 25, (64, 16384), dtype=torch.int32, device=dev)
    for _ in range(3):
        if kw == "goals":
            env.rollout(a, goals=g, trajectory=True)
        else:
            env.rollout(a, trajectory=True, **kw)
torch.cuda.synchronize()
print("12 rollout() calls: v1 fused, v2 fused, v4 plain, v5 two-level, 3 each, 16384 envs, T=64")
