import importlib, sys, torch
sys.path.insert(0, ".")
PKG = importlib.import_module("gym-lmaze_amd")
dev = torch.device("cuda", 0)
N, T = 65536, 16
grid = PKG.LmazeVecEnv(N, variant="v0", layout=PKG.layouts.open_room(11, (5, 5)), device=dev)
fov = PKG.LmazeFovealVecEnv(N, variant="v2", device=dev, seed=1)
a = torch.randint(0, 4, (T, N), dtype=torch.int32, device=dev)
obs_t = torch.empty((T, N, 11, 11), dtype=torch.int32, device=dev)
fobs_t = torch.empty((T,) + tuple(fov.obs.shape), dtype=torch.float32, device=dev)
for _ in range(3):
    grid.rollout(a, obs_t=obs_t, obs_every=1)
    grid.rollout(a, obs_every=0)
    fov.rollout(a, auto_reset=True, obs_t=fobs_t, obs_every=1)
torch.cuda.synchronize()
print("9 rollout() calls at 65536 envs, T=16: v0 11x11 obs_every=1 and obs_every=0, v2 fused obs_every=1, 3 each")
