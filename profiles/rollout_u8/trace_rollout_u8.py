import importlib, sys, torch
sys.path.insert(0, ".")
PKG = importlib.import_module("gym-lmaze_amd")
dev = torch.device("cuda", 0)
N, T = 65536, 16
env = PKG.LmazeVecEnv(N, variant="v0", layout=PKG.layouts.open_room(11, (5, 5)), device=dev, obs_dtype="u8")
a = torch.randint(0, 4, (T, N), dtype=torch.int32, device=dev)
obs_t = torch.empty((T, N, 11, 11), dtype=torch.uint8, device=dev)
for _ in range(3):
    env.rollout(a)
    env.rollout(a, trajectory=True)
    env.rollout(a, obs_t=obs_t, obs_every=1)
torch.cuda.synchronize()
print("9 u8 rollout() calls at 65536 x 11x11, T=16: plain, trajectory=True, obs_every=1, 3 each")
