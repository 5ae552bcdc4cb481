"""Host plumbing shared by LmazeVecEnv and LmazeFovealVecEnv: device, the per-env state block and its host mirror,
streams, argument conversion, the reset epoch (host-counted, or device-resident under graph capture), captured
rollouts, episode counters and the autotune() driver.  Nothing here is arithmetic of the step path."""
import numpy as np
import torch

from . import _abi
from . import _tables
from . import _tuning

_NUMPY = {torch.int32: np.int32, torch.float32: np.float32, torch.uint8: np.uint8}


def _align(n, a=256):
    return (n + a - 1) // a * a


def resolve_device(device):
    if device is None:
        device = "cuda"
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("gym-lmaze_amd runs on MI355X only (device=%r): the HIP kernels are the "
                           "only implementation of the step path, there is no CPU fallback" % (device,))
    if not torch.cuda.is_available():
        raise RuntimeError("gym-lmaze_amd: no HIP device visible; the step path cannot run")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class VecEnvBase(object):
    """What both engines do the same way.  A subclass sets `params`, `obs` and `_expanded`, and defines
    _set_policy(policy) and _set_obs(ptr) for autotune()."""

    _tuner = None                                   # LmazeVecEnv's online tuner while it runs
    _STATS_KEYS = ("done", "goal_rewards", "done_steps")
    _gc_ptr = None                                  # goal counts summed by episode_stats(), where the variant keeps them

    def _init_common(self, num_envs, device, seed, env_base):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.device = resolve_device(device)
        self.seed, self.env_base, self._epoch = int(seed), int(env_base), 0
        self.tuned_policy = None        # the policy autotune() (or the online tuner) has chosen
        self.placement = None           # autotune(placement_trials=K): where the observation buffer ended up
        self._captured = 0              # captured rollouts: they keep raw pointers, so autotune() no longer moves obs

    def _alloc_state(self, fields):
        """ONE allocation for every per-env scalar, so that a host mirror is a single copy.  fields: (name, dtype,
        values per env); each becomes the attribute `name`, a view of the block (uint8 flags as bool)."""
        N, offs, total = self.num_envs, [], 0
        for _, dt, w in fields:
            offs.append(total)
            total += _align(N * w * dt.itemsize)
        self._state = torch.zeros(total, dtype=torch.uint8, device=self.device)
        # device-resident epoch pair of captured steps that reset envs; allocated here, never under capture (an
        # allocation inside a capture becomes a memset node that every replay would re-run)
        self._epoch_words = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._p_epoch = self._epoch_words.data_ptr()
        self._views = {}
        for (name, dt, w), off in zip(fields, offs):
            v = self._state[off:off + N * w * dt.itemsize].view(dt).view((N, w) if w > 1 else (N,))
            self._views[name] = v
            setattr(self, name, v.view(torch.bool) if dt == torch.uint8 else v)
        self._persistent = [self._state]            # what snapshot() saves

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _guard(self):
        return torch.cuda.device(self.device)

    def _as_i32(self, x, numel):
        if isinstance(x, torch.Tensor):
            t = x if (x.device == self.device and x.dtype == torch.int32) else x.to(device=self.device, dtype=torch.int32)
        else:
            t = torch.as_tensor(np.asarray(x, dtype=np.int64).astype(np.int32), device=self.device)
        t = t.reshape(-1).contiguous()
        if t.numel() != numel:
            raise ValueError("expected %d values, got %d" % (numel, t.numel()))
        return t

    def _mask_ptr(self, mask):
        """(uint8 mask tensor, its address) -- keep the tensor alive across the launch; (None, None) = every env."""
        if mask is None:
            return None, None
        m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask), device=self.device)
        m = m.to(device=self.device)
        m = (m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).to(torch.uint8)).contiguous()
        if m.numel() != self.num_envs:
            raise ValueError("mask must have %d entries" % self.num_envs)
        return m, m.data_ptr()

    def _check_rows(self, who, *tensors):
        for t in tensors:
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.dim() == 2
                                      and t.shape[1] == self.num_envs and t.device == self.device and t.is_contiguous()):
                raise ValueError("%s wants contiguous int32[T,N] tensors on %s" % (who, self.device))

    def _obs_slots(self, T, obs_every, obs_t, like, allow_final=False, name="obs_t"):
        """Checks a rollout's recording request (obs_every, and its out-parameter obs_t shaped (T // k, N) + like.shape[1:]
        with like's dtype) before anything is launched; returns k.  allow_final: obs_every = 0, the final planes only
        (obs_t None), is accepted."""
        if isinstance(obs_every, bool) or not isinstance(obs_every, (int, np.integer)):
            raise ValueError("obs_every must be an int")
        k = int(obs_every)
        if k < (0 if allow_final else 1):
            raise ValueError("obs_every must be >= %d%s" % (0 if allow_final else 1,
                                                            "" if allow_final else " (obs_every=0 is the grid env's)"))
        if k == 0:
            if obs_t is not None:
                raise ValueError("obs_every=0 records the final planes only: %s must be None" % name)
            return 0
        shape = (int(T) // k, self.num_envs) + tuple(like.shape[1:])
        if not isinstance(obs_t, torch.Tensor):
            raise ValueError("%s must be a tensor of shape %s" % (name, shape))
        if tuple(obs_t.shape) != shape:
            raise ValueError("%s has shape %s, expected %s" % (name, tuple(obs_t.shape), shape))
        if obs_t.dtype != like.dtype:
            raise ValueError("%s has dtype %s, expected %s" % (name, obs_t.dtype, like.dtype))
        if obs_t.device != self.device or not obs_t.is_contiguous() or obs_t.data_ptr() % 16:
            raise ValueError("%s must be contiguous, on %s and 16-byte aligned" % (name, self.device))
        return k

    def _traj_rows(self, T, streams=1):
        """A rollout's trajectory rows: float32[T,N] reward and uint8[T,N] done for each of `streams` streams (the second:
        foveal_reward / foveal_done)."""
        return [torch.empty((int(T), self.num_envs), dtype=dt, device=self.device)
                for _ in range(streams) for dt in (torch.float32, torch.uint8)]

    def _rollout_result(self, rows):
        """What rollout() returns: the final (obs, reward, done) and, with trajectory rows, each stream's reward row and
        done row (as bool)."""
        out = (self.obs, self.reward, self.done)
        for i in range(0, len(rows or ()), 2):
            out += (rows[i], rows[i + 1].view(torch.bool))
        return out

    # ------------------------------------------------------------------ closed-loop rollouts (rollout_policy() and its kin)
    @staticmethod
    def _steps(T):
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 0:
            raise ValueError("T must be an int >= 0")
        return int(T)

    greedy_table = staticmethod(_tables.greedy_table)

    def _closed_loop(self, who, name, call, T, k, obs_t, trajectory, actions_t, key_t, streams=1, more=None):
        """What every closed-loop rollout does around its ABI call `name`, once its table and its recording request (k =
        _obs_slots()) are checked: the actions_t / key_t rows (checked; allocated under trajectory=True), the trajectory
        rows of `streams` streams, the launch -- call(row addresses, actions_t's, key_t's, the slots') returns the ABI's
        code -- the epoch, which advances by T, and the result: rollout()'s, then under trajectory=True actions_t, key_t.
        more: further int32[T,N] rows as (label, tensor or None) pairs (the two-level loop's goals_t, goal_key_t), treated as
        actions_t / key_t are; their addresses are call's fifth argument and they follow key_t in the result."""
        named = [("actions_t", actions_t), ("key_t", key_t)] + list(more or ())
        self._check_rows(who, *(t for _, t in named))
        for label, t in named:
            if t is not None and t.shape[0] != T:
                raise ValueError("%s must have T = %d rows" % (label, T))
        rows = self._traj_rows(T, streams) if trajectory else None
        if trajectory:
            named = [(label, torch.empty((T, self.num_envs), dtype=torch.int32, device=self.device) if t is None else t)
                     for label, t in named]
        ptrs = [None if t is None else t.data_ptr() for _, t in named]
        slots = obs_t.data_ptr() if k > 0 and obs_t.shape[0] > 0 else None
        with self._guard():
            rc = call([r.data_ptr() for r in rows or ()], ptrs[0], ptrs[1], slots, *([ptrs[2:]] if more is not None else []))
        _abi.check(name, rc)
        self._epoch += T
        out = self._rollout_result(rows)
        return out + tuple(t for _, t in named) if trajectory else out

    def host_state(self, raw=None):
        """Every per-env scalar on the host: numpy views of ONE device->host copy of the state block.  raw: bytes of
        the block already on the host (uint8 array the size of `_state`), parsed instead of copying again."""
        h = self._state.cpu().numpy() if raw is None else raw
        base, out = self._state.data_ptr(), {}
        for name, v in self._views.items():
            off = v.data_ptr() - base
            out[name] = h[off:off + v.numel() * v.element_size()].view(_NUMPY[v.dtype]).reshape(tuple(v.shape))
        return out

    def _write_state(self, name, src):
        dst = self._views[name] if name in self._views else getattr(self, name)
        t = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))
        dst.copy_(t.to(device=self.device).to(dst.dtype).reshape(dst.shape))

    def snapshot(self):
        """Everything a step reads and writes except the observations (per-env scalars, visit maps) and the epoch."""
        return tuple(t.clone() for t in self._persistent) + (self._epoch,)

    def restore(self, snap):
        for t, s in zip(self._persistent, snap):
            t.copy_(s)
        self._epoch = snap[-1]

    # ------------------------------------------------------------------ the reset epoch
    def _epoch_args(self, resets, slot):
        """(epoch, epoch_in_dev, epoch_out_dev) for a launch that may reset envs.  Eagerly the host counts the epochs
        (advanced here); under capture (slot = index t of the launch in the captured sequence) the count is on the
        device, in two words the launches hand on to each other, so the frozen host arguments stay valid for every
        replay (see begin_replay)."""
        if not resets:
            return 0, None, None
        if slot is None:
            self._epoch += 1
            return self._epoch - 1, None, None
        t = int(slot)
        return 0, self._p_epoch + 8 * (t & 1), self._p_epoch + 8 * ((t + 1) & 1)

    def begin_replay(self, n_launches):
        """Call before replaying a captured sequence of n_launches steps that reset envs: hands the host's epoch count to
        the device word the first launch reads (one tiny fill on the current stream, no sync) and reserves n_launches
        epochs, so every replay -- and every eager call in between -- draws placements no earlier launch has used."""
        self._epoch_words[0:1].fill_(self._epoch)
        self._epoch += int(n_launches)

    def _capture(self, n_launches, resets, record):
        """Capture what record() launches (a rollout()) into ONE hipGraph; returns a RolloutGraph (call .replay()).  For
        launch-bound batch sizes (65 536 x 8x8 is 6 us per step, a third of it launch gap).  The launches allocate
        nothing and never synchronise, so they are capturable as they are.  With resets in the rollout the epoch is a
        device word the launches hand on to each other (epoch_in_dev / epoch_out_dev), so every replay draws fresh
        placements, exactly those the same steps launched eagerly would draw.  What is recorded is what rollout()
        launches: LmazeVecEnv without auto_reset records its one-launch lmaze_rollout (u8: lmaze_rollout_u8), with
        auto_reset T step launches; LmazeFovealVecEnv always records T step launches."""
        if self._tuner is not None:             # still cycling through candidates: a graph bakes the default policy
            self.params.launch_hint = 0
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                record()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self._captured += 1
        return RolloutGraph(self, graph, int(n_launches), resets)

    # ------------------------------------------------------------------ off the step path
    def episode_stats(self, all_ranks=False):
        """Counters over the batch, off the step path (lmaze_episode_stats): "done" (envs with done set),
        "goal_rewards" (envs whose reward is the goal reward), "done_steps" (step counts summed over the done envs) and,
        for LmazeVecEnv, "goal_count".  all_ranks=True sums them over the process group (one all_reduce of four int64
        over RCCL): the only collective the library ever issues.  Synchronises (returns Python ints)."""
        v = self._views
        out = torch.empty(4, dtype=torch.int64, device=self.device)
        with self._guard():
            rc = _abi.lib.lmaze_episode_stats(v["done"].data_ptr(), v["reward"].data_ptr(), v["step_count"].data_ptr(),
                                              self._gc_ptr, self.params.reward_goal, self.num_envs, out.data_ptr(),
                                              self._stream())
        _abi.check("lmaze_episode_stats", rc)
        if all_ranks:
            from .sharding import sum_over_ranks
            out = sum_over_ranks(out, device=self.device)
        return dict(zip(self._STATS_KEYS, out.tolist()))

    def _tune(self, rows, step_row, frames=(), placement_trials=0, **kw):
        """_tuning.autotune() over real steps: step_row(r) launches one step on action row r (rows cycled in order)
        under the policy _set_policy() chose, on the buffer _set_obs() pointed at.  snapshot() and `frames` are saved
        before and restored after, so results are unaffected; the chosen policy stays in force.  Returns the
        timings."""
        if int(placement_trials) > 1 and self._captured:
            raise RuntimeError("autotune(placement_trials > 1) would move the observation buffer under %d captured "
                               "rollout(s), which keep raw pointers to it: tune before capture_rollout()" % self._captured)
        snap = self.snapshot()
        saved = [f.clone() for f in frames]
        k = [0]

        def run(n):
            for _ in range(n):
                step_row(k[0] % rows)
                k[0] += 1

        with self._guard():
            timings, best, placement = _tuning.autotune(run, self._set_policy, self._set_obs, self.obs,
                                                        placement_trials=placement_trials, **kw)
            self.restore(snap)
            for f, s in zip(frames, saved):
                f.copy_(s)
        if placement is not None:
            self.placement, self._expanded = placement, None
        self._set_policy(best)
        self.tuned_policy = best
        return timings


class RolloutGraph:
    """A captured rollout (capture_rollout): replay() relaunches its steps in one go."""

    def __init__(self, env, graph, n_launches, auto_reset):
        self.env, self.graph, self.n_launches, self.auto_reset = env, graph, n_launches, auto_reset

    def replay(self):
        if self.auto_reset:
            self.env.begin_replay(self.n_launches)
        self.graph.replay()
