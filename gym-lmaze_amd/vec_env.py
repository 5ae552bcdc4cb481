"""LmazeVecEnv: N independent L-mazes held as struct-of-arrays torch tensors in HBM and
stepped by one HIP kernel per step() through the C ABI of include/lmaze.h.

Host side only: buffer ownership, argument marshalling, stream selection.  All arithmetic
of the path (collision check, position update, reward/done, plane render, xE render,
masked reset) runs in liblmaze_hip.so; there is no CPU implementation in this package.

Reference semantics: gym_lmaze/envs/lmaze_env.py (v0) and lmaze_env_v3.py (v3).
"""
import collections
import ctypes as C
import logging

import numpy as np
import torch

from . import _abi
from . import _tables
from . import layouts as L
from ._base import VecEnvBase
from ._tuning import OnlineTuner

_log = logging.getLogger("gym_lmaze_amd")

# per-variant constants the reference hard-codes in __init__
VARIANTS = {
    # lmaze_env.py:16-25, planes lmaze_env.py:208-215 (ball, wall, goal, blank)
    "v0": dict(id=_abi.VARIANT_V0, layout=L.V0_GRID_12, expansion=7, step_limit=100,
               rewards=(-1.0, -0.01, 100.0), channel_mask=(_abi.OBS_BALL, _abi.OBS_WALL, _abi.OBS_GOAL, _abi.OBS_FREE),
               n_actions=4),
    # lmaze_env_v3.py:76-99, planes lmaze_env_v3.py:291-293 (free, ball, goal)
    "v3": dict(id=_abi.VARIANT_V3, layout=L.V3_GRID_18, expansion=4, step_limit=100,
               rewards=(-1.0, -0.01, 100.0), channel_mask=(_abi.OBS_FREE, _abi.OBS_BALL, _abi.OBS_GOAL),
               n_actions=4),
}


class LmazeVecEnv(VecEnvBase):
    """N mazes with `variant` transition rules.

    layout            one layout for every env: row strings / char array / uint8[G,G]
                      (default: the reference's shipped layout for the variant)
    per_env_layouts   uint8[N,G,G] (numpy or torch): every env has its own maze
    env_base          global index of local env 0 when the batch is one shard of a larger
                      one (keys the reset draws; see include/lmaze.h lmaze_reset)
    obs_dtype         "int32" (default; the compact planes BASELINE's metric is quoted on) or "u8": the same LMAZE_OBS_* bit
                      mask in one byte per cell, uint8[N,G,G], 37 + G*G bytes per env-step instead of 37 + 4 G*G (shared
                      layouts, G >= 4; lmaze_step_u8 -- no launch-policy knobs; rollout() is one lmaze_rollout_u8 launch)
    online_autotune   OPT-IN (default False: the library's default launch policy, nothing timed).  True, on
                      large shared-layout batches only (the streaming regime): time the launch policies on
                      the caller's own first ~200 steps, in the caller's own loop -- after 100 untimed steps they cycle
                      through the 8 policies of ONLINE_CANDIDATES, 12 samples each, each launch bracketed by an event
                      pair; a step under a losing policy can take up to twice as long (76 against 152 us for (2, 1) at
                      1M x 11x11) -- and keep the fastest, the library default unless another beats it by more than 1.5 %
                      (see OnlineTuner; `tuning_progress()` reports where it is, `tuned_policy` the winner; one
                      log line when it starts and one when it ends); autotune() or set_launch_policy() switch it off.
                      Results never depend on the policy.
    """
    _STATS_KEYS = VecEnvBase._STATS_KEYS + ("goal_count",)

    def __init__(self, num_envs, variant="v0", layout=None, per_env_layouts=None, device=None,
                 expansion=None, step_limit=None, rewards=None, seed=0, env_base=0, validate=True,
                 online_autotune=False, obs_dtype="int32"):
        if variant not in VARIANTS:
            raise ValueError("unknown variant %r (have %s)" % (variant, sorted(VARIANTS)))
        spec = VARIANTS[variant]
        self.variant = variant
        self._init_common(num_envs, device, seed, env_base)
        self.expansion = int(expansion if expansion is not None else spec["expansion"])
        self.step_limit = int(step_limit if step_limit is not None else spec["step_limit"])
        self.rewards = tuple(float(r) for r in (rewards if rewards is not None else spec["rewards"]))
        self.channel_mask = spec["channel_mask"]
        self._is_v3 = variant == "v3"

        N = self.num_envs
        if per_env_layouts is not None:
            lay = per_env_layouts
            if not isinstance(lay, torch.Tensor):
                lay = torch.from_numpy(L.to_codes(np.asarray(lay)))
            if lay.dtype != torch.uint8 or lay.dim() != 3 or lay.shape[0] != N or lay.shape[1] != lay.shape[2]:
                raise ValueError("per_env_layouts must be uint8[N,G,G]")
            lay = lay.to(self.device).contiguous()
            if validate:
                _validate_on_device(lay, need_goal=not self._is_v3)
            self.layout_mode = _abi.LAYOUT_PER_ENV
            self.layout = lay
        else:
            codes = L.to_codes(layout if layout is not None else spec["layout"])
            if codes.ndim != 2:
                raise ValueError("layout must be [G,G]; use per_env_layouts for [N,G,G]")
            if validate:
                L.validate(codes, need_goal_marker=not self._is_v3)
            self.layout_mode = _abi.LAYOUT_SHARED
            self.layout = torch.from_numpy(codes.copy()).to(self.device)
        self.grid = int(self.layout.shape[-1])
        if not (3 <= self.grid <= _abi.MAX_GRID):
            raise ValueError("grid side must be in [3, %d]" % _abi.MAX_GRID)
        G = self.grid

        self._alloc_state([("ball_xy", torch.int32, 2), ("goal_xy", torch.int32, 2), ("step_count", torch.int32, 1),
                           ("reward", torch.float32, 1), ("goal_count", torch.int32, 1), ("done", torch.uint8, 1)])
        if obs_dtype not in ("int32", "u8"):
            raise ValueError("obs_dtype must be 'int32' or 'u8'")
        self._u8 = obs_dtype == "u8"
        if self._u8 and (self.layout_mode != _abi.LAYOUT_SHARED or G < 4):
            raise ValueError("obs_dtype='u8' needs a shared layout with G >= 4")
        self.obs = torch.zeros((N, G, G), dtype=torch.uint8 if self._u8 else torch.int32, device=self.device)
        self._expanded = None

        self.params = _abi.make_params(spec["id"], G, self.layout_mode, self.step_limit, *self.rewards)
        self._pp = C.byref(self.params)
        self._cmask = (C.c_int32 * len(self.channel_mask))(*self.channel_mask)
        self._bind_pointers()
        streaming = self.layout_mode == _abi.LAYOUT_SHARED and N * G * G * 4 > (192 << 20) and not self._u8
        self._tuner = OnlineTuner(self.ONLINE_CANDIDATES) if (online_autotune and streaming) else None
        if self._tuner is not None:
            _log.info("gym-lmaze_amd: online launch-policy tuning on for the next ~%d steps of this %d-env batch",
                      self._tuner.warm + self._tuner.samples * len(self.ONLINE_CANDIDATES), N)

        if not self._is_v3:
            # v0 looks the goal up once from the layout (lmaze_env.py:100-102): first 'X', row-major
            self._fill_goal_from_layout()
        self.reset()

    # ------------------------------------------------------------------ plumbing
    def _bind_pointers(self):
        self._p_layout = self.layout.data_ptr()
        self._p_ball = self.ball_xy.data_ptr()
        self._p_goal = self.goal_xy.data_ptr()
        self._p_step = self.step_count.data_ptr()
        self._p_reward = self.reward.data_ptr()
        self._p_done = self.done.data_ptr()
        self._p_gc = self.goal_count.data_ptr()
        self._p_obs = self.obs.data_ptr()
        self._gc_ptr = None if self._is_v3 else self._p_gc

    def _fill_goal_from_layout(self):
        G = self.grid
        flat = (self.layout.reshape(-1, G * G) == ord("X")).to(torch.int32)
        has = flat.sum(dim=1) > 0
        first = torch.argmax(flat, dim=1).to(torch.int32)
        first = torch.where(has, first, torch.full_like(first, -1))
        gx = torch.div(first, G, rounding_mode="floor")
        gy = first - gx * G
        g = torch.stack([gx, gy], dim=1).to(torch.int32)
        self.goal_xy.copy_(g.expand(self.num_envs, 2) if g.shape[0] == 1 else g)

    # ------------------------------------------------------------------ the hot path
    def step(self, actions, render=True, auto_reset=False):
        """One step() of every env.  Returns (obs, reward, done, actions): obs is the compact
        int32[N,G,G] plane buffer (rewritten in place every step), reward float32[N], done
        bool[N].  render=False skips the observation write (transition only).
        auto_reset=True first resets the envs whose done flag is still set from the previous
        step (the user loop `if done: env.reset()`), fused into the same kernel; the result is
        bit-identical to `reset(mask=done)` followed by `step(actions)`."""
        a = self._as_i32(actions, self.num_envs)
        with self._guard():
            self._launch_step(a.data_ptr(), self._p_obs if render else None, auto_reset)
        return self.obs, self.reward, self.done, actions

    def step_raw(self, action_ptr, auto_reset=False, epoch_slot=None):
        """step() on a raw device pointer to int32[N] actions (no tensor handling): for
        rollouts over a pre-generated [T,N] action tensor, e.g. under graph capture.  epoch_slot
        (auto_reset under capture): index t of the launch within the captured sequence -- the reset epoch
        then lives on the device (see begin_replay)."""
        self._launch_step(action_ptr, self._p_obs, auto_reset, epoch_slot)

    def tuning_progress(self):
        """None when no online tuning is running, else (timed launches collected, launches needed)."""
        t = self._tuner
        if t is None:
            return None
        return sum(len(v) for v in t.timings.values()), t.samples * len(t.candidates)

    def set_launch_policy(self, per_cu, chunks=1):
        """Fix the launch policy (workgroups per CU, chunks per workgroup) and stop any tuning.  On-die 8x8 batches (up
        to 192 MiB of planes, shared layout) run the wave-autonomous kernel, which reads the same two fields as waves
        per workgroup (1, 2, 4) and envs per wave (1: 64, 2: 32, 3: 16) -- include/lmaze.h, launch_hint; a value
        outside those sets means its default there.  `_abi.describe_step(env.params, N)` shows what a hint selects."""
        self.params.launch_hint = self.launch_hint_of(per_cu, chunks)
        self._tuner = None

    def _launch_step(self, action_ptr, obs_ptr, auto_reset, epoch_slot=None):
        tuner = self._tuner
        if tuner is not None and obs_ptr is not None and not torch.cuda.is_current_stream_capturing():
            cand = tuner.next_candidate()
            self._set_policy(cand)
            best = tuner.time(cand, self._launch_step_raw, action_ptr, obs_ptr, auto_reset, epoch_slot)
            if best is not None:                     # every candidate has its samples: keep the fastest
                self._set_policy(best)
                self.tuned_policy, self._tuner = best, None
                _log.info("gym-lmaze_amd: online tuning done, launch policy (workgroups per CU, chunks) = %s", best)
            return
        self._launch_step_raw(action_ptr, obs_ptr, auto_reset, epoch_slot)

    def _launch_step_raw(self, action_ptr, obs_ptr, auto_reset, epoch_slot=None):
        lib, N, st = _abi.lib, self.num_envs, self._stream()
        if self._u8:
            epoch, e_in, e_out = self._epoch_args(auto_reset, epoch_slot)
            rc = lib.lmaze_step_u8(self._pp, self._p_layout, action_ptr, self._p_ball, self._p_goal if self._is_v3 else None,
                                   self._p_step, self._p_reward, self._p_done, None if self._is_v3 else self._p_gc, obs_ptr, N,
                                   1 if auto_reset else 0, self.seed & (2 ** 64 - 1), epoch, self.env_base, e_in, e_out, st)
            _abi.check("lmaze_step_u8", rc)
            return
        if auto_reset:
            seed = self.seed & (2 ** 64 - 1)
            epoch, e_in, e_out = self._epoch_args(True, epoch_slot)
            if self._is_v3:
                rc = lib.lmaze_step_v3_autoreset(self._pp, self._p_layout, action_ptr, self._p_ball, self._p_goal,
                                                 self._p_step, self._p_reward, self._p_done, obs_ptr, N,
                                                 seed, epoch, self.env_base, e_in, e_out, st)
            else:
                rc = lib.lmaze_step_v0_autoreset(self._pp, self._p_layout, action_ptr, self._p_ball, self._p_step,
                                                 self._p_reward, self._p_done, self._p_gc, obs_ptr, N,
                                                 seed, epoch, self.env_base, e_in, e_out, st)
        elif self._is_v3:
            rc = lib.lmaze_step_v3(self._pp, self._p_layout, action_ptr, self._p_ball, self._p_goal,
                                   self._p_step, self._p_reward, self._p_done, obs_ptr, N, st)
        else:
            rc = lib.lmaze_step_v0(self._pp, self._p_layout, action_ptr, self._p_ball, self._p_step,
                                   self._p_reward, self._p_done, self._p_gc, obs_ptr, N, st)
        _abi.check("lmaze_step_" + self.variant, rc)

    def _set_policy(self, policy):
        self.params.launch_hint = self.launch_hint_of(*policy)

    def _set_obs(self, ptr):
        self._p_obs = ptr

    # launch policies autotune() tries: (workgroups per CU, chunks per workgroup) -> LmazeParams.launch_hint
    DEFAULT_POLICY = (0, 0)       # launch_hint = 0: the library's per-shape default (lmaze_step.hip step_plan)
    # a third element selects the envs per workgroup where the kernel offers a choice (11x11, 12x12: 1 = 64, 2 = 32, 3 = 16;
    # 14x14, 18x18: 1 = 32, 2 = 16; large 8x8 batches: 1 = 128, 2 = 64; 32x32: 1 = 8, 2 = 4; any other G: 1 = 256, 2 = 64,
    # 3 = 16 -- include/lmaze.h)
    CANDIDATES = ((0, 0), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2), (5, 2), (6, 2), (7, 2), (8, 1), (8, 2),
                  (6, 1, 2), (8, 1, 2), (5, 1, 2), (4, 2, 2), (3, 1, 2), (4, 1, 2), (3, 2, 2), (4, 1, 1), (3, 2, 1), (2, 1, 1), (2, 2, 1), (8, 1, 3), (5, 2, 3))

    # the online tuner's own, shorter list (it runs inside the caller's loop): the default and the pairs that have won on
    # some box for some shape (profiles/r02/shape_sweep.jsonl)
    ONLINE_CANDIDATES = ((0, 0), (3, 1), (3, 2), (5, 2), (8, 1), (6, 1, 2), (8, 2, 2), (5, 2, 2))

    @staticmethod
    def launch_hint_of(per_cu, chunks=1, epb_sel=0, no_stagger=False):
        """LmazeParams.launch_hint for `per_cu` workgroups per CU, `chunks` chunks per workgroup and, where the kernel
        offers the choice, the envs-per-workgroup selector (include/lmaze.h: bits 10-11); no_stagger: bit 9."""
        return (int(per_cu) & 15) | ((int(chunks) & 15) << 4) | ((int(epb_sel) & 3) << 10) | (0x200 if no_stagger else 0)

    def autotune(self, auto_reset=False, actions=None, steps=24, candidates=None, warm=150, between=None, rounds=3,
                 placement_trials=0):
        """Pick the launch policy (LmazeParams.launch_hint: workgroups per CU, chunks per workgroup) by
        timing real steps with HIP events (_tuning.autotune: `warm` untimed launches, `rounds` interleaved passes, the
        median counts, the library default (0, 0) kept unless beaten by more than 1.5 %); the state is snapshotted and
        restored, so results are unaffected.  The optimum is narrow and depends on shape, device and -- most of all -- on
        WHERE THE INPUTS COME FROM: the policy that wins when actions and state sit in the Infinity Cache (3 workgroups
        per CU) loses a third of its rate when the actions are a fresh row from HBM every step (lmaze_step.hip
        step_plan).  So pass the action tensor the rollout will use (`actions`: int32[T,N] on the
        device; the rows are cycled exactly as rollout() would); without one, a private ring of rows larger
        than the cache is generated, the conservative assumption.  `between`: a callable that enqueues, on the
        current stream, whatever runs between two steps in the real loop (the policy's forward pass): back to
        back, consecutive step launches overlap head to tail and find their state in the cache, and 3
        workgroups per CU win; with half a gigabyte of other traffic in between, that policy took 115 us per
        step instead of 86 and 8 per CU took 93 (tools/evict_study.py) -- then each step is timed on its
        own with an event pair and the median counts.
        placement_trials=K (K > 1): the step is first timed with the (5, 2) policy on K - 1 further allocations of the
        observation buffer, and the fastest becomes the storage of `self.obs` (the same tensor object).  Where the driver
        placed the 500-MB write target is worth 3-5 % at the default policy and up to 20 % under a capped one.  Round 3
        measured what differs (tools/placement_pmc.py under rocprofv3 --pmc, LAB_NOTES.md R3.2): NOT address translation
        (UTCL1 misses 0.06 % of requests on fast and slow buffers alike) but the memory side -- 25 % more DRAM
        write-credit stall cycles (TCC_EA0_WRREQ_DRAM_CREDIT_STALL) on the slow allocations, i.e. which channels / banks
        the buffer's physical pages load; a 2-MiB-aligned arena shows the same spread.  `self.placement` records the
        trial times and, under the policy finally chosen, the first allocation's time beside the kept one's (bench.py:
        roofline.frac_first_allocation).
        Returns {(per_cu, chunks): ms per step}.  Only the shared-layout kernel has these knobs."""
        obs_bytes = self.num_envs * self.grid * self.grid * 4
        if self.layout_mode != _abi.LAYOUT_SHARED or obs_bytes <= (192 << 20) or self._u8:
            return {}       # the knobs only pay in the streaming (non-temporal store) regime; the u8 kernel has none
        cands = [tuple(c) if isinstance(c, (tuple, list)) else (int(c), 1) for c in (candidates or self.CANDIDATES)]
        N = self.num_envs
        if actions is None:
            rows = max(2, min(512, (320 << 20) // (4 * N) + 1))          # > 256 MiB of action rows
            actions = torch.randint(0, 4, (rows, N), dtype=torch.int32, device=self.device)
        self._check_rows("autotune(actions=...)", actions)
        base, stride = actions.data_ptr(), N * 4
        # an explicit autotune replaces the online tuner, which its launches bypass
        timings = self._tune(int(actions.shape[0]),
                             lambda r: self._launch_step_raw(base + r * stride, self._p_obs, auto_reset),
                             candidates=cands, default=self.DEFAULT_POLICY, trial_policy=(5, 2), steps=steps, warm=warm,
                             rounds=rounds, placement_trials=placement_trials, between=between)
        self._tuner = None
        self.observe()
        return timings

    def rollout(self, actions, auto_reset=True, device_epoch=False, trajectory=False, obs_t=None, obs_every=None):
        """T steps over a device tensor int32[T,N] of actions, one kernel per step, no host
        sync (capture_rollout() records it into a hipGraph for launch-bound batch sizes).
        device_epoch: keep the reset epoch on the device (what capture_rollout uses; bit-identical to the
        host-counted epochs when begin_replay(T) precedes it).  Returns the final (obs, reward, done); trajectory=True adds
        every step's reward float32[T,N] and done bool[T,N].  The whole rollout is ONE launch (shared and per-env
        layouts, any batch size; the envs' state stays in registers across the T steps) (include/lmaze.h
        lmaze_rollout; the u8 env: lmaze_rollout_u8).  With device_epoch it is T step launches.
        obs_every=k >= 1 records observations into the caller's obs_t, shaped (T // k, N, G, G) with obs's dtype: slot j
        is what obs holds after step (j + 1) k - 1 (lmaze_rollout_obs / lmaze_rollout_obs_u8, still one launch; the u8
        env's slots may have any N).  obs_every=0 stores the final planes only (obs_t None).  Steps that fill no slot
        store no planes; the final obs, state, rows and epoch are those of the plain rollout.  Not with device_epoch, nor
        while the online tuner runs."""
        self._check_rows("rollout()", actions)
        base, stride = actions.data_ptr(), self.num_envs * 4
        T, N = int(actions.shape[0]), self.num_envs
        k = None
        if obs_every is not None:
            if device_epoch or self._tuner is not None:
                raise ValueError("rollout(obs_every=...) is not available with a device-resident epoch or while the online tuner runs")
            k = self._obs_slots(T, obs_every, obs_t, self.obs, allow_final=True)
        elif obs_t is not None:
            raise ValueError("obs_t needs obs_every")
        if not device_epoch and self._tuner is None:
            # lmaze_rollout (the u8 env: lmaze_rollout_u8): ONE launch (the envs' state stays in registers across the T
            # steps); bit-identical to T step() calls
            rows = self._traj_rows(T) if trajectory else None
            args = (self._pp, self._p_layout, base, T, self._p_ball, self._p_goal if self._is_v3 else None, self._p_step,
                    self._p_reward, self._p_done, None if self._is_v3 else self._p_gc, self._p_obs,
                    rows[0].data_ptr() if rows else None, rows[1].data_ptr() if rows else None,
                    N, 1 if auto_reset else 0, self.seed & (2 ** 64 - 1), self._epoch, self.env_base)
            name = ("lmaze_rollout" if k is None else "lmaze_rollout_obs") + ("_u8" if self._u8 else "")
            with self._guard():
                if k is None:
                    rc = getattr(_abi.lib, name)(*args, self._stream())
                else:
                    slots = obs_t.data_ptr() if k > 0 and obs_t.shape[0] > 0 else None
                    rc = getattr(_abi.lib, name)(*args, slots, k, self._stream())
            _abi.check(name, rc)
            if auto_reset:
                self._epoch += T
            return self._rollout_result(rows)
        if trajectory:
            raise ValueError("rollout(trajectory=True) is not available with a device-resident epoch or while the online tuner runs")
        with self._guard():
            for t in range(actions.shape[0]):
                self._launch_step(base + t * stride, self._p_obs, auto_reset, t if device_epoch else None)
        return self.obs, self.reward, self.done

    def rollout_policy(self, T, policy=None, q=None, epsilon=0.0, key="ball", auto_reset=True, trajectory=False,
                       actions_t=None, key_t=None, obs_t=None, obs_every=0):
        """T steps in ONE launch with a tabular epsilon-greedy policy inside the kernel (include/lmaze.h
        lmaze_rollout_policy; the u8 env: lmaze_rollout_policy_u8): no action tensor, no per-step launches.
        policy   uint8 device tensor, the greedy action id of every key: G*G entries for key="ball" (the ball's row-major
                 cell, ball_x * G + ball_y), G**4 for key="goal" (v3: goal cell * G*G + ball cell).  Ids above 3 are no move.
        q        instead of policy: a float tensor [S, A] of action values, reduced on the device by greedy_table().
        epsilon  exploration rate in [0, 1]: with that probability (in steps of 2**-32) the step takes a uniform action 0-3,
                 drawn by Philox from (seed, env, epoch); 0 draws nothing.
        key="env"  a table PER ENV (lmaze_env_rollout_policy; int32 planes, shared and per-env layouts): policy uint8
                 [N, G*G] or flat [N*G*G], q float [N, G*G, A] or [N*G*G, A] -- what solve() returns on per-env layouts, or
                 a population of policies on one maze.  Row i * G*G + ball cell, which is also what key_t holds, so
                 gae(values=v.reshape(-1), key_t=..., key_tail=state_keys("env")) and table_stats(keys=N*G*G) take the rows
                 as they are.  i is this env object's own index 0 <= i < N (a shard's local index, not env_base + i).  v3:
                 the table is keyed by the ball cell alone and a fused reset re-draws the goal, so tables solved for the
                 current goals are stale after a reset: use auto_reset=False, or goal-free tables (v0's goal is the layout's
                 'X' and does not move).
        Returns what rollout() returns -- the final (obs, reward, done), with trajectory=True also reward float32[T,N] and
        done bool[T,N] -- and then, with trajectory=True, actions_t and key_t int32[T,N] (the caller's, or allocated).
        obs_every=k >= 1 records into obs_t as rollout() does; the default 0 stores the final planes only.  The epoch
        advances by T whether or not auto_reset is set: exploration consumes epochs too.  Not with a device-resident epoch
        (under stream capture: the host's epoch would be frozen into the graph), nor while the online tuner runs."""
        T, entries = self._closed_loop_key("rollout_policy()", T, key)
        _tables.exactly_one("rollout_policy()", policy=policy, q=q)
        if key == "env":
            N, S = self.num_envs, self.grid ** 2
            if isinstance(q, torch.Tensor) and q.dim() == 3 and tuple(q.shape[:2]) == (N, S):
                q = q.reshape(N * S, q.shape[2])
            if isinstance(policy, torch.Tensor) and tuple(policy.shape) not in ((N, S), (N * S,)):
                raise ValueError("policy must be uint8 [%d, %d] or flat [%d] (key='env')" % (N, S, N * S))
            policy = _tables.greedy_policy(policy, q, entries, self.device, "key='env', N=%d, G=%d" % (N, self.grid))
            if policy.data_ptr() % 4:
                raise ValueError("policy must be 4-byte aligned (key='env')")
            return self._rollout_table("env_rollout_policy", (policy.data_ptr(), _abi.epsilon_u32(epsilon)), T, auto_reset,
                                       trajectory, actions_t, key_t, obs_t, obs_every)
        policy = _tables.greedy_policy(policy, q, entries, self.device, "key=%r, G=%d" % (key, self.grid))
        return self._rollout_table("rollout_policy", (policy.data_ptr(), _abi.KEY_MODES[key], _abi.epsilon_u32(epsilon)), T,
                                   auto_reset, trajectory, actions_t, key_t, obs_t, obs_every)

    def rollout_sample(self, T, probs=None, logits=None, temperature=1.0, thresholds=None, key="ball", auto_reset=True,
                       trajectory=False, actions_t=None, key_t=None, obs_t=None, obs_every=0):
        """T steps in ONE launch with a categorical table policy inside the kernel (include/lmaze.h lmaze_rollout_sample;
        the u8 env: lmaze_rollout_sample_u8): every env-step draws its action from the distribution of its key.  Exactly
        one of
        probs       float device tensor [S, 4] of non-negative weights, converted by _abi.sampling_thresholds();
        logits      float device tensor [S, 4]: sampling_thresholds(softmax(logits.double() / temperature)), temperature > 0
                    (a Boltzmann policy);
        thresholds  the table itself, uint32 (or int32, the same bits) device tensor [S, 4], contiguous and 16-byte
                    aligned: cumulative thresholds c0 <= c1 <= c2 and a reserved word per key.
        S = G*G for key="ball" (ball_x * G + ball_y), G**4 for key="goal" (v3: goal cell * G*G + ball cell).  The action is
        (r >= c0) + (r >= c1) + (r >= c2) for one Philox value r per (seed, env, epoch); a cumulative probability of 1 is
        stored as 1 - 2**-32, so deterministic policies belong to rollout_policy().  Returns what rollout_policy() returns;
        obs_t / obs_every, the rows and the restrictions are its own too.  The epoch advances by T.
        key="env": a table PER ENV (lmaze_env_rollout_sample), rows [N, G*G, 4] or flat [N*G*G, 4], row i * G*G + ball cell;
        key_t, the index i and the note on v3 and the fused reset as in rollout_policy(key="env")."""
        T, entries = self._closed_loop_key("rollout_sample()", T, key)
        G = self.grid
        _tables.exactly_one("rollout_sample()", probs=probs, logits=logits, thresholds=thresholds)
        if key == "env":                               # contiguous rows [N, G*G, 4] are the flat table's own memory
            def flat(t):
                whole = isinstance(t, torch.Tensor) and tuple(t.shape) == (self.num_envs, G * G, 4) and t.is_contiguous()
                return t.view(entries, 4) if whole else t
            probs, logits, thresholds = flat(probs), flat(logits), flat(thresholds)
        thresholds = _tables.threshold_table(probs, logits, thresholds, temperature, entries, 4, self.device,
                                             "key=%r, G=%d" % (key, G))
        table_args = (thresholds.data_ptr(),) if key == "env" else (thresholds.data_ptr(), _abi.KEY_MODES[key])
        return self._rollout_table("env_rollout_sample" if key == "env" else "rollout_sample", table_args, T, auto_reset, trajectory,
                                   actions_t, key_t, obs_t, obs_every)

    def rollout_qlearn(self, T, q, alpha=0.1, gamma=0.99, epsilon=0.1, auto_reset=True, trajectory=True, td_t=None,
                       actions_t=None, key_t=None, obs_t=None, obs_every=0):
        """T steps of tabular Q-LEARNING in ONE launch, a learner per env (include/lmaze.h lmaze_env_rollout_qlearn): every
        env acts epsilon-greedily on its own table of action values, steps, and updates the table from the transition.
        q        float32 device tensor [N, G*G, 4] or flat [N*G*G, 4], contiguous and 16-byte aligned, UPDATED IN PLACE and
                 never copied (anything else is a ValueError: a silent copy would lose the update).  Row i * G*G + ball
                 cell, i this env object's own index, as rollout_policy(key="env").
        alpha, gamma  step size and discount, rounded to float32; not validated.
        epsilon  exploration rate in [0, 1], as rollout_policy()'s.
        td_t     optional float32 [T, N] device tensor, filled with every step's TD error.
        Per env-step: the greedy action is the FIRST maximum of the row (solve()'s rule), epsilon mixes in a uniform action
        by rollout_policy()'s draw, the step is step()'s, and q[c, a] += alpha * (target - q[c, a]) with target = reward
        when the step returned done (the step limit counts), else reward + gamma * max q[c'] read before the write; float32,
        every operation rounded on its own, so a numpy loop reproduces the table bit for bit.
        Returns what rollout_policy(key="env") returns: (obs, reward, done) and, with trajectory=True (the default here),
        reward_t, done_t, actions_t, key_t.  Its refusals too: not the u8 env, not under stream capture, not while the
        online tuner runs, N * G*G <= 2**31 - 1.  The epoch advances by T.
        What composes with it: solve() gives the table it converges towards (v0; and a v_init-style warm start goes the
        other way: q.max(-1) of a learnt table starts solve()); rollout_policy(q=q, key="env") runs the learnt table
        without learning; state_keys("env") / gae(values=..., key_t=...) / table_stats(keys=N*G*G) take its rows as they
        are.  v3: the key is the ball cell alone and a fused reset re-draws the goal, so with auto_reset what is learnt is
        goal-free."""
        T, entries = self._closed_loop_key("rollout_qlearn()", T, "env")
        N, S = self.num_envs, self.grid ** 2
        if not (isinstance(q, torch.Tensor) and q.dtype == torch.float32 and q.device == self.device and q.is_contiguous()
                and tuple(q.shape) in ((N, S, 4), (entries, 4)) and q.data_ptr() % 16 == 0):
            raise ValueError("q must be a contiguous, 16-byte aligned float32 tensor [%d, %d, 4] or [%d, 4] on %s: it is updated "
                             "in place" % (N, S, entries, self.device))
        if td_t is not None and not (isinstance(td_t, torch.Tensor) and td_t.dtype == torch.float32 and td_t.device == self.device
                                     and td_t.is_contiguous() and tuple(td_t.shape) == (T, N)):
            raise ValueError("td_t must be a contiguous float32 tensor [%d, %d] on %s" % (T, N, self.device))
        table_args = (q.data_ptr(), C.c_float(float(alpha)), C.c_float(float(gamma)), _abi.epsilon_u32(epsilon))
        return self._rollout_table("env_rollout_qlearn", table_args, T, auto_reset, trajectory, actions_t, key_t, obs_t, obs_every,
                                   after_rows=(None if td_t is None else td_t.data_ptr(),))

    def _closed_loop_key(self, who, T, key):
        """What rollout_policy() and rollout_sample() refuse before they look at their table; returns T as an int and the
        number of keys, i.e. of table rows."""
        if self._tuner is not None or torch.cuda.is_current_stream_capturing():
            raise ValueError("%s is not available with a device-resident epoch or while the online tuner runs" % who)
        T = self._steps(T)
        if key == "env":
            if self._u8:
                raise ValueError("key='env' needs the int32 planes: the u8 env has no rollout with a table per env")
            if self.num_envs * self.grid ** 2 > 2 ** 31 - 1:
                raise ValueError("key='env' needs N * G*G <= 2**31 - 1: the key is an int32 row")
            return T, self.num_envs * self.grid ** 2
        if key not in _abi.KEY_MODES:
            raise ValueError("key must be 'ball', 'goal' or 'env'")
        if key == "goal" and not self._is_v3:
            raise ValueError("key='goal' needs the v3 variant: v0 keeps no per-env goal")
        return T, self.grid ** 4 if key == "goal" else self.grid ** 2

    def _rollout_table(self, method, table_args, T, auto_reset, trajectory, actions_t, key_t, obs_t, obs_every, after_rows=()):
        """The launch of rollout_policy() / rollout_sample(): lmaze_<method> or, for the u8 env, lmaze_<method>_u8, which
        differ in table_args alone -- (table, key_mode, epsilon_u32) or (table, key_mode); key="env", lmaze_env_<method>:
        (table, epsilon_u32) or (table,); rollout_qlearn(): (q, alpha, gamma, epsilon_u32) and after_rows = (td_t,), the row
        addresses that follow key_t's."""
        name = "lmaze_" + method + ("_u8" if self._u8 else "")
        k = self._obs_slots(T, obs_every, obs_t, self.obs, allow_final=True)

        def call(rows, p_actions, p_key, slots):
            return getattr(_abi.lib, name)(
                self._pp, self._p_layout, *table_args, T, self._p_ball, self._p_goal if self._is_v3 else None, self._p_step,
                self._p_reward, self._p_done, None if self._is_v3 else self._p_gc, self._p_obs, *(rows or (None, None)),
                p_actions, p_key, *after_rows, self.num_envs, 1 if auto_reset else 0, self.seed & (2 ** 64 - 1), self._epoch, self.env_base,
                slots, k, self._stream())
        return self._closed_loop(method + "()", name, call, T, k, obs_t, trajectory, actions_t, key_t)

    def observe(self, mask_ptr=None):
        """Re-render the compact planes of the current state (no transition)."""
        if self._u8:
            with self._guard():
                rc = _abi.lib.lmaze_observe_u8(self._pp, self._p_layout, self._p_ball, self._p_goal if self._is_v3 else None,
                                               mask_ptr, self._p_obs, self.num_envs, self._stream())
            _abi.check("lmaze_observe_u8", rc)
            return self.obs
        with self._guard():
            rc = _abi.lib.lmaze_observe(self._pp, self._p_layout, self._p_ball,
                                        self._p_goal if self._is_v3 else None, self._p_obs,
                                        self.num_envs, self._stream())
        _abi.check("lmaze_observe", rc)
        return self.obs

    def _start_table(self, start, thresholds, key, keep_goal, validate):
        """reset()'s law as the table lmaze_reset_start reads, uint32[rows, G*G].  The refusals stand in this order: both of
        start / thresholds, the shape key asks for, key="goal" on v0 (and on per-env layouts), keep_goal on v0, and with
        validate a row of the caller's thresholds that decreases or neither ends in 2**31 nor is all zero."""
        name = _tables.exactly_one("reset()", start=start, thresholds=thresholds)
        if key not in _abi.ROW_MODES:
            raise ValueError("key must be 'ball', 'goal' or 'env'")
        S, N = self.grid ** 2, self.num_envs
        shapes = {"ball": ((1, S), (S,)), "goal": ((S, S),), "env": ((N, S),)}[key]
        table = start if name == "start" else thresholds
        kinds = "a float" if name == "start" else "a contiguous uint32 (or int32)"
        ok = isinstance(table, torch.Tensor) and table.device == self.device and tuple(table.shape) in shapes
        if ok and name == "start":
            ok = table.is_floating_point()
        elif ok:
            ok = table.dtype in (torch.uint32, torch.int32) and table.is_contiguous()
        if not ok:
            raise ValueError("%s must be %s tensor %s on %s (key=%r)" % (name, kinds, " or ".join(str(list(s)) for s in shapes),
                                                                        self.device, key))
        if key == "goal" and not self._is_v3:
            raise ValueError("key='goal' needs the v3 variant: v0 keeps no per-env goal")
        if key == "goal" and self.layout_mode != _abi.LAYOUT_SHARED:
            raise ValueError("key='goal' draws from one table of goal rows on a shared layout; per-env layouts take key='env'")
        if keep_goal and not self._is_v3:
            raise ValueError("keep_goal needs the v3 variant: v0 keeps no per-env goal")
        if name == "start":
            return start_thresholds(table.reshape(-1, S))
        if validate:
            w = table.reshape(-1, S).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            if bool((w[:, 1:] < w[:, :-1]).any()):
                raise ValueError("a row of thresholds decreases")
            if not bool(((w[:, -1] == 2 ** 31) | (w == 0).all(1)).all()):
                raise ValueError("a row of thresholds neither ends in 2**31 nor is all zero")
        return table

    def reset(self, mask=None, seed=None, *, start=None, thresholds=None, key="ball", keep_goal=False, validate=True):
        """Masked on-device reset (mask: bool/uint8[N], None = all).  Returns the compact obs.
        With neither start nor thresholds: lmaze_reset's uniform law (reset_distribution()).  With exactly one of them the
        ball is drawn from a law the caller gives, in one placement launch (include/lmaze.h lmaze_reset_start), from the
        same draw of (seed, epoch, env_base + i) -- the v3 goal is lmaze_reset's own, or kept with keep_goal=True:
        start       float weights, non-negative, a row need not sum to 1: what occupancy(start=...) takes and
                    distance_band() makes; turned into thresholds by start_thresholds().  A row of zeros: the ball stays.
        thresholds  the table itself, uint32 (or int32, the same bits): the caller's memory, never copied.  validate=False
                    skips the check of its rows (a device synchronisation).
        key         "ball": one row for every env, [1, G*G] or [G*G]; "goal": v3 on a shared layout, [G*G, G*G], the row of
                    the env's goal cell; "env": [N, G*G], row i for env i of this object, on shared or per-env layouts.
        The cell is not excluded for being a wall or the goal.  The fused resets of step(auto_reset=True) and of the
        rollouts keep the uniform law: a curriculum runs auto_reset=False and resets the done envs between launches.  Not
        for captured graphs."""
        table = None
        if start is not None or thresholds is not None:
            table = self._start_table(start, thresholds, key, keep_goal, validate)
        elif keep_goal:
            raise ValueError("keep_goal belongs to a reset from start= or thresholds=")
        if seed is not None:
            self.seed = int(seed)
            self._epoch = 0
        m, m_ptr = self._mask_ptr(mask)
        if table is not None:
            with self._guard():
                rc = _abi.lib.lmaze_reset_start(self._pp, self._p_layout, m_ptr, table.data_ptr(), _abi.ROW_MODES[key],
                                                1 if keep_goal else 0, self.seed & (2 ** 64 - 1), self._epoch, self.env_base,
                                                self._p_ball, self._p_goal if self._is_v3 else None, self._p_step,
                                                self._p_reward, self._p_done, None if self._u8 else self._p_obs,
                                                self.num_envs, self._stream())
            _abi.check("lmaze_reset_start", rc)
        else:
            with self._guard():
                rc = _abi.lib.lmaze_reset(self._pp, self._p_layout, m_ptr, self.seed & (2 ** 64 - 1), self._epoch,
                                          self.env_base, self._p_ball, self._p_goal if self._is_v3 else None,
                                          self._p_step, self._p_reward, self._p_done, None if self._u8 else self._p_obs,
                                          self.num_envs, self._stream())
            _abi.check("lmaze_reset", rc)
        self._epoch += 1
        if self._u8:
            self.observe(mask_ptr=m_ptr)       # the narrow planes of the envs that were reset
        return self.obs

    def set_state(self, ball_xy=None, goal_xy=None, step_count=None, reward=None, goal_count=None, done=None):
        """Inject state (placement chosen by the caller, e.g. the reference's own RNG stream)."""
        for name, src in (("ball_xy", ball_xy), ("goal_xy", goal_xy), ("step_count", step_count), ("reward", reward),
                          ("goal_count", goal_count), ("done", done)):
            if src is not None:
                self._write_state(name, src)

    def expanded(self, out=None):
        """Reference-layout observation float32[N,C,G*E,G*E] of the current compact planes
        (the upsample loop of lmaze_env.py:217-234)."""
        N, G, E, Cn = self.num_envs, self.grid, self.expansion, len(self.channel_mask)
        if out is None:
            if self._expanded is None:
                self._expanded = torch.empty((N, Cn, G * E, G * E), dtype=torch.float32, device=self.device)
            out = self._expanded
        src = self.obs.to(torch.int32) if self._u8 else self.obs      # the x E render reads int32 planes
        with self._guard():
            rc = _abi.lib.lmaze_render_expanded(src.data_ptr(), G, E, self._cmask, Cn, out.data_ptr(), N,
                                                self._stream())
        _abi.check("lmaze_render_expanded", rc)
        return out

    def state_keys(self, key="ball"):
        """int32[N]: the key of every env's CURRENT state, by the rule the key_t rows of rollout_policy() / rollout_sample()
        are written with -- coordinates clamped onto the grid, ball_x * G + ball_y, and for key="goal" (v3 only) goal cell
        * G*G + ball cell; for key="env" (rollout_policy(key="env")) i * G*G + ball cell of env i, this object's own index.
        Right after a rollout this is gae()'s key_tail.  Plain torch ops on ball_xy / goal_xy."""
        if key != "env" and key not in _abi.KEY_MODES:
            raise ValueError("key must be 'ball' or 'goal'")
        if key == "goal" and not self._is_v3:
            raise ValueError("key='goal' needs the v3 variant: v0 keeps no per-env goal")
        G = self.grid
        b = self.ball_xy.clamp(0, G - 1)
        k = b[:, 0] * G + b[:, 1]
        if key == "env":
            if self.num_envs * G * G > 2 ** 31 - 1:
                raise ValueError("key='env' needs N * G*G <= 2**31 - 1: the key is an int32 row")
            k = k + torch.arange(self.num_envs, dtype=k.dtype, device=k.device) * (G * G)
        if key == "goal":
            g = self.goal_xy.clamp(0, G - 1)
            k = k + (g[:, 0] * G + g[:, 1]) * (G * G)
        return k.to(torch.int32).contiguous()

    def _problem_key(self, key, env_ok=True):
        """What solve(), score() and evaluate() ask of key before anything of their own."""
        if key not in ("ball", "goal") + (("env",) if env_ok else ()):
            raise ValueError("key must be 'ball', 'goal' or 'env'" if env_ok else "key must be 'ball' or 'goal'")
        if key == "goal" and not self._is_v3:
            raise ValueError("key='goal' needs the v3 variant: v0 keeps no per-env goal")

    def _problems(self, who, key, goal):
        """The problems `who` ("solve", "score", "evaluate") runs for a judged key: (goals, P, single).  One problem on a shared
        layout with key="ball" (single; v3 takes its goal from goal=), G*G with key="goal", one per goal cell in row-major order,
        else N, v3 with each env's current goal.  goals is int32[P, 2] on v3 and None on v0."""
        G, S, dev = self.grid, self.grid * self.grid, self.device
        shared = self.layout_mode == _abi.LAYOUT_SHARED
        if goal is not None and not (shared and key == "ball" and self._is_v3):
            raise ValueError("goal= belongs to key='ball' on a shared-layout v3 env")
        if not shared and key == "goal":
            raise ValueError("key='goal' %ss one shared layout for every goal cell; per-env layouts %s each env's own goal" % (who, who))
        single = shared and key == "ball"
        P = 1 if single else (S if key == "goal" else self.num_envs)
        goals = None
        if self._is_v3:
            if single:
                if goal is None or len(goal) != 2:
                    raise ValueError("%s(key='ball') on a shared-layout v3 env needs goal=(x, y)" % who)
                goals = torch.tensor([[int(goal[0]), int(goal[1])]], dtype=torch.int32, device=dev)
            elif key == "goal":
                cells = torch.arange(S, dtype=torch.int32, device=dev)
                goals = torch.stack([torch.div(cells, G, rounding_mode="floor"), cells % G], dim=1).to(torch.int32).contiguous()
            else:
                goals = self.goal_xy
        return goals, P, single

    def solve(self, gamma=0.99, sweeps=4096, key="ball", rewards=None, v_init=None, goal=None):
        """Value iteration on this env's own maze(s), in ONE launch (solve_tables(), include/lmaze.h lmaze_solve): the
        tables rollout_policy(q=...), rollout_sample(logits=...) and gae(values=...) take.  It reads no planes, so the u8
        env solves as well.  rewards defaults to the env's.
        shared layout, key="ball"   one problem: q float32[G*G, 4], v float32[G*G], policy uint8[G*G], sweeps_run and delta
                                    0-d.  v3 needs goal=(x, y): a shared-layout v3 env has no single goal.
        shared layout, key="goal"   v3 only: G*G problems, one per goal cell in row-major order; q [G**4, 4], v [G**4],
                                    policy [G**4], indexed by the key of state_keys("goal"); sweeps_run, delta [G*G].
        per-env layouts             N problems, env i's layout and (v3) its current goal_xy: q [N, G*G, 4], ... -- the tables
                                    rollout_policy(q=..., key="env") / rollout_sample(logits=..., key="env") run.
        v_init: float32 [problems, G*G].  Returns SolvedTables(q, v, policy, sweeps_run, delta)."""
        self._problem_key(key, env_ok=False)
        goals, _, single = self._problems("solve", key, goal)
        t = solve_tables(self.layout, self.variant, goals=goals, gamma=gamma, sweeps=sweeps,
                         rewards=self.rewards if rewards is None else rewards, v_init=v_init, validate=False)
        return _unbatch(t, key, single, ("sweeps_run", "delta"))

    def score(self, policy=None, q=None, key="ball", goal=None):
        """How good tables are on this env's own maze(s), in ONE launch (score_tables(), include/lmaze.h lmaze_score): from
        every cell the fewest steps to done, the steps the table's greedy walk takes (-1: it never arrives), and per problem
        the counts (reachable, arrived, shortest, excess).  The problems are chosen as solve() chooses them; the rewards are
        the env's.  policy uint8 or q float32 (first maximum), at most one; neither: distances only, steps is None.
        shared layout, key="ball"   one problem: policy [G*G] / q [G*G, 4]; optimal, steps int32[G*G], summary int32[4].  v3
                                    needs goal=(x, y).
        shared layout, key="goal"   v3 only: G*G problems, one per goal cell; policy [G**4] / q [G**4, 4] indexed by the key of
                                    state_keys("goal"); optimal, steps [G**4], summary [G*G, 4].
        shared layout, key="env"    N tables on the one maze, v3 with env i's current goal: policy [N, G*G] / q [N, G*G, 4];
                                    optimal, steps [N, G*G], summary [N, 4].
        per-env layouts             env i's maze and (v3) its current goal, tables [N, G*G] / [N, G*G, 4]: what solve() returns
                                    and rollout_qlearn() updates; outputs as key="env".
        Returns ScoredTables(optimal, steps, summary)."""
        self._problem_key(key)
        if policy is not None and q is not None:
            raise ValueError("give policy= or q=, not both")
        goals, P, single = self._problems("score", key, goal)
        S, shared = self.grid * self.grid, self.layout_mode == _abi.LAYOUT_SHARED
        table = policy if policy is not None else q
        if table is not None:
            if not isinstance(table, torch.Tensor) or table.numel() != P * S * (1 if policy is not None else 4):
                raise ValueError("the table must be a tensor of %d problems x %d states%s" % (P, S, "" if policy is not None else " x 4"))
            table = table.reshape((P, S) if policy is not None else (P, S, 4))
        outputs = SCORE_OUTPUTS if table is not None else ("optimal", "summary")
        if shared and key == "env" and table is None and not self._is_v3:
            raise ValueError("key='env' on a shared v0 layout scores N tables on one maze: without a table use key='ball'")
        t = score_tables(self.layout, policy=table if policy is not None else None, q=table if q is not None else None,
                         variant=self.variant, goals=goals, rewards=self.rewards, outputs=outputs, validate=False)
        return _unbatch(t, key, single, ("summary",))

    def evaluate(self, policy=None, q=None, epsilon=0.0, probs=None, logits=None, temperature=1.0, thresholds=None, key="ball",
                 goal=None, gamma=0.99, sweeps=4096, tol=0.0, v_init=None):
        """What the table a closed-loop rollout runs is WORTH on this env's own maze(s), exactly, in ONE launch
        (evaluate_tables(), include/lmaze.h lmaze_evaluate): Q^pi and V^pi of the epsilon-greedy policy rollout_policy() runs
        (policy= or q=, with epsilon=) or of the categorical one rollout_sample() runs (probs=, logits= with temperature=, or
        thresholds=); exactly one table.  The problems are chosen as score() chooses them; the rewards are the env's.
        shared layout, key="ball"   one problem: policy [G*G], the others [G*G, 4]; q float32[G*G, 4], v float32[G*G],
                                    sweeps_run and delta 0-d.  v3 needs goal=(x, y).
        shared layout, key="goal"   v3 only: G*G problems, one per goal cell; policy [G**4], the others [G**4, 4], indexed by
                                    the key of state_keys("goal"); q [G**4, 4], v [G**4], sweeps_run, delta [G*G].
        shared layout, key="env"    N tables on the one maze, v3 with env i's current goal: policy [N, G*G], the others
                                    [N, G*G, 4]; q [N, G*G, 4], v [N, G*G], sweeps_run, delta [N].
        per-env layouts             env i's maze and (v3) its current goal; tables and outputs as key="env".  v.reshape(-1)
                                    is the critic gae(values=, key_t=, key_tail=state_keys("env")) takes.
        v_init: float32 [problems, G*G].  Returns EvaluatedTables(q, v, sweeps_run, delta)."""
        self._problem_key(key)
        tables = {"policy": policy, "q": q, "probs": probs, "logits": logits, "thresholds": thresholds}
        name = _tables.exactly_one("evaluate()", **tables)
        goals, P, single = self._problems("evaluate", key, goal)
        S = self.grid * self.grid
        table = tables[name]
        width = 1 if name == "policy" else 4
        if not isinstance(table, torch.Tensor) or table.numel() != P * S * width:
            raise ValueError("%s must be a tensor of %d problems x %d states%s" % (name, P, S, "" if width == 1 else " x 4"))
        tables[name] = table.reshape((P, S) if width == 1 else (P, S, 4))
        if isinstance(v_init, torch.Tensor) and v_init.numel() == P * S:      # what evaluate() and solve() return: [G*G], [G**4]
            v_init = v_init.reshape(P, S)
        t = evaluate_tables(self.layout, epsilon=epsilon, temperature=temperature, variant=self.variant, goals=goals, gamma=gamma,
                            sweeps=sweeps, tol=tol, rewards=self.rewards, v_init=v_init, validate=False, **tables)
        return _unbatch(t, key, single, ("sweeps_run", "delta"))

    def _occupancy_start(self, start, key, goals, P, single):
        """occupancy()'s start as float32[P, G*G]: "reset", "state" (refused for key="goal") or a tensor of that many elements"""
        if not isinstance(start, torch.Tensor):
            if start not in ("reset", "state"):
                raise ValueError("start must be 'reset', 'state' or a tensor")
            if start == "state" and key == "goal":
                raise ValueError("start='state' has no meaning for key='goal': its problems are goal cells, not envs")
        S = self.grid * self.grid
        if isinstance(start, torch.Tensor):
            if start.numel() != P * S:
                raise ValueError("start must be a float32 tensor of %d problems x %d states" % (P, S))
            return start.reshape(P, S)
        if start == "reset":
            start = reset_distribution(self.layout, self.variant, goals)
            return start if start.shape[0] == P else start.expand(P, S).contiguous()
        cells = self.state_keys("ball").long()
        if single:                                   # the envs' histogram on the one problem
            return (torch.bincount(cells, minlength=S).to(torch.float32) / float(self.num_envs)).reshape(1, S)
        start = torch.zeros((P, S), dtype=torch.float32, device=self.device)
        start[torch.arange(P, device=self.device), cells] = 1.0
        return start

    def occupancy(self, policy=None, q=None, epsilon=0.0, probs=None, logits=None, temperature=1.0, thresholds=None, key="ball",
                  goal=None, start="reset", gamma=0.99, sweeps=4096, tol=0.0, d_init=None):
        """WHERE the table a closed-loop rollout runs spends its discounted time on this env's own maze(s), exactly, in ONE
        launch (occupancy_tables(), include/lmaze.h lmaze_occupancy): evaluate()'s adjoint.  The table inputs, the problems
        (key=, goal=) and the shapes are evaluate()'s; d is shaped like its v and d_sa like its q.
        start  "reset": reset_distribution(), the law of the cell reset() places the ball on;
               "state": the envs' current ball cells -- one-hot per problem where the problems are the envs (key="env", per-env
               layouts), their histogram / N on the one problem of a shared layout with key="ball"; refused for key="goal";
               or a float32 tensor shaped like evaluate()'s v.
        With evaluate() of the same table, (start * v).sum(-1) = (d_sa * r).sum() is the expected return.
        d_init: float32 [problems, G*G].  Returns OccupancyTables(d, d_sa, sweeps_run, delta)."""
        self._problem_key(key)
        tables = {"policy": policy, "q": q, "probs": probs, "logits": logits, "thresholds": thresholds}
        name = _tables.exactly_one("occupancy()", **tables)
        goals, P, single = self._problems("occupancy", key, goal)
        S = self.grid * self.grid
        table = tables[name]
        width = 1 if name == "policy" else 4
        if not isinstance(table, torch.Tensor) or table.numel() != P * S * width:
            raise ValueError("%s must be a tensor of %d problems x %d states%s" % (name, P, S, "" if width == 1 else " x 4"))
        tables[name] = table.reshape((P, S) if width == 1 else (P, S, 4))
        start = self._occupancy_start(start, key, goals, P, single)
        if isinstance(d_init, torch.Tensor) and d_init.numel() == P * S:
            d_init = d_init.reshape(P, S)
        t = occupancy_tables(self.layout, start=start, epsilon=epsilon, temperature=temperature, variant=self.variant, goals=goals,
                             gamma=gamma, sweeps=sweeps, tol=tol, rewards=self.rewards, d_init=d_init, validate=False, **tables)
        return _unbatch(t, key, single, ("sweeps_run", "delta"))

    def capture_rollout(self, actions, auto_reset=False, obs_t=None, obs_every=None):
        """rollout(actions, auto_reset) captured into ONE hipGraph (see VecEnvBase._capture); call .replay().  Recording
        observations (obs_t / obs_every) is not captured: ValueError."""
        if obs_t is not None or obs_every is not None:
            raise ValueError("capture_rollout() does not record observations: call rollout(obs_t=..., obs_every=...)")
        return self._capture(actions.shape[0], auto_reset,
                             lambda: self.rollout(actions, auto_reset=auto_reset, device_epoch=auto_reset))

    def planes(self, out=None):
        """The reference's unexpanded planes float32[N,C,G,G] (what it calls retState, lmaze_env.py:208-215):
        the x1 case of the expanded render, ready as network input."""
        N, G, Cn = self.num_envs, self.grid, len(self.channel_mask)
        if out is None:
            out = torch.empty((N, Cn, G, G), dtype=torch.float32, device=self.device)
        with self._guard():
            rc = _abi.lib.lmaze_render_expanded(self._p_obs, G, 1, self._cmask, Cn, out.data_ptr(), N, self._stream())
        _abi.check("lmaze_render_expanded", rc)
        return out


def discounted_returns(reward_t, done_t, gamma, tail=None, out=None):
    """Discounted returns-to-go over trajectory rows, in ONE launch (include/lmaze.h lmaze_returns): walking t = T-1 .. 0,
    ret = reward_t[t] where done_t[t], else reward_t[t] + gamma * ret, starting from `tail` (float32[N], the value behind
    the last row; default 0).  reward_t float32[T,N] and done_t bool / uint8[T,N], contiguous on one GPU -- the rows of
    any rollout(trajectory=True), rollout_policy() or rollout_sample(), grid or foveal.  float32 with the product and the
    sum rounded separately, so a float32 loop on the host gives the same bits.  out: float32[T,N] to fill (it may be
    reward_t itself); default a new tensor.  Returns it."""
    def rows(t, dtypes):
        return (isinstance(t, torch.Tensor) and t.dtype in dtypes and t.dim() == 2 and t.is_cuda and t.is_contiguous()
                and t.device == reward_t.device and tuple(t.shape) == tuple(reward_t.shape))
    if not (isinstance(reward_t, torch.Tensor) and rows(reward_t, (torch.float32,))):
        raise ValueError("reward_t must be a contiguous float32[T,N] tensor on a GPU")
    if not rows(done_t, (torch.bool, torch.uint8)):
        raise ValueError("done_t must be a contiguous bool or uint8 tensor of reward_t's shape, on its device")
    T, N = reward_t.shape
    if tail is not None and not (isinstance(tail, torch.Tensor) and tail.dtype == torch.float32 and tail.device == reward_t.device
                                 and tail.is_contiguous() and tuple(tail.shape) == (N,)):
        raise ValueError("tail must be a contiguous float32[N] tensor on reward_t's device")
    if out is None:
        out = torch.empty_like(reward_t)
    elif not rows(out, (torch.float32,)):
        raise ValueError("out must be a contiguous float32 tensor of reward_t's shape, on its device")
    if T == 0 or N == 0:          # nothing to do; an empty tensor has no address to pass
        return out
    with torch.cuda.device(reward_t.device):
        rc = _abi.lib.lmaze_returns(reward_t.data_ptr(), done_t.data_ptr(), None if tail is None else tail.data_ptr(), float(gamma),
                                    out.data_ptr(), T, N, torch.cuda.current_stream(reward_t.device).cuda_stream)
    _abi.check("lmaze_returns", rc)
    return out


def _rows_like(ref, t, dtypes):
    return (isinstance(t, torch.Tensor) and t.dtype in dtypes and t.dim() == 2 and t.is_cuda and t.is_contiguous()
            and t.device == ref.device and tuple(t.shape) == tuple(ref.shape))


def gae(reward_t, done_t, gamma, lam, value_t=None, tail=None, values=None, key_t=None, key_tail=None, out=None, targets=True):
    """Generalised advantage estimation GAE(lambda) over trajectory rows, in ONE launch (include/lmaze.h lmaze_advantages /
    lmaze_advantages_table): walking t = T-1 .. 0 with v the value of row t and v_next the value of the row behind,
        adv = reward_t[t] - v where done_t[t], else ((reward_t[t] + gamma * v_next) - v) + (gamma * lam) * adv
    in float32, every operation rounded on its own, so a float32 loop on the host gives the same bits.  A done row cuts the
    bootstrap and the trace; the done of a step limit is terminal like any other.  Exactly one value source:
    value_t         rows form: float32[T,N] values, and tail float32[N], the value behind the last row (default 0);
    values + key_t  table form: values float32[S], key_t int32[T,N] (the key_t rows of rollout_policy() / rollout_sample()),
                    v = values[key] for 0 <= key < S and 0 otherwise; key_tail int32[N] keys the state behind the last row
                    (LmazeVecEnv.state_keys() of the env whose rollout has just returned; default: value 0).
    reward_t float32[T,N], done_t bool / uint8[T,N], contiguous on one GPU.  out: float32[T,N] to fill with the advantages
    (it may be reward_t); default a new tensor.  targets: True allocates the value targets adv + v, a float32[T,N] tensor
    fills it (rows form: it may be value_t), False skips them.  Returns (adv_t, target_t or None)."""
    T, N, dev, table = _value_source("gae()", reward_t, done_t, value_t, tail, values, key_t, key_tail)
    if out is None:
        out = torch.empty_like(reward_t)
    elif not _rows_like(reward_t, out, (torch.float32,)):
        raise ValueError("out must be a contiguous float32 tensor of reward_t's shape, on its device")
    if targets is True:
        targets = torch.empty_like(reward_t)
    elif targets is False or targets is None:
        targets = None
    elif not _rows_like(reward_t, targets, (torch.float32,)):
        raise ValueError("targets must be True, False or a contiguous float32 tensor of reward_t's shape, on its device")
    if T == 0 or N == 0:          # nothing to do; an empty tensor has no address to pass
        return out, targets

    def ptr(t):
        return None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if table:
            name = "lmaze_advantages_table"
            rc = _abi.lib.lmaze_advantages_table(reward_t.data_ptr(), done_t.data_ptr(), key_t.data_ptr(), ptr(key_tail),
                                                 values.data_ptr(), values.numel(), float(gamma), float(lam), out.data_ptr(),
                                                 ptr(targets), T, N, stream)
        else:
            name = "lmaze_advantages"
            rc = _abi.lib.lmaze_advantages(reward_t.data_ptr(), done_t.data_ptr(), value_t.data_ptr(), ptr(tail), float(gamma),
                                           float(lam), out.data_ptr(), ptr(targets), T, N, stream)
    _abi.check(name, rc)
    return out, targets


def _value_source(who, reward_t, done_t, value_t, tail, values, key_t, key_tail):
    """What gae() and vtrace() check of their rows and of their one value source -- value_t= with tail=, or values= with key_t=
    and key_tail= -- before anything of their own.  Returns (T, N, device, whether it is the table form)."""
    if not (isinstance(reward_t, torch.Tensor) and _rows_like(reward_t, reward_t, (torch.float32,))):
        raise ValueError("reward_t must be a contiguous float32[T,N] tensor on a GPU")
    if not _rows_like(reward_t, done_t, (torch.bool, torch.uint8)):
        raise ValueError("done_t must be a contiguous bool or uint8 tensor of reward_t's shape, on its device")
    T, N = reward_t.shape
    dev = reward_t.device
    table = values is not None or key_t is not None
    if table == (value_t is not None):
        raise ValueError("%s wants exactly one value source: value_t=, or values= with key_t=" % who)

    def per_env(t, dtype):
        return (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous() and tuple(t.shape) == (N,))
    if table:
        if tail is not None:
            raise ValueError("tail= belongs to the rows form; the table form takes key_tail=")
        if not (isinstance(values, torch.Tensor) and values.dtype == torch.float32 and values.dim() == 1 and values.numel() >= 1
                and values.device == dev and values.is_contiguous()):
            raise ValueError("values must be a contiguous float32[S] tensor, S >= 1, on reward_t's device")
        if not _rows_like(reward_t, key_t, (torch.int32,)):
            raise ValueError("key_t must be a contiguous int32 tensor of reward_t's shape, on its device")
        if key_tail is not None and not per_env(key_tail, torch.int32):
            raise ValueError("key_tail must be a contiguous int32[N] tensor on reward_t's device")
    else:
        if key_tail is not None:
            raise ValueError("key_tail= belongs to the table form; the rows form takes tail=")
        if not _rows_like(reward_t, value_t, (torch.float32,)):
            raise ValueError("value_t must be a contiguous float32 tensor of reward_t's shape, on its device")
        if tail is not None and not per_env(tail, torch.float32):
            raise ValueError("tail must be a contiguous float32[N] tensor on reward_t's device")
    return T, N, dev, table


def table_stats(key_t, actions_t=None, weight_t=None, *, keys, actions=4, count=None, total=None):
    """Counts and sums per (key, action) over trajectory rows, in ONE launch and bitwise reproducible (include/lmaze.h
    lmaze_table_stats): for every sample, bin = (key, action) -- action 0 when actions_t is None, which needs actions=1 --
    count[bin] += 1 and total[bin] += rint(weight * 2**24), in int64.  A sample is skipped entirely when its key is outside
    [0, keys), its action outside [0, actions) (rollout_policy() writes ids above 3 for "no move"), or its weight is not
    finite or |w| >= 2**31.  key_t, actions_t int32 and weight_t float32: contiguous tensors of one shape on one GPU (the
    [T, N] rows of a rollout, or any slice that stays contiguous).  count, total: int64[keys, actions] tables that are ADDED
    ONTO (so statistics can span rollouts); a missing one is allocated as zeros.  Returns (count, total), total None when
    weight_t is; table_means() turns them into means.  Integer sums do not depend on the order of the additions: the tables
    of several ranks are summed exactly by torch.distributed.all_reduce(count) / all_reduce(total) -- the library adds no
    collective of its own."""
    if not (isinstance(key_t, torch.Tensor) and key_t.dtype == torch.int32 and key_t.is_cuda and key_t.is_contiguous()):
        raise ValueError("key_t must be a contiguous int32 tensor on a GPU")
    dev = key_t.device
    for name, t, dt in (("actions_t", actions_t, torch.int32), ("weight_t", weight_t, torch.float32)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and t.device == dev and t.is_contiguous()
                                  and tuple(t.shape) == tuple(key_t.shape)):
            raise ValueError("%s must be a contiguous %s tensor of key_t's shape, on its device" % (name, str(dt).split(".")[-1]))
    for name, v in (("keys", keys), ("actions", actions)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("%s must be an int >= 1" % name)
    keys, actions = int(keys), int(actions)
    if actions > 255 or keys * actions > 1 << 28:
        raise ValueError("actions must be <= 255 and keys * actions <= 2**28")
    if actions_t is None and actions != 1:
        raise ValueError("actions_t=None needs actions=1")
    if total is not None and weight_t is None:
        raise ValueError("total= needs weight_t=")
    for name, t in (("count", count), ("total", total)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device == dev and t.is_contiguous()
                                  and tuple(t.shape) == (keys, actions)):
            raise ValueError("%s must be a contiguous int64[%d, %d] tensor on key_t's device" % (name, keys, actions))
    if count is None:
        count = torch.zeros((keys, actions), dtype=torch.int64, device=dev)
    if total is None and weight_t is not None:
        total = torch.zeros((keys, actions), dtype=torch.int64, device=dev)
    m = key_t.numel()
    if m == 0:
        return count, total
    with torch.cuda.device(dev):
        rc = _abi.lib.lmaze_table_stats(key_t.data_ptr(), None if actions_t is None else actions_t.data_ptr(),
                                        None if weight_t is None else weight_t.data_ptr(), m, keys, actions, count.data_ptr(),
                                        None if total is None else total.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _abi.check("lmaze_table_stats", rc)
    return count, total


def table_means(count, total, fill=0.0):
    """Per-(key, action) means of table_stats()' tables, float64[keys, actions]: total / 2**24 / count where count > 0,
    `fill` elsewhere.  Plain torch on the tables' device; after an all_reduce of both tables, the mean over every rank."""
    if not (isinstance(count, torch.Tensor) and isinstance(total, torch.Tensor) and count.dtype == torch.int64
            and total.dtype == torch.int64 and count.shape == total.shape and count.device == total.device):
        raise ValueError("count and total must be int64 tensors of one shape on one device")
    seen = count > 0
    mean = total.to(torch.float64) / 16777216.0 / count.clamp(min=1).to(torch.float64)
    return torch.where(seen, mean, torch.full_like(mean, float(fill)))


def _unbatch(t, key, single, per_problem):
    """What an env method returns of the *_tables() result t: its only problem without the batch dimension; for key="goal" the
    per-state outputs [G*G, G*G, ...] as [G**4, ...], indexed by the key of state_keys("goal"), those named in per_problem as
    they are; else t."""
    if single:
        return type(t)(*[None if x is None else x[0] for x in t])
    if key == "goal":
        return t._replace(**{n: x.reshape(-1, *x.shape[2:]) for n, x in t._asdict().items() if x is not None and n not in per_problem})
    return t


class _Mazes(collections.namedtuple("_Mazes", "spec v3 dev G S shared layouts")):
    """The maze side of a solve_tables() / score_tables() / evaluate_tables() call, checked: the variant's spec, whether it is
    v3, layouts' device, the grid side, G*G, whether one [G, G] layout serves every problem, and the contiguous layouts."""
    __slots__ = ()

    @classmethod
    def of(cls, layouts, variant, validate):
        if variant not in VARIANTS:
            raise ValueError("unknown variant %r (have %s)" % (variant, sorted(VARIANTS)))
        v3 = variant == "v3"
        if not (isinstance(layouts, torch.Tensor) and layouts.dtype == torch.uint8 and layouts.is_cuda and layouts.dim() in (2, 3)
                and layouts.shape[-1] == layouts.shape[-2]):
            raise ValueError("layouts must be a uint8 tensor [G,G] or [P,G,G] on a GPU")
        G = int(layouts.shape[-1])
        if not (3 <= G <= _abi.MAX_GRID):
            raise ValueError("grid side must be in [3, %d]" % _abi.MAX_GRID)
        layouts = layouts.contiguous()
        if validate:
            _validate_on_device(layouts.reshape(-1, G, G), need_goal=not v3)
        return cls(VARIANTS[variant], v3, layouts.device, G, G * G, layouts.dim() == 2, layouts)

    def problems(self, goals, table=None):
        """P, from the checked goals (v3) or the layouts; one shared v0 layout leaves it to the table: its length, or 1."""
        if self.v3:
            if not (isinstance(goals, torch.Tensor) and goals.dtype == torch.int32 and goals.device == self.dev and goals.dim() == 2
                    and goals.shape[1] == 2 and goals.is_contiguous() and (self.shared or goals.shape[0] == self.layouts.shape[0])):
                raise ValueError("goals must be a contiguous int32 tensor [P,2] on layouts' device (v3)")
            return int(goals.shape[0])
        if goals is not None:
            raise ValueError("goals= belongs to v3: v0's goal is the layout's 'X'")
        if not self.shared:
            return int(self.layouts.shape[0])
        return 1 if table is None else int(table.shape[0])

    def rewards(self, rewards):
        rewards = tuple(float(r) for r in (rewards if rewards is not None else self.spec["rewards"]))
        if len(rewards) != 3:
            raise ValueError("rewards must be (wall, move, goal)")
        return rewards

    def launch(self, entry, rewards, goals, P, own, out):
        """lmaze_solve / _score / _evaluate on layouts' device and current stream: the maze side, the entry's `own` arguments,
        the outputs in their order.  P == 0 launches nothing."""
        if P > 0:
            params = _abi.make_params(self.spec["id"], self.G, _abi.LAYOUT_SHARED if self.shared else _abi.LAYOUT_PER_ENV,
                                      self.spec["step_limit"], *rewards)
            with torch.cuda.device(self.dev):
                rc = getattr(_abi.lib, entry)(C.byref(params), self.layouts.data_ptr(), goals.data_ptr() if self.v3 else None, P, *own,
                                              *[None if o is None else o.data_ptr() for o in out.values()],
                                              torch.cuda.current_stream(self.dev).cuda_stream)
            _abi.check(entry, rc)


def _check_sweeps(sweeps):
    if isinstance(sweeps, bool) or not isinstance(sweeps, (int, np.integer)) or not 1 <= sweeps < 2 ** 31:
        raise ValueError("sweeps must be an int >= 1")


def _check_v_init(v_init, dev, P, S, name="v_init"):
    if v_init is not None and not (isinstance(v_init, torch.Tensor) and v_init.dtype == torch.float32 and v_init.device == dev
                                   and v_init.is_contiguous() and tuple(v_init.shape) == (P, S)):
        raise ValueError("%s must be a contiguous float32[%d, %d] tensor on layouts' device" % (name, P, S))


def _alloc_outputs(shapes, outputs, dev):
    """{name: zeros or None} in shapes' order, from name -> (shape, dtype) and the names asked for."""
    return {k: (torch.zeros(shape, dtype=dtype, device=dev) if k in outputs else None) for k, (shape, dtype) in shapes.items()}


class SolvedTables(collections.namedtuple("SolvedTables", "q v policy sweeps_run delta")):
    """What solve_tables() returns: q float32[P, S, 4], v float32[P, S], policy uint8[P, S], sweeps_run int32[P], delta
    float32[P]; an output that was not asked for is None."""
    __slots__ = ()


SOLVE_OUTPUTS = ("q", "v", "policy", "sweeps_run", "delta")


def solve_tables(layouts, variant="v0", goals=None, gamma=0.99, sweeps=4096, rewards=None, v_init=None, outputs=SOLVE_OUTPUTS,
                 validate=True):
    """Value iteration on the GPU: the optimal action values of every maze, in ONE launch (include/lmaze.h lmaze_solve).
    layouts  uint8 device tensor [G, G] (one layout for every problem) or [P, G, G] (problem p solves its own maze), the
             reference's cell characters, validated like the env's own layouts (validate=False skips that).
    variant  "v0" (the goal is the layout's 'X') or "v3" (the goal of problem p is goals[p]).
    goals    v3: int32 [P, 2] (x, y) on layouts' device; with a [G, G] layout P is goals' length, for v0 it is 1.
    gamma, sweeps   the discount and the most Jacobi sweeps to run; a problem stops at the first sweep that leaves every
             value's bits unchanged (that sweep counts), and sweeps_run tells.
    rewards  (wall, move, goal); default the variant's.
    v_init   float32 [P, G*G] warm start; default 0.
    outputs  the names of the outputs to compute, of "q", "v", "policy", "sweeps_run", "delta"; at least one of the first three.
    State s = x * G + y is the key of LmazeVecEnv.state_keys().  What the solver is and is not: the grid variants only; the
    infinite-horizon discounted problem, the step limit is not in the model; v0's sticky pairs (a move onto an 'S' cell, which
    the step refuses while repeating the previous reward) have no reward of their own and are excluded, q = -inf; a state on a
    'W' cell has q = v = 0.  float32 with every operation rounded on its own, so a float32 numpy loop reproduces every bit.
    Returns SolvedTables(q, v, policy, sweeps_run, delta)."""
    m = _Mazes.of(layouts, variant, validate)
    P, S = m.problems(goals), m.S
    _check_sweeps(sweeps)
    rewards = m.rewards(rewards)
    outputs = tuple(outputs)
    if not set(outputs) <= set(SOLVE_OUTPUTS) or not set(outputs) & {"q", "v", "policy"}:
        raise ValueError("outputs must name some of %s, at least one of q, v, policy" % (SOLVE_OUTPUTS,))
    _check_v_init(v_init, m.dev, P, S)
    out = _alloc_outputs({"q": ((P, S, 4), torch.float32), "v": ((P, S), torch.float32), "policy": ((P, S), torch.uint8),
                          "sweeps_run": ((P,), torch.int32), "delta": ((P,), torch.float32)}, outputs, m.dev)
    m.launch("lmaze_solve", rewards, goals, P, (float(gamma), int(sweeps), None if v_init is None else v_init.data_ptr()), out)
    return SolvedTables(**out)


class ScoredTables(collections.namedtuple("ScoredTables", "optimal steps summary")):
    """What score_tables() returns: optimal int32[P, S], steps int32[P, S], summary int32[P, 4] (reachable, arrived, shortest,
    excess); an output that was not asked for is None."""
    __slots__ = ()


SCORE_OUTPUTS = ("optimal", "steps", "summary")


def score_tables(layouts, policy=None, q=None, variant="v0", goals=None, rewards=None, outputs=SCORE_OUTPUTS, validate=True):
    """How good a table is, exactly and from every cell at once, in ONE launch (include/lmaze.h lmaze_score): no rollout, no
    step limit, and a loop is told from a long path.
    layouts  uint8 device tensor [G, G] (one maze for every problem) or [P, G, G], as solve_tables().
    policy   uint8 [P, G*G]: the action of every state (what solve_tables().policy is) -- or
    q        float32 [P, G*G, 4]: the action is the first maximum by a strict '>' (what solve_tables().q is and what
             rollout_qlearn() updates).  At most one of the two; none when only "optimal" is asked for.  With a [G, G] layout
             and v0, P is the table's length: a population of tables on one maze.
    variant, goals, rewards   as solve_tables(): the model is the same.
    outputs  some of "optimal" (the fewest steps after which done can be set, -1: never, and on walls), "steps" (the steps
             after which the table's walk sets it, -1: never -- a cycle, a wall bump, a sticky pair, an action above 3) and
             "summary" (per problem: cells that can reach done, cells whose walk arrives, cells whose walk is a shortest one,
             and the steps the arriving walks take beyond the fewest).
    validate=False skips the layouts' check and the device-side check that no policy byte is above 3.
    Returns ScoredTables(optimal, steps, summary)."""
    m = _Mazes.of(layouts, variant, validate)
    S, dev = m.S, m.dev
    if policy is not None and q is not None:
        raise ValueError("give policy= or q=, not both")
    table = policy if policy is not None else q
    if table is not None:
        want = (torch.uint8, 2) if policy is not None else (torch.float32, 3)
        if not (isinstance(table, torch.Tensor) and table.dtype == want[0] and table.device == dev and table.dim() == want[1]
                and table.is_contiguous() and tuple(table.shape[1:]) == ((S,) if policy is not None else (S, 4))):
            raise ValueError("policy must be a contiguous uint8[P, %d] and q a contiguous float32[P, %d, 4] tensor on layouts' device"
                             % (S, S))
    P = m.problems(goals, table)
    if table is not None and int(table.shape[0]) != P:
        raise ValueError("the table has %d problems, the mazes %d" % (int(table.shape[0]), P))
    rewards = m.rewards(rewards)
    outputs = tuple(outputs)
    if not outputs or not set(outputs) <= set(SCORE_OUTPUTS):
        raise ValueError("outputs must name some of %s" % (SCORE_OUTPUTS,))
    if "steps" in outputs and table is None:
        raise ValueError("'steps' needs a table: policy= or q=")
    if validate and policy is not None and bool((policy > 3).any()):
        raise ValueError("policy holds a byte above 3: the actions are 0..3")
    out = _alloc_outputs({"optimal": ((P, S), torch.int32), "steps": ((P, S), torch.int32), "summary": ((P, 4), torch.int32)},
                         outputs, dev)
    m.launch("lmaze_score", rewards, goals, P,
             (None if policy is None else policy.data_ptr(), None if q is None else q.data_ptr()), out)
    return ScoredTables(**out)


def _policy_table(m, kind, goals, policy, q, epsilon, probs, logits, temperature, thresholds):
    """The one table of an evaluate_tables() / occupancy_tables() call on the mazes m, checked; kind is what _tables.exactly_one
    named.  Returns (kind, table, epsilon_u32, P): kind "policy", "q" or "thresholds" -- probs= and logits= converted as
    rollout_sample() converts them -- and P from the goals, the layouts or the table (_Mazes.problems)."""
    S, dev = m.S, m.dev
    eps = _abi.epsilon_u32(epsilon)
    if kind in ("probs", "logits", "thresholds") and eps != 0:
        raise ValueError("epsilon belongs to policy= and q=: a categorical table already says how it explores")
    if kind in ("probs", "logits"):
        src = probs if kind == "probs" else logits
        if not (isinstance(src, torch.Tensor) and src.dim() == 3 and tuple(src.shape[1:]) == (S, 4)):
            raise ValueError("%s must be a float tensor [P, %d, 4] on layouts' device" % (kind, S))
        P = int(src.shape[0])                       # the source's: one shared v0 layout leaves P to the table
        rows = src.reshape(P * S, 4)
        thresholds = _tables.threshold_table(rows if kind == "probs" else None, rows if kind == "logits" else None, None,
                                             temperature, P * S, 4, dev, "P=%d, G=%d" % (P, m.G)).view(P, S, 4)
    if kind == "policy":
        table, ok = policy, (isinstance(policy, torch.Tensor) and policy.dtype == torch.uint8 and policy.dim() == 2
                             and tuple(policy.shape[1:]) == (S,))
    elif kind == "q":
        table, ok = q, (isinstance(q, torch.Tensor) and q.dtype == torch.float32 and q.dim() == 3 and tuple(q.shape[1:]) == (S, 4)
                        and q.data_ptr() % 16 == 0)
    else:
        table, ok = thresholds, (isinstance(thresholds, torch.Tensor) and thresholds.dtype in (torch.uint32, torch.int32)
                                 and thresholds.dim() == 3 and tuple(thresholds.shape[1:]) == (S, 4)
                                 and thresholds.data_ptr() % 16 == 0)
    if not (ok and table.device == dev and table.is_contiguous()):
        raise ValueError("policy must be a contiguous uint8[P, %d], q a contiguous float32[P, %d, 4] and thresholds a contiguous, "
                         "16-byte aligned uint32[P, %d, 4] tensor on layouts' device" % (S, S, S))
    P = m.problems(goals, table)
    if int(table.shape[0]) != P:
        raise ValueError("the table has %d problems, the mazes %d" % (int(table.shape[0]), P))
    return ("thresholds" if kind in ("probs", "logits") else kind), table, eps, P


class EvaluatedTables(collections.namedtuple("EvaluatedTables", "q v sweeps_run delta")):
    """What evaluate_tables() returns: q float32[P, S, 4] (Q^pi), v float32[P, S] (V^pi), sweeps_run int32[P], delta
    float32[P]; an output that was not asked for is None."""
    __slots__ = ()


EVALUATE_OUTPUTS = ("q", "v", "sweeps_run", "delta")


def evaluate_tables(layouts, policy=None, q=None, epsilon=0.0, probs=None, logits=None, temperature=1.0, thresholds=None,
                    variant="v0", goals=None, gamma=0.99, sweeps=4096, tol=0.0, rewards=None, v_init=None,
                    outputs=EVALUATE_OUTPUTS, validate=True):
    """Exact policy evaluation on the GPU: V^pi and Q^pi of the stochastic table a closed-loop rollout would run, for every
    maze, in ONE launch (include/lmaze.h lmaze_evaluate) -- no Monte-Carlo estimate, no host loop.
    layouts  uint8 device tensor [G, G] (one maze for every problem) or [P, G, G], as solve_tables().
    Exactly one of
    policy      uint8 [P, G*G] with epsilon: the epsilon-greedy policy rollout_policy(policy=, epsilon=) runs;
    q           float32 [P, G*G, 4] with epsilon: the same, the greedy action being the first maximum by a strict '>';
    probs       float [P, G*G, 4] of non-negative weights, converted by _abi.sampling_thresholds() as rollout_sample() does;
    logits      float [P, G*G, 4]: sampling_thresholds(softmax(logits.double() / temperature)), temperature > 0;
    thresholds  the table itself, uint32 (or int32, the same bits) [P, G*G, 4], contiguous and 16-byte aligned.
    What is evaluated is exactly the table that would be run: epsilon converts as rollout_policy() converts it, the
    categorical inputs go through rollout_sample()'s conversion (a row of probability 1 keeps 2**-32 on action 3) and a
    thresholds row that is not monotone is weighed by its three words in ascending order, the law the sampler's compares
    give it; epsilon != 0 with a categorical input is refused.  q= is read by the learner's rule (rollout_qlearn()'s first
    maximum, also on a row with a NaN); rollout_policy(q=) reads a row with a NaN as "no move", so policy=greedy_table(q)
    evaluates exactly what it runs.  With a [G, G] layout and v0, P is the table's length.
    variant, goals, rewards, gamma, v_init   as solve_tables(): the model is the same.
    sweeps, tol   a problem stops at the first Jacobi sweep that leaves every value's bits unchanged (that sweep counts), at
             the first whose delta is <= tol when tol > 0, or after `sweeps`.
    outputs  some of "q", "v", "sweeps_run", "delta"; at least one of the first two.
    What the evaluator is and is not: the grid variants only; the infinite-horizon discounted problem, the step limit is not
    in the model; the mass a policy puts on v0's sticky pairs, which solve_tables() excludes, is renormalised over the usable
    pairs (a state with no usable mass has v = 0); float32 Jacobi with every operation rounded on its own, so a float32 numpy
    loop reproduces every bit.  validate=False skips the layouts' check.
    Returns EvaluatedTables(q, v, sweeps_run, delta)."""
    m = _Mazes.of(layouts, variant, validate)
    S, dev = m.S, m.dev
    kind = _tables.exactly_one("evaluate_tables()", policy=policy, q=q, probs=probs, logits=logits, thresholds=thresholds)
    kind, table, eps, P = _policy_table(m, kind, goals, policy, q, epsilon, probs, logits, temperature, thresholds)
    _check_sweeps(sweeps)
    rewards = m.rewards(rewards)
    outputs = tuple(outputs)
    if not set(outputs) <= set(EVALUATE_OUTPUTS) or not set(outputs) & {"q", "v"}:
        raise ValueError("outputs must name some of %s, at least one of q, v" % (EVALUATE_OUTPUTS,))
    _check_v_init(v_init, dev, P, S)
    out = _alloc_outputs({"q": ((P, S, 4), torch.float32), "v": ((P, S), torch.float32), "sweeps_run": ((P,), torch.int32),
                          "delta": ((P,), torch.float32)}, outputs, dev)
    m.launch("lmaze_evaluate", rewards, goals, P,
             (table.data_ptr() if kind == "policy" else None, table.data_ptr() if kind == "q" else None, eps,
              table.data_ptr() if kind not in ("policy", "q") else None, float(gamma), int(sweeps), float(tol),
              None if v_init is None else v_init.data_ptr()), out)
    return EvaluatedTables(**out)


class OccupancyTables(collections.namedtuple("OccupancyTables", "d d_sa sweeps_run delta")):
    """What occupancy_tables() returns: d float32[P, S] (the discounted state occupancy), d_sa float32[P, S, 4] (d(s) * p_a(s)),
    sweeps_run int32[P], delta float32[P]; an output that was not asked for is None."""
    __slots__ = ()


OCCUPANCY_OUTPUTS = ("d", "d_sa", "sweeps_run", "delta")


def reset_distribution(layouts, variant="v0", goals=None):
    """The law of the ball cell reset() draws, float32[P, G*G]: uniform over the cells include/lmaze.h lmaze_reset accepts --
    v0: interior, not 'W', not 'X'; v3: interior, not 'W', not the problem's goal (goals int [P, 2]; with a [G, G] layout P
    is goals' length, for v0 it is 1).  A problem without an accepted cell gets a row of zeros.  Plain torch, on layouts'
    device, which need not be a GPU."""
    if variant not in ("v0", "v3"):
        raise ValueError("reset_distribution() knows the grid variants 'v0' and 'v3'")
    if not (isinstance(layouts, torch.Tensor) and layouts.dtype == torch.uint8 and layouts.dim() in (2, 3)
            and layouts.shape[-1] == layouts.shape[-2] and layouts.shape[-1] >= 3):
        raise ValueError("layouts must be a uint8 tensor [G,G] or [P,G,G]")
    G = int(layouts.shape[-1])
    lay = layouts.reshape(-1, G, G)
    ok = lay != ord("W")
    ok[:, 0, :] = ok[:, -1, :] = ok[:, :, 0] = ok[:, :, -1] = False
    if variant == "v3":
        if not (isinstance(goals, torch.Tensor) and goals.dim() == 2 and goals.shape[1] == 2 and goals.device == layouts.device
                and (layouts.dim() == 2 or goals.shape[0] == lay.shape[0])):
            raise ValueError("goals must be an int tensor [P,2] on layouts' device (v3)")
        g = goals.long()
        ok = ok.reshape(-1, G * G).expand(g.shape[0], G * G).clone()
        rows = torch.nonzero((g[:, 0] >= 0) & (g[:, 0] < G) & (g[:, 1] >= 0) & (g[:, 1] < G)).reshape(-1)
        ok[rows, g[rows, 0] * G + g[rows, 1]] = False
    else:
        if goals is not None:
            raise ValueError("goals= belongs to v3: v0's goal is the layout's 'X'")
        ok = (ok & (lay != ord("X"))).reshape(-1, G * G)
    n = ok.sum(1, keepdim=True).clamp(min=1)
    return (ok.to(torch.float32) / n.to(torch.float32)).contiguous()


def start_thresholds(start):
    """The table reset(thresholds=...) and lmaze_reset_start take, uint32[P, S] on start's device, of a float tensor
    start[P, S] (or [S]: one row) of non-negative weights; a row need not sum to 1.  In float64:
        a_j = start_0 + ... + start_j (running sums), s = a_(S-1);   c_j = floor(a_j / s * 2**31 + 0.5)
    over the cells that have mass, then a running maximum: a zero-mass cell gets c_j = c_(j-1), c_(-1) = 0; the word of the
    last massive cell and every word behind it is exactly 2**31.  Cell j is then drawn with probability
    (c_j - c_(j-1)) / 2**31, within 2**-30 of start_j / s, and a cell without mass is never drawn.  A row of zero total mass
    becomes a row of zeros, lmaze_reset_start's "the ball stays" row.  Refuses negative or non-finite entries."""
    if not (isinstance(start, torch.Tensor) and start.is_floating_point() and start.dim() in (1, 2) and start.shape[-1] >= 1):
        raise ValueError("start must be a float tensor [P, S] or [S]")
    p = start.detach().to(torch.float64).reshape(-1, start.shape[-1])
    if not bool(torch.isfinite(p).all()) or bool((p < 0).any()):
        raise ValueError("start holds a negative or non-finite entry")
    S = p.shape[1]
    a = torch.cumsum(p, dim=1)
    s = a[:, -1:]
    if not bool(torch.isfinite(s).all()):
        raise ValueError("a row of start has no finite sum")
    massive = p > 0
    c = torch.floor(a / torch.where(s > 0, s, torch.ones_like(s)) * 2147483648.0 + 0.5).clamp_(max=2147483648.0).to(torch.int64)
    c = torch.cummax(torch.where(massive, c, torch.zeros_like(c)), dim=1).values
    # from the last massive cell on: exactly 2**31 (a row without mass has no such cell and stays 0)
    cells = torch.arange(S, device=p.device)
    last = torch.where(massive, cells, torch.full_like(cells, -1)).max(dim=1, keepdim=True).values
    c = torch.where((last >= 0) & (cells >= last), torch.full_like(c, 2147483648), c)
    return torch.where(c >= 2147483648, c - 4294967296, c).to(torch.int32).view(torch.uint32).contiguous()   # the same 32 bits


def distance_band(optimal, lo, hi, layouts, variant="v0", goals=None, empty="reset"):
    """A curriculum stage over the distance field, float32[P, G*G]: uniform over the cells reset_distribution() gives mass AND
    whose optimal -- score()'s fewest steps to done, int [P, G*G] or [G*G] -- lies in [lo, hi].  lo / hi: ints, or int tensors
    [P] for a stage per maze.  A problem whose band is empty gets reset_distribution()'s row (empty="reset") or a row of zeros
    (empty="zero": reset(start=...) then leaves that ball where it is).  layouts, variant, goals: as reset_distribution(); one
    shared row serves every problem of optimal.  Plain torch: the law occupancy(start=...) and reset(start=...) take as it is.
    ("Mazes by difficulty" needs no helper: sort score()'s summary column, e.g. summary[:, 0].argsort().)"""
    if empty not in ("reset", "zero"):
        raise ValueError("empty must be 'reset' or 'zero'")
    base = reset_distribution(layouts, variant, goals)
    S = base.shape[1]
    if not (isinstance(optimal, torch.Tensor) and not optimal.is_floating_point() and optimal.device == base.device
            and optimal.numel() % S == 0 and optimal.numel() > 0):
        raise ValueError("optimal must be an int tensor [P, %d] on layouts' device" % S)
    opt = optimal.reshape(-1, S).long()
    P = opt.shape[0]
    if base.shape[0] not in (1, P):
        raise ValueError("optimal holds %d problems, the layouts and goals %d" % (P, base.shape[0]))
    base = base.expand(P, S)

    def bound(x, name):
        if isinstance(x, torch.Tensor):
            if x.is_floating_point() or x.numel() != P or x.device != base.device:
                raise ValueError("%s must be an int or an int tensor [%d] on layouts' device" % (name, P))
            return x.reshape(P, 1).long()
        return int(x)

    band = (base > 0) & (opt >= bound(lo, "lo")) & (opt <= bound(hi, "hi"))
    n = band.sum(1, keepdim=True)
    law = band.to(torch.float32) / n.clamp(min=1).to(torch.float32)
    if empty == "reset":
        law = torch.where(n > 0, law, base)
    return law.contiguous()


def _check_start(start, dev, P, S, validate):
    _check_v_init(start, dev, P, S, "start")
    if start is None:
        raise ValueError("start must be a contiguous float32[%d, %d] tensor on layouts' device" % (P, S))
    if validate and not bool(((start >= 0) & torch.isfinite(start)).all()):
        raise ValueError("start holds a negative or non-finite entry")


def occupancy_tables(layouts, start=None, policy=None, q=None, epsilon=0.0, probs=None, logits=None, temperature=1.0, thresholds=None,
                     variant="v0", goals=None, gamma=0.99, sweeps=4096, tol=0.0, rewards=None, d_init=None,
                     outputs=OCCUPANCY_OUTPUTS, validate=True):
    """Exact discounted occupancy on the GPU: where the stochastic table a closed-loop rollout would run spends its discounted
    time, d = start + gamma * P_pi^T d, for every maze, in ONE launch (include/lmaze.h lmaze_occupancy) -- evaluate_tables()'s
    adjoint, over the same model and the same probabilities.
    layouts, the five table inputs, epsilon, temperature, variant, goals, rewards, gamma, sweeps, tol   as evaluate_tables().
    start    float32 [P, G*G] on layouts' device: the mass every sweep adds; need not sum to 1.  None: reset_distribution(),
             the law of the cell reset() places the ball on.
    d_init   float32 [P, G*G] warm start; default 0, from which a non-negative start makes every sweep monotone and the exact
             stop certain.
    outputs  some of "d", "d_sa", "sweeps_run", "delta"; at least one of the first two.
    With evaluate_tables() of the same table: J = (start * v).sum(-1) = (d_sa * r).sum() is the expected return per maze, and
    d[..., None] * p * (q - v[..., None]) / temperature the exact gradient of J in the logits, where no pair of the state is
    excluded.  What it is and is not: as evaluate_tables() -- the grid variants only; the infinite-horizon discounted problem;
    mass on v0's sticky pairs is renormalised over the usable ones; mass on a terminal pair is absorbed; float32 Jacobi with
    every operation rounded on its own, so a float32 numpy loop reproduces every bit.  validate=False skips the layouts' check
    and the check that start has no negative or non-finite entry.
    Returns OccupancyTables(d, d_sa, sweeps_run, delta)."""
    kind = _tables.exactly_one("occupancy_tables()", policy=policy, q=q, probs=probs, logits=logits, thresholds=thresholds)
    m = _Mazes.of(layouts, variant, validate)
    S, dev = m.S, m.dev
    kind, table, eps, P = _policy_table(m, kind, goals, policy, q, epsilon, probs, logits, temperature, thresholds)
    _check_sweeps(sweeps)
    rewards = m.rewards(rewards)
    outputs = tuple(outputs)
    if not set(outputs) <= set(OCCUPANCY_OUTPUTS) or not set(outputs) & {"d", "d_sa"}:
        raise ValueError("outputs must name some of %s, at least one of d, d_sa" % (OCCUPANCY_OUTPUTS,))
    if start is None:
        start = reset_distribution(m.layouts, variant, goals)
        if start.shape[0] != P:                     # one shared v0 layout under P tables
            start = start.expand(P, S).contiguous()
    else:
        _check_start(start, dev, P, S, validate)
    _check_v_init(d_init, dev, P, S, "d_init")
    out = _alloc_outputs({"d": ((P, S), torch.float32), "d_sa": ((P, S, 4), torch.float32), "sweeps_run": ((P,), torch.int32),
                          "delta": ((P,), torch.float32)}, outputs, dev)
    m.launch("lmaze_occupancy", rewards, goals, P,
             (table.data_ptr() if kind == "policy" else None, table.data_ptr() if kind == "q" else None, eps,
              table.data_ptr() if kind == "thresholds" else None, start.data_ptr(), float(gamma), int(sweeps), float(tol),
              None if d_init is None else d_init.data_ptr()), out)
    return OccupancyTables(**out)


def _validate_on_device(lay, need_goal=True):
    W = ord("W")
    ok = ((lay[:, 0, :] == W).all() & (lay[:, -1, :] == W).all() & (lay[:, :, 0] == W).all()
          & (lay[:, :, -1] == W).all())
    if not bool(ok):
        raise ValueError("every layout needs a full 'W' border")
    codes = torch.tensor([ord(c) for c in "WBSX"], dtype=torch.uint8, device=lay.device)
    if not bool(torch.isin(lay, codes).all()):
        raise ValueError("layout cells must be one of 'W', 'B', 'S', 'X'")
    if need_goal and not bool((lay == ord("X")).flatten(1).any(dim=1).all()):
        raise ValueError("a layout has no 'X' cell")
