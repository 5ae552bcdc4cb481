"""LmazeFovealVecEnv: N envs of the foveal variants (v1, v2, v4) as struct-of-arrays torch
tensors in HBM, stepped by one HIP kernel per step() -- or per rollout() of T steps -- through lmaze_foveal_*
(include/lmaze.h).

Host side only (buffers, marshalling, stream); the transition, the visit-map update and the
5x5 window render run in liblmaze_hip.so.  Reference: gym_lmaze/envs/lmaze_env_v1.py,
lmaze_env_v2.py, lmaze_env_v4.py.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi
from . import _tables
from . import layouts as L
from ._base import VecEnvBase

FOVEAL_VARIANTS = {
    # lmaze_env_v1.py:21-36
    "v1": dict(id=_abi.VARIANT_V1, layouts=(L.V1_GRID_14,), channels=4, expansion=7, step_limit=200,
               foveal_step_limit=10, rewards=(-1.0, 0.01, 1.0), n_actions=4),
    # lmaze_env_v2.py:26-49
    "v2": dict(id=_abi.VARIANT_V2, layouts=L.FOVEAL_GRIDS_18, channels=5, expansion=7, step_limit=50,
               foveal_step_limit=0, rewards=(-1.0, -0.01, 100.0), n_actions=25),
    # lmaze_env_v4.py:23-48
    "v4": dict(id=_abi.VARIANT_V4, layouts=L.FOVEAL_GRIDS_18, channels=7, expansion=7, step_limit=50,
               foveal_step_limit=0, rewards=(-1.0, -0.01, 100.0), n_actions=25),
    # lmaze_env_v5.py:21-49: local step limit 10 (>=), foveal step limit 50 (>=); 4 local actions, 25 planner goals
    "v5": dict(id=_abi.VARIANT_V5, layouts=L.FOVEAL_GRIDS_18, channels=7, expansion=7, step_limit=10,
               foveal_step_limit=50, rewards=(-1.0, -0.01, 100.0), n_actions=4),
    "v6": dict(id=_abi.VARIANT_V6, layouts=L.FOVEAL_GRIDS_18, channels=7, expansion=7, step_limit=10,
               foveal_step_limit=50, rewards=(-1.0, -0.01, 100.0), n_actions=4),
}


class LmazeFovealVecEnv(VecEnvBase):
    """N foveal mazes.  obs is float32[N,C,5,5] -- the reference's retState before its x7 loop;
    expanded() gives the (C,35,35) reference layout."""

    def __init__(self, num_envs, variant="v2", layouts=None, device=None, seed=0, env_base=0, reset=True):
        if variant not in FOVEAL_VARIANTS:
            raise ValueError("unknown foveal variant %r (have %s)" % (variant, sorted(FOVEAL_VARIANTS)))
        spec = FOVEAL_VARIANTS[variant]
        self.variant = variant
        self._init_common(num_envs, device, seed, env_base)
        N = self.num_envs
        self.channels = spec["channels"]
        self.expansion = spec["expansion"]
        tabs = [L.to_codes(t) for t in (layouts if layouts is not None else spec["layouts"])]
        G = tabs[0].shape[0]
        pad = 2 if variant == "v1" else 2   # the 5x5 window must stay inside the array
        for t in tabs:
            if t.shape != (G, G):
                raise ValueError("all layouts must share one square shape")
            L.validate(t, need_goal_marker=(variant == "v1"))
            W = ord("W")
            if not ((t[:pad] == W).all() and (t[-pad:] == W).all() and (t[:, :pad] == W).all() and (t[:, -pad:] == W).all()):
                raise ValueError("foveal layouts need a %d-cell 'W' padding (lmaze_env_v1.py:40-53)" % pad)
        if variant == "v1" and len(tabs) != 1:
            raise ValueError("v1 has a single layout")
        self.grid = G
        self.n_layouts = len(tabs)
        self.layouts = torch.from_numpy(np.stack(tabs).copy()).to(self.device)

        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        self._alloc_state([("ball_xy", i32, 2), ("goal_xy", i32, 2), ("fgoal_xy", i32, 2), ("layout_id", i32, 1),
                           ("step_count", i32, 1), ("foveal_step_count", i32, 1), ("reward", f32, 1),
                           ("foveal_reward", f32, 1), ("done", u8, 1), ("foveal_done", u8, 1), ("ball1_xy", i32, 2),
                           ("fovea_xy", i32, 4), ("last_xy", i32, 2), ("foveal_goal", i32, 1)])
        self._two_level = variant in ("v5", "v6")
        # the visit map in the library's clock-relative 4x4 tiles (include/lmaze.h "The visit map"): opaque here; the
        # reference's float[N,G,G] is the `visit` property (lmaze_foveal_materialise_visit)
        self._has_visit = variant in ("v4", "v5", "v6")
        self._visit_tiles = self._visit_clock = None
        if self._has_visit:
            nbytes = int(_abi.lib.lmaze_foveal_visit_bytes(G, N))
            self._visit_tiles = torch.zeros(nbytes // 4, dtype=torch.float32, device=self.device)
            self._visit_clock = torch.zeros(N, dtype=torch.int32, device=self.device)
            assert self._visit_tiles.data_ptr() % 64 == 0
            self._persistent += [self._visit_tiles, self._visit_clock]
        self.obs_local = (torch.zeros((N, 4, _abi.FOVEA, _abi.FOVEA), dtype=torch.float32, device=self.device)
                          if self._two_level else None)
        self._expanded_local = None
        self.obs = torch.zeros((N, self.channels, _abi.FOVEA, _abi.FOVEA), dtype=torch.float32, device=self.device)
        self._expanded = None

        r = spec["rewards"]
        self.params = _abi.LmazeFovealParams(spec["id"], G, self.n_layouts, spec["step_limit"],
                                             spec["foveal_step_limit"], r[0], r[1], r[2], 0)
        self._pp = C.byref(self.params)
        ptrs = {name: v.data_ptr() for name, v in self._views.items()}
        for name, t in (("visit", self._visit_tiles), ("obs", self.obs), ("obs_local", self.obs_local),
                        ("visit_clock", self._visit_clock)):
            ptrs[name] = t.data_ptr() if t is not None else None
        self.bufs = _abi.LmazeFovealBuffers(**ptrs)
        self._pb = C.byref(self.bufs)
        self._p_layouts = self.layouts.data_ptr()
        if variant == "v1":
            # goal = the 'X' cell (lmaze_env_v1.py:86-88); kept for the drop-in attributes
            c = int(np.flatnonzero(tabs[0].reshape(-1) == ord("X"))[0])
            self.goal_xy.copy_(torch.tensor([[c // G, c % G]], dtype=torch.int32).expand(N, 2))
        if reset:
            self.reset()

    # ------------------------------------------------------------------ the visit map (v4, v5, v6)
    @property
    def visit(self):
        """The reference's state[2]: float32[N,G,G] true values, materialised from the clock-relative tiles (a NEW
        tensor on every access; off the step path).  None for v1 / v2."""
        if not self._has_visit:
            return None
        out = torch.empty((self.num_envs, self.grid, self.grid), dtype=torch.float32, device=self.device)
        with self._guard():
            rc = _abi.lib.lmaze_foveal_materialise_visit(self._pp, self._pb, out.data_ptr(), self.num_envs, self._stream())
        _abi.check("lmaze_foveal_materialise_visit", rc)
        return out

    def load_visit(self, values):
        """Take float32[N,G,G] true values (e.g. the reference's own state[2]) as the visit map."""
        t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values, dtype=np.float32))
        t = t.to(device=self.device, dtype=torch.float32).reshape(self.num_envs, self.grid, self.grid).contiguous()
        with self._guard():
            rc = _abi.lib.lmaze_foveal_load_visit(self._pp, self._pb, t.data_ptr(), self.num_envs, self._stream())
        _abi.check("lmaze_foveal_load_visit", rc)

    # ------------------------------------------------------------------ the path
    def step(self, actions, auto_reset=False, epoch_slot=None):
        """v1: ids 0..3 (else no move); v2/v4: 0..24 = 5*row+col of the target cell in the window.
        Returns (obs, reward, done, actions); v1's second stream is in foveal_reward / foveal_done.
        auto_reset=True (v1, v2, v4) first resets the envs whose done flag is still set from the previous
        step, fused into the same kernel: bit-identical to reset(mask=done) + step(actions).
        epoch_slot=t (under hipGraph capture, t = index of the launch in the captured sequence) keeps the
        reset epoch on the device so that replays draw fresh placements; call begin_replay(T) before each."""
        self.step_raw(self._as_i32(actions, self.num_envs).data_ptr(), auto_reset, epoch_slot)
        return self.obs, self.reward, self.done, actions

    def step_raw(self, action_ptr, auto_reset=False, epoch_slot=None):
        """step() on a raw device pointer to int32[N] actions (rollouts over a pre-generated [T,N] tensor)."""
        with self._guard():
            if auto_reset:
                if self._two_level:
                    raise ValueError("auto_reset is not defined for v5/v6 (episodes restart through the two-level step: "
                                     "hier_step)")
                epoch, e_in, e_out = self._epoch_args(True, epoch_slot)
                rc = _abi.lib.lmaze_foveal_step_autoreset(self._pp, self._p_layouts, action_ptr, self._pb, self.num_envs,
                                                          self.seed & (2 ** 64 - 1), epoch, self.env_base,
                                                          e_in, e_out, self._stream())
            else:
                rc = _abi.lib.lmaze_foveal_step(self._pp, self._p_layouts, action_ptr, self._pb, self.num_envs, self._stream())
        _abi.check("lmaze_foveal_step", rc)

    def hier_step(self, actions, goals, epoch_slot=None):
        """v5/v6: the two-level loop around step() as ONE launch (lmaze_v5_hier_step) -- reset() for the envs whose
        globalDone (`done`) is set on entry, plannerStep(goals[i]) for those whose localDone (`foveal_done`) is set
        or that were just reset, then step(actions[i]) for everybody.  Bit-identical to reset(mask=done),
        planner_step(goals, mask=done | foveal_done), step(actions).  Returns (obs, obs_local, reward,
        foveal_reward, done, foveal_done) -- the tensors of the reference's 8-tuple (lmaze_env_v5.py:285-292)."""
        a = self._as_i32(actions, self.num_envs)
        g = self._as_i32(goals, self.num_envs)
        self.hier_step_raw(a.data_ptr(), g.data_ptr(), epoch_slot)
        return self.obs, self.obs_local, self.reward, self.foveal_reward, self.done, self.foveal_done

    def hier_step_raw(self, action_ptr, goal_ptr, epoch_slot=None):
        if not self._two_level:
            raise ValueError("hier_step is the two-level loop of v5/v6")
        with self._guard():
            epoch, e_in, e_out = self._epoch_args(True, epoch_slot)
            rc = _abi.lib.lmaze_v5_hier_step(self._pp, self._p_layouts, action_ptr, goal_ptr, self._pb, self.num_envs,
                                             self.seed & (2 ** 64 - 1), epoch, self.env_base, e_in, e_out, self._stream())
        _abi.check("lmaze_v5_hier_step", rc)

    def rollout(self, actions, goals=None, auto_reset=False, device_epoch=False, trajectory=False, obs_t=None,
                obs_local_t=None, obs_every=None):
        """T steps over device tensors int32[T,N], no host sync: step(actions[t]) -- with the reset fused in when
        auto_reset (v1, v2, v4) -- or, for v5/v6 with `goals`, the two-level step hier_step(actions[t], goals[t]).
        The whole rollout is ONE launch (lmaze_foveal_rollout, include/lmaze.h), bit-identical to the T step launches --
        except the plain v5/v6 step without goals, which stays T launches;
        the epoch ends where those would leave it (+T with auto_reset or goals).  device_epoch=True keeps the reset
        epoch on the device and launches T steps instead (what capture_rollout records).  Returns the final
        (obs, reward, done); trajectory=True adds every step's reward float32[T,N] and done bool[T,N] and, v1 / v5 / v6,
        foveal_reward float32[T,N] and foveal_done bool[T,N] (the second stream) as well.
        obs_every=k >= 1 records observations into the caller's obs_t, float32 (T // k, N, C, 5, 5): slot j is what obs
        holds after step (j + 1) k - 1 (lmaze_foveal_rollout_obs, still one launch; the plain v5/v6 step copies obs after
        each recorded step launch); v5/v6 also obs_local_t (T // k, N, 4, 5, 5), optional.  The final obs, state and rows
        are those of the plain rollout.  Not with device_epoch."""
        hier = goals is not None
        if obs_every is not None:
            self._check_rows("rollout()", actions, goals)
            if device_epoch:
                raise ValueError("rollout(obs_every=...) is not available with a device-resident epoch")
            if obs_local_t is not None and not self._two_level:
                raise ValueError("obs_local_t: v5/v6 only")
        k = self._recording(0 if obs_every is None else int(actions.shape[0]), obs_every, obs_t, obs_local_t)
        self._check_rows("rollout()", actions, goals)
        if hier and (not self._two_level or goals.shape[0] != actions.shape[0]):
            raise ValueError("planner goals: v5/v6 only, one row per step")
        if self._two_level and not hier:
            if auto_reset:
                raise ValueError("v5/v6 restart episodes through the two-level step: pass goals")
        T, N = int(actions.shape[0]), self.num_envs
        base, stride = actions.data_ptr(), N * 4

        def launch(t, slot=None):                       # step t as its own launch (slot: its index under capture)
            if hier:
                self.hier_step_raw(base + t * stride, goals.data_ptr() + t * stride, slot)
            else:
                self.step_raw(base + t * stride, auto_reset=auto_reset, epoch_slot=slot if auto_reset else None)

        if device_epoch:
            if trajectory:
                raise ValueError("rollout(trajectory=True) is not available with a device-resident epoch")
            self._step_loop(T, lambda t: launch(t, t))
            return self.obs, self.reward, self.done
        rows = self._traj_rows(T, 2 if self.variant in ("v1", "v5", "v6") else 1) if trajectory else None
        if ((k and ((hier and self.grid != 18) or (self.variant == "v1" and self.grid != 14)))
                or (self._two_level and not hier)):
            # T launches: the two-level recording form exists at G = 18 only, v1's at G = 14 only (include/lmaze.h
            # lmaze_foveal_rollout_obs), and the plain v5/v6 step has no one-launch form (lmaze_foveal_rollout)
            self._step_loop(T, launch, rows, k, obs_t, obs_local_t)
        elif T > 0:
            resets = hier or bool(auto_reset)
            ptrs = [r.data_ptr() for r in rows] if rows else []
            ptrs += [None] * (4 - len(ptrs))
            args = (self._pp, self._p_layouts, base, goals.data_ptr() if hier else None, T, self._pb, N,
                    1 if resets else 0, self.seed & (2 ** 64 - 1), self._epoch, self.env_base, *ptrs)
            with self._guard():
                if not k:
                    rc = _abi.lib.lmaze_foveal_rollout(*args, self._stream())
                else:
                    some = obs_t.shape[0] > 0
                    rc = _abi.lib.lmaze_foveal_rollout_obs(*args, obs_t.data_ptr() if some else None,
                                                           obs_local_t.data_ptr() if some and obs_local_t is not None else None,
                                                           k, self._stream())
            _abi.check("lmaze_foveal_rollout_obs" if k else "lmaze_foveal_rollout", rc)
            if resets:
                self._epoch += T
        return self._rollout_result(rows)

    def rollout_policy(self, T, policy=None, q=None, epsilon=0.0, auto_reset=True, trajectory=False, actions_t=None, key_t=None,
                       obs_t=None, obs_every=None):
        """T steps in ONE launch with a tabular epsilon-greedy policy inside the kernel (include/lmaze.h
        lmaze_foveal_rollout_policy; v1, v2, v4): no action tensor, no per-step launches.
        policy   uint8 device tensor of L*G*G entries, the greedy action id of every key = layout row * G*G + ball_x * G +
                 ball_y (v1: one layout).  Ids mean what they mean to step(): v1 above 3 no move, v2/v4 above 24 untouched.
        q        instead of policy: a float tensor [L*G*G, A] of action values, reduced on the device by greedy_table().
        epsilon  exploration rate in [0, 1]: with that probability (in steps of 2**-32) the step takes a uniform action
                 (0-3 for v1, 0-24 for v2/v4), drawn by Philox from (seed, env, epoch); 0 draws nothing.
        Returns what rollout() returns -- the final (obs, reward, done), with trajectory=True also every stream's rows --
        and then, with trajectory=True, actions_t and key_t int32[T,N] (the caller's, or allocated).  obs_every=k >= 1
        records into obs_t as rollout() does.  The epoch advances by T whether or not auto_reset is set: exploration
        consumes epochs too.  Not for v5/v6 (their closed loop needs two tables), nor with a device-resident epoch (under
        stream capture: the host's epoch would be frozen into the graph)."""
        if self._two_level:
            raise ValueError("rollout_policy() is not available for v5/v6: their two-level step needs two tables")
        T = self._steps(T)
        _tables.exactly_one("rollout_policy()", policy=policy, q=q)
        eps = _abi.epsilon_u32(epsilon)
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("rollout_policy() is not available with a device-resident epoch (under stream capture)")
        policy = _tables.greedy_policy(policy, q, self.n_layouts * self.grid * self.grid, self.device,
                                       "L=%d, G=%d" % (self.n_layouts, self.grid))
        k = self._recording(T, obs_every, obs_t)
        return self._launch_closed("rollout_policy()", "lmaze_foveal_rollout_policy", (policy.data_ptr(), eps), T, k, obs_t,
                                   trajectory, actions_t, key_t, streams=2 if self.variant == "v1" else 1, auto_reset=auto_reset)

    def rollout_sample(self, T, probs=None, logits=None, temperature=1.0, thresholds=None, auto_reset=True, trajectory=False,
                       actions_t=None, key_t=None, obs_t=None, obs_every=None):
        """T steps in ONE launch with a categorical table policy inside the kernel (include/lmaze.h
        lmaze_foveal_rollout_sample; v1, v2, v4): every env-step draws its action from the distribution of its key = layout
        row * G*G + ball_x * G + ball_y (state_keys()).  With S = L*G*G keys and A = 4 (v1) or 25 (v2/v4) actions, exactly one of
        probs       float device tensor [S, A] of non-negative weights, converted by _abi.sampling_thresholds(probs, actions=A);
        logits      float device tensor [S, A]: sampling_thresholds(softmax(logits.double() / temperature)), temperature > 0
                    (a Boltzmann policy);
        thresholds  the table itself, uint32 (or int32, the same bits) device tensor, contiguous and 16-byte aligned: [S, 4]
                    for v1 (c0 <= c1 <= c2 and a reserved word, the grid envs' format), [S, 24] for v2/v4.
        The action is the number of the row's thresholds that one Philox value r per (seed, env, epoch) has reached; a
        cumulative probability of 1 is stored as 1 - 2**-32, so deterministic policies belong to rollout_policy().  Returns
        what rollout_policy() returns; obs_t / obs_every, the rows and the restrictions (not for v5/v6, not under stream
        capture) are its own too.  The epoch advances by T whether or not auto_reset is set."""
        if self._two_level:
            raise ValueError("rollout_sample() is not available for v5/v6: their two-level step needs two tables")
        T = self._steps(T)
        _tables.exactly_one("rollout_sample()", probs=probs, logits=logits, thresholds=thresholds)
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("rollout_sample() is not available with a device-resident epoch (under stream capture)")
        table = _tables.threshold_table(probs, logits, thresholds, temperature, self.n_layouts * self.grid * self.grid,
                                        4 if self.variant == "v1" else _abi.FOVEA * _abi.FOVEA, self.device,
                                        "L=%d, G=%d" % (self.n_layouts, self.grid))
        k = self._recording(T, obs_every, obs_t)
        return self._launch_closed("rollout_sample()", "lmaze_foveal_rollout_sample", (table.data_ptr(),), T, k, obs_t,
                                   trajectory, actions_t, key_t, streams=2 if self.variant == "v1" else 1, auto_reset=auto_reset)

    def rollout_hier_policy(self, T, controller=None, controller_q=None, planner=None, planner_q=None, epsilon=0.0,
                            planner_epsilon=0.0, controller_key="offset", trajectory=False, actions_t=None, key_t=None,
                            goals_t=None, goal_key_t=None, obs_t=None, obs_local_t=None, obs_every=None):
        """v5/v6: T two-level steps (hier_step) in ONE launch with BOTH policies inside the kernel (include/lmaze.h
        lmaze_v5_rollout_policy): a planner table picks the foveal goal of the envs that enter a step done or locally done,
        a controller table the action of every env; no action or goal tensors, no per-step launches.
        planner         uint8 device tensor of L*G*G entries: the goal id (0..24; above: the plannerStep is skipped) of every
                        planner key = state_keys();  planner_q instead: a float tensor [L*G*G, 25], reduced by greedy_table()
        controller      uint8 device tensor, the action id (0..3; above: no move) of every controller key = controller_keys():
                        100 entries for controller_key="offset" (the foveal goal's offset from the ball), 100*L*G*G for "cell"
                        (planner key * 100 + offset);  controller_q instead: a float tensor [keys, 4]
        epsilon, planner_epsilon   exploration rates in [0, 1] of the controller (a uniform action 0..3) and of the planner
                        (a uniform goal 0..24), both from one Philox draw per (seed, env, epoch); nothing is drawn when both are 0
        Returns what rollout(actions, goals=) returns -- the final (obs, reward, done), with trajectory=True also reward,
        done, foveal_reward, foveal_done rows -- and then, with trajectory=True, actions_t, key_t, goals_t, goal_key_t
        int32[T,N] (the caller's, or allocated); goals_t / goal_key_t hold -1 where an env did not plan, which
        table_stats() skips.  obs_every=k >= 1 records into obs_t and, optionally, obs_local_t as rollout() does.  The epoch
        advances by T.  Not for v1/v2/v4 (rollout_policy() is theirs), nor under stream capture."""
        if not self._two_level:
            raise ValueError("rollout_hier_policy() is the two-level closed loop of v5/v6; v1/v2/v4 have rollout_policy()")
        T = self._steps(T)
        _tables.exactly_one("rollout_hier_policy()", controller=controller, controller_q=controller_q)
        _tables.exactly_one("rollout_hier_policy()", planner=planner, planner_q=planner_q)
        eps, peps = _abi.epsilon_u32(epsilon), _abi.epsilon_u32(planner_epsilon)
        ck = self._controller_key(controller_key)
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("rollout_hier_policy() is not available with a device-resident epoch (under stream capture)")
        cells, what = self.n_layouts * self.grid * self.grid, "L=%d, G=%d" % (self.n_layouts, self.grid)
        for q, A, name in ((controller_q, 4, "controller_q"), (planner_q, _abi.FOVEA * _abi.FOVEA, "planner_q")):
            if q is not None and not (isinstance(q, torch.Tensor) and q.dim() == 2 and q.shape[1] == A):
                raise ValueError("%s must be a float tensor [keys, %d]" % (name, A))
        controller = _tables.greedy_policy(controller, controller_q, 100 * cells if ck else 100, self.device,
                                           "controller_key=%r, %s" % (controller_key, what))
        planner = _tables.greedy_policy(planner, planner_q, cells, self.device, what)
        k = self._recording(T, obs_every, obs_t, obs_local_t)
        return self._launch_closed("rollout_hier_policy()", "lmaze_v5_rollout_policy",
                                   (controller.data_ptr(), ck, eps, planner.data_ptr(), peps), T, k, obs_t, trajectory, actions_t,
                                   key_t, streams=2, obs_local_t=obs_local_t, more=[("goals_t", goals_t), ("goal_key_t", goal_key_t)])

    def rollout_hier_sample(self, T, controller_probs=None, controller_logits=None, controller_thresholds=None, planner_probs=None,
                            planner_logits=None, planner_thresholds=None, temperature=1.0, planner_temperature=None,
                            controller_key="offset", trajectory=False, actions_t=None, key_t=None, goals_t=None, goal_key_t=None,
                            obs_t=None, obs_local_t=None, obs_every=None):
        """v5/v6: T two-level steps (hier_step) in ONE launch with a categorical planner and a categorical controller inside
        the kernel (include/lmaze.h lmaze_v5_rollout_sample): every env that enters a step done or locally done draws its
        foveal goal from the distribution of its planner key = state_keys(), every env its action from the distribution of
        its controller key = controller_keys(controller_key).  With K = 100 ("offset") or 100*L*G*G ("cell") controller keys
        and S = L*G*G planner keys, exactly one per level of
        controller_probs / planner_probs            float device tensors [K, 4] / [S, 25] of non-negative weights, converted by
                                                    _abi.sampling_thresholds(probs, actions=4 | 25);
        controller_logits / planner_logits          float device tensors [K, 4] / [S, 25]: sampling_thresholds(softmax(
                                                    logits.double() / temperature)); the planner's temperature is
                                                    planner_temperature, which defaults to temperature; both > 0;
        controller_thresholds / planner_thresholds  the tables themselves, uint32 (or int32, the same bits) device tensors,
                                                    contiguous and 16-byte aligned: [K, 4] (c0 <= c1 <= c2 and a reserved
                                                    word, the grid envs' format) / [S, 24].
        The goal and the action are the numbers of their row's thresholds that the words r.z and r.x of one Philox draw per
        (seed, env, epoch) have reached: always 0..24 and 0..3, so no plannerStep is skipped and every step moves or hits a
        wall.  Returns what rollout_hier_policy() returns; the rows, obs_t / obs_local_t / obs_every and the restrictions
        (not for v1/v2/v4, not under stream capture) are its own too.  The epoch advances by T."""
        if not self._two_level:
            raise ValueError("rollout_hier_sample() is the two-level closed loop of v5/v6; v1/v2/v4 have rollout_sample()")
        T = self._steps(T)
        _tables.exactly_one("rollout_hier_sample()", controller_probs=controller_probs, controller_logits=controller_logits,
                            controller_thresholds=controller_thresholds)
        _tables.exactly_one("rollout_hier_sample()", planner_probs=planner_probs, planner_logits=planner_logits,
                            planner_thresholds=planner_thresholds)
        ck = self._controller_key(controller_key)
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("rollout_hier_sample() is not available with a device-resident epoch (under stream capture)")
        cells, what = self.n_layouts * self.grid * self.grid, "L=%d, G=%d" % (self.n_layouts, self.grid)
        controller = _tables.threshold_table(controller_probs, controller_logits, controller_thresholds, temperature,
                                             100 * cells if ck else 100, 4, self.device,
                                             "controller_key=%r, %s" % (controller_key, what), prefix="controller_")
        planner = _tables.threshold_table(planner_probs, planner_logits, planner_thresholds,
                                          temperature if planner_temperature is None else planner_temperature, cells,
                                          _abi.FOVEA * _abi.FOVEA, self.device, what, prefix="planner_")
        k = self._recording(T, obs_every, obs_t, obs_local_t)
        return self._launch_closed("rollout_hier_sample()", "lmaze_v5_rollout_sample",
                                   (controller.data_ptr(), ck, planner.data_ptr()), T, k, obs_t, trajectory, actions_t, key_t,
                                   streams=2, obs_local_t=obs_local_t, more=[("goals_t", goals_t), ("goal_key_t", goal_key_t)])

    def _recording(self, T, obs_every, obs_t, obs_local_t=None):
        """A rollout's recording request, checked before anything is launched: k = obs_every with obs_t -- and, v5/v6,
        obs_local_t, optional -- shaped for T steps (_obs_slots); 0 when nothing is to be recorded (obs_every None), where
        there may be nowhere to record to either."""
        if obs_every is None:
            if obs_local_t is not None or (self._two_level and obs_t is not None):
                raise ValueError("obs_t / obs_local_t need obs_every")
            if obs_t is not None:
                raise ValueError("obs_t needs obs_every")
            return 0
        k = self._obs_slots(T, obs_every, obs_t, self.obs)
        if obs_local_t is not None:
            self._obs_slots(T, obs_every, obs_local_t, self.obs_local, name="obs_local_t")
        return k

    def _launch_closed(self, who, entry, table_args, T, k, obs_t, trajectory, actions_t, key_t, streams, auto_reset=None,
                       obs_local_t=None, more=None):
        """The launch of the four closed-loop methods, through _closed_loop: `entry`(params, layouts, *table_args, T, buffers,
        N, [auto_reset,] seed, epoch, env_base, the trajectory rows padded to four, actions_t, key_t, [goals_t, goal_key_t,]
        obs_t, [obs_local_t,] k, stream).  The bracketed ones part the one-level entries (auto_reset) from the two-level
        ones (more = the goal rows, and obs_local_t's slots beside obs_t's)."""
        two_level = more is not None

        def call(rows, p_actions, p_key, slots, goal_rows=()):
            local = obs_local_t.data_ptr() if slots is not None and obs_local_t is not None else None
            return getattr(_abi.lib, entry)(
                self._pp, self._p_layouts, *table_args, T, self._pb, self.num_envs, *(() if two_level else (1 if auto_reset else 0,)),
                self.seed & (2 ** 64 - 1), self._epoch, self.env_base, *(rows + [None] * (4 - len(rows))), p_actions, p_key,
                *goal_rows, slots, *((local,) if two_level else ()), k, self._stream())
        return self._closed_loop(who, entry, call, T, k, obs_t, trajectory, actions_t, key_t, streams=streams, more=more)

    @staticmethod
    def _controller_key(controller_key):
        ck = _abi.controller_key_id(controller_key)
        if ck not in (0, 1):
            raise ValueError("controller_key must be 'offset' or 'cell'")
        return ck

    def controller_keys(self, controller_key="offset"):
        """v5/v6, int32[N]: the controller key of every env's CURRENT state, by the rule the key_t rows of
        rollout_hier_policy() are written with -- d = clamp(fgoal_x - ball_x + 4, 0, 9) * 10 + clamp(fgoal_y - ball_y + 4, 0, 9),
        and for "cell" state_keys() * 100 + d.  Plain torch ops; state_keys() is the planner key."""
        if not self._two_level:
            raise ValueError("controller_keys() is the two-level controller's key: v5/v6 only")
        ck = self._controller_key(controller_key)
        o = (self.fgoal_xy.to(torch.int64) - self.ball_xy.to(torch.int64) + 4).clamp(0, 9)
        d = o[:, 0] * 10 + o[:, 1]
        if ck:
            d = d + self.state_keys().to(torch.int64) * 100
        return d.to(torch.int32).contiguous()

    def state_keys(self):
        """int32[N]: the key of every env's CURRENT state, by the rule the key_t rows of rollout_policy() are written with --
        layout row (clamped to 0..L-1; 0 for v1) * G*G + ball_x * G + ball_y, coordinates clamped onto the grid.  Right after
        a rollout this is gae()'s key_tail.  Plain torch ops on layout_id / ball_xy."""
        G = self.grid
        b = self.ball_xy.clamp(0, G - 1)
        k = b[:, 0] * G + b[:, 1]
        if self.variant != "v1":
            k = k + self.layout_id.clamp(0, self.n_layouts - 1) * (G * G)
        return k.to(torch.int32).contiguous()

    def _step_loop(self, T, launch, rows=None, k=None, obs_t=None, obs_local_t=None):
        """rollout() as T launches: launch(t) queues step t; then its rows of the trajectory are copied out and, every k-th
        step, its observations into their slots."""
        for t in range(T):
            launch(t)
            if rows:
                for r, src in zip(rows, (self.reward, self.done, self.foveal_reward, self.foveal_done)):
                    r[t].copy_(src)
            if k and (t + 1) % k == 0:
                obs_t[(t + 1) // k - 1].copy_(self.obs)
                if obs_local_t is not None:
                    obs_local_t[(t + 1) // k - 1].copy_(self.obs_local)

    def capture_rollout(self, actions, goals=None, auto_reset=False, obs_t=None, obs_local_t=None, obs_every=None):
        """rollout(actions, goals, auto_reset) captured into ONE hipGraph (see VecEnvBase._capture); call .replay().
        The rollout resets envs with auto_reset or with goals (the two-level step).  Recording observations (obs_t /
        obs_every) is not captured: ValueError."""
        if obs_t is not None or obs_local_t is not None or obs_every is not None:
            raise ValueError("capture_rollout() does not record observations: call rollout(obs_t=..., obs_every=...)")
        resets = bool(auto_reset) or goals is not None
        return self._capture(actions.shape[0], resets,
                             lambda: self.rollout(actions, goals=goals, auto_reset=auto_reset, device_epoch=resets))

    # launch policies autotune() tries: LmazeFovealParams.launch_hint = ((chunks per workgroup - 1) << 8) |
    # (envs-per-workgroup code << 4) | workgroups per CU
    CANDIDATES = (0x00, 0x20, 0x26, 0x30, 0x34, 0x35, 0x36, 0x43, 0x40, 0x45, 0x120, 0x220, 0x130, 0x134, 0x140, 0x145)

    def autotune(self, actions, goals=None, auto_reset=False, steps=24, candidates=None, warm=100, rounds=3,
                 placement_trials=0):
        """Pick LmazeFovealParams.launch_hint by timing real steps with HIP events on the caller's own action tensor
        (int32[T,N] on the device, rows cycled; `goals` likewise for the v5/v6 two-level step) -- _tuning.autotune, as
        LmazeVecEnv.autotune: the median of `rounds` interleaved passes, the library default (hint 0) kept unless beaten
        by more than 1.5 %; state, visit maps and the observations are snapshotted and restored, so results are
        unaffected.  The best (envs per workgroup, workgroups per CU) pair moves from device to device -- v2 at 1M envs:
        uncapped 96 us on one box and 102 on the next, 6 per CU 95 and 95, 5 per CU 99 and 90.  placement_trials=K
        (K > 1): the step is first timed (uncapped policy 0x30, the sensitive one) on K - 1 further allocations of the
        observation buffer and the fastest becomes the storage of `self.obs`; where the driver placed the write target is
        worth up to 8 % uncapped and 2-3 % at the tuned cap (tools/placement_pmc.py, LAB_NOTES.md R3.2).
        Returns {hint: ms}."""
        self._check_rows("autotune()", actions, goals)
        if self._two_level and goals is None:
            raise ValueError("v5/v6: autotune() times the two-level step and needs planner goals")
        abase, gbase, stride = actions.data_ptr(), None if goals is None else goals.data_ptr(), self.num_envs * 4
        if self._two_level:
            G = int(goals.shape[0])
            step_row = lambda r: self.hier_step_raw(abase + r * stride, gbase + (r % G) * stride)  # noqa: E731
        else:
            step_row = lambda r: self.step_raw(abase + r * stride, auto_reset=auto_reset)  # noqa: E731
        # the observations too: the tuning steps render into them, and with placement trials self.obs may
        # be another allocation by now -- the caller must see the frame of the restored state
        frames = [f for f in (self.obs, self.obs_local) if f is not None]
        return self._tune(int(actions.shape[0]), step_row, frames, candidates=list(candidates or self.CANDIDATES),
                          default=0, trial_policy=0x30, steps=steps, warm=warm, rounds=rounds,
                          placement_trials=placement_trials)

    def _set_policy(self, hint):
        self.params.launch_hint = int(hint)

    def _set_obs(self, ptr):
        self.bufs.obs = ptr

    def reset(self, mask=None, place=True, seed=None):
        """Masked reset; place=False keeps the caller's ball/goal/layout_id (set_state)."""
        if seed is not None:
            self.seed, self._epoch = int(seed), 0
        m, m_ptr = self._mask_ptr(mask)
        with self._guard():
            rc = _abi.lib.lmaze_foveal_reset(self._pp, self._p_layouts, m_ptr, 1 if place else 0,
                                             self.seed & (2 ** 64 - 1), self._epoch, self.env_base, self._pb,
                                             self.num_envs, self._stream())
        _abi.check("lmaze_foveal_reset", rc)
        self._epoch += 1
        return self.obs

    def set_foveal_goal(self, ij, mask=None):
        """v1 setFovealGoal(i, j) (lmaze_env_v1.py:104-110); ij int[N,2]."""
        t = self._as_i32(ij, 2 * self.num_envs)
        m, m_ptr = self._mask_ptr(mask)
        with self._guard():
            rc = _abi.lib.lmaze_v1_set_foveal_goal(self._pp, self._p_layouts, t.data_ptr(), m_ptr, self._pb,
                                                   self.num_envs, self._stream())
        _abi.check("lmaze_v1_set_foveal_goal", rc)
        return self.obs

    def planner_step(self, goal, mask=None):
        """v5/v6 plannerStep(goal) (lmaze_env_v5.py:158-182); goal int[N] in 0..24.  Returns obs_local."""
        t = self._as_i32(goal, self.num_envs)
        m, m_ptr = self._mask_ptr(mask)
        with self._guard():
            rc = _abi.lib.lmaze_v5_planner_step(self._pp, self._p_layouts, t.data_ptr(), m_ptr, self._pb,
                                                self.num_envs, self._stream())
        _abi.check("lmaze_v5_planner_step", rc)
        return self.obs_local

    def safe_foveal_goal(self):
        """v6 safeFovealGoal() (lmaze_env_v6.py:505-523): int32[N] window cell that is not a wall."""
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        with self._guard():
            rc = _abi.lib.lmaze_v6_safe_foveal_goal(self._pp, self._p_layouts, self.seed & (2 ** 64 - 1), self._epoch,
                                                    self.env_base, self._pb, out.data_ptr(), self.num_envs,
                                                    self._stream())
        _abi.check("lmaze_v6_safe_foveal_goal", rc)
        self._epoch += 1
        return out

    def expanded_local(self):
        """(4,35,35) reference layout of obs_local (lmaze_env_v5.py:373-379)."""
        N, E = self.num_envs, self.expansion
        if self._expanded_local is None:
            self._expanded_local = torch.empty((N, 4, 5 * E, 5 * E), dtype=torch.float32, device=self.device)
        with self._guard():
            rc = _abi.lib.lmaze_expand_planes(self.obs_local.data_ptr(), 4, _abi.FOVEA, E,
                                              self._expanded_local.data_ptr(), N, self._stream())
        _abi.check("lmaze_expand_planes", rc)
        return self._expanded_local

    def set_state(self, **kw):
        for name, src in kw.items():
            self._write_state(name, src)

    def expanded(self, out=None):
        """(C, 5E, 5E) reference layout of the current obs (the x7 loop, lmaze_env_v2.py:197-203)."""
        N, Cn, E = self.num_envs, self.channels, self.expansion
        if out is None:
            if self._expanded is None:
                self._expanded = torch.empty((N, Cn, 5 * E, 5 * E), dtype=torch.float32, device=self.device)
            out = self._expanded
        with self._guard():
            rc = _abi.lib.lmaze_expand_planes(self.obs.data_ptr(), Cn, _abi.FOVEA, E, out.data_ptr(), N, self._stream())
        _abi.check("lmaze_expand_planes", rc)
        return out
