"""ctypes binding of liblmaze_hip.so -- the C ABI declared in include/lmaze.h.

This is the only way the package reaches the kernels, and there is no other compute path:
if the library is missing or does not load, importing this module raises.  Build it with
`python -c "import __graft_entry__ as g; g.build()"` or `make -C gym-lmaze_amd/csrc`.
"""
import ctypes as C
import os

# torch FIRST: its wheel bundles its own libamdhip64 / libhsa-runtime64, and liblmaze_hip.so needs the same
# sonames.  Loaded in this order the dynamic linker gives both ONE HIP runtime (torch's); loaded the other
# way round the process ends up with two HSA runtimes and the second one finds no device (every launch then
# fails with hipErrorNoDevice) -- seen on MI355X with `import gym_lmaze` before `import torch`.
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LMAZE_HIP_LIB") or os.path.join(HERE, "liblmaze_hip.so")   # override: another build of the same ABI

ABI_VERSION = 4
VARIANT_V0, VARIANT_V3 = 0, 3
VARIANT_V1, VARIANT_V2, VARIANT_V4, VARIANT_V5, VARIANT_V6 = 1, 2, 4, 5, 6
FOVEA = 5
LAYOUT_SHARED, LAYOUT_PER_ENV = 0, 1
OBS_BALL, OBS_WALL, OBS_GOAL, OBS_FREE = 1, 2, 4, 8
MAX_GRID, MAX_CHANNELS = 64, 8


class LmazeParams(C.Structure):
    """struct LmazeParams of include/lmaze.h (constants the reference hard-codes in __init__)."""
    _fields_ = [("variant", C.c_int32), ("grid", C.c_int32), ("layout_mode", C.c_int32),
                ("step_limit", C.c_int32), ("reward_wall", C.c_float), ("reward_move", C.c_float),
                ("reward_goal", C.c_float), ("launch_hint", C.c_int32)]


class LmazeFovealParams(C.Structure):
    """struct LmazeFovealParams of include/lmaze.h."""
    _fields_ = [("variant", C.c_int32), ("grid", C.c_int32), ("n_layouts", C.c_int32), ("step_limit", C.c_int32),
                ("foveal_step_limit", C.c_int32), ("reward_wall", C.c_float), ("reward_move", C.c_float),
                ("reward_goal", C.c_float), ("launch_hint", C.c_int32)]


FOVEAL_BUFFER_FIELDS = ("ball_xy", "goal_xy", "fgoal_xy", "layout_id", "step_count", "foveal_step_count",
                        "reward", "foveal_reward", "done", "foveal_done", "visit", "obs",
                        "ball1_xy", "fovea_xy", "last_xy", "foveal_goal", "obs_local", "visit_clock")


class LmazeFovealBuffers(C.Structure):
    """struct LmazeFovealBuffers of include/lmaze.h: device pointers, one element per env."""
    _fields_ = [(n, C.c_void_p) for n in FOVEAL_BUFFER_FIELDS]


class LmazeError(RuntimeError):
    def __init__(self, fn, code):
        self.code = code
        RuntimeError.__init__(self, "%s failed: %d (%s)" % (fn, code, strerror(code)))


def _signatures():
    """name -> argument types of every function include/lmaze.h declares; a family that shares a list is written once.
    tests/test_abi_symbols.py reads the header's prototypes and checks every entry here against them: the return type, the
    number of arguments, each argument's kind and width."""
    vp, i32, i64, u32, u64, f32, text = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_char_p
    P, FP, FB = C.POINTER(LmazeParams), C.POINTER(LmazeFovealParams), C.POINTER(LmazeFovealBuffers)
    draw = [u64, u64, i64]                                    # seed, epoch, env_base
    epochs = draw + [vp, vp, vp]                              # ... epoch_in_dev, epoch_out_dev, stream
    batch = [i64, i32] + draw                                 # n, auto_reset, seed, epoch, env_base
    slots = [vp, i32, vp]                                     # obs_t, obs_every, stream
    law = [vp, vp, u32, vp]                                   # policy, q, epsilon_u32, thresholds: one table, one form

    def same(names, args):
        return dict.fromkeys(names.split(), args)

    def describe(first, flags):
        """(params or counts, n, int32 flags ..., text_host, len)"""
        return first + [i64] + [i32] * flags + [text, i32]

    def grid_rollout(table, rows):
        """(params, layout, actions or table ..., T, state and row pointers ..., n, auto_reset, seed, epoch, env_base -- then
        the stream, or the slots"""
        return [P, vp] + table + [i32] + [vp] * rows + batch

    def foveal_rollout(table, auto_reset, rows):
        """(params, layouts, table ..., T, buffers, n, [auto_reset,] seed, epoch, env_base, row and slot pointers ..., k, stream)"""
        return [FP, vp] + table + [i32, FB, i64] + [i32] * auto_reset + draw + [vp] * rows + [i32, vp]

    return {
        "lmaze_abi_version": [],
        "lmaze_strerror": [C.c_int],
        "lmaze_device_info": [C.c_int, C.POINTER(i32), text, i32],
        **same("lmaze_step_v0 lmaze_step_v3", [P] + [vp] * 8 + [i64, vp]),
        **same("lmaze_step_v0_autoreset lmaze_step_v3_autoreset", [P] + [vp] * 8 + [i64] + epochs),
        "lmaze_step_u8": [P] + [vp] * 9 + [i64, i32] + epochs,
        "lmaze_observe": [P] + [vp] * 4 + [i64, vp],
        "lmaze_observe_u8": [P] + [vp] * 5 + [i64, vp],
        "lmaze_reset": [P, vp, vp] + draw + [vp] * 6 + [i64, vp],
        "lmaze_reset_start": [P, vp, vp, vp, i32, i32] + draw + [vp] * 6 + [i64, vp],
        "lmaze_episode_stats": [vp] * 4 + [f32, i64, vp, vp],
        "lmaze_bandwidth_probe": [vp, vp, i64, vp],
        "lmaze_render_expanded": [vp, i32, i32, C.POINTER(i32), i32, vp, i64, vp],
        "lmaze_expand_planes": [vp, i32, i32, i32, vp, i64, vp],
        # the grid rollouts: actions, or a table in their place
        **same("lmaze_rollout lmaze_rollout_u8", grid_rollout([vp], 9) + [vp]),
        **same("lmaze_rollout_obs lmaze_rollout_obs_u8", grid_rollout([vp], 9) + slots),
        **same("lmaze_rollout_policy lmaze_rollout_policy_u8", grid_rollout([vp, i32, u32], 11) + slots),
        **same("lmaze_rollout_sample lmaze_rollout_sample_u8", grid_rollout([vp, i32], 11) + slots),
        "lmaze_env_rollout_policy": grid_rollout([vp, u32], 11) + slots,
        "lmaze_env_rollout_sample": grid_rollout([vp], 11) + slots,
        "lmaze_env_rollout_qlearn": grid_rollout([vp, f32, f32, u32], 12) + slots,
        # the foveal variants
        "lmaze_foveal_step": [FP, vp, vp, FB, i64, vp],
        "lmaze_foveal_step_autoreset": [FP, vp, vp, FB, i64] + epochs,
        "lmaze_foveal_reset": [FP, vp, vp, i32] + draw + [FB, i64, vp],
        **same("lmaze_v1_set_foveal_goal lmaze_v5_planner_step", [FP, vp, vp, vp, FB, i64, vp]),
        "lmaze_v5_hier_step": [FP, vp, vp, vp, FB, i64] + epochs,
        "lmaze_v6_safe_foveal_goal": [FP, vp] + draw + [FB, vp, i64, vp],
        "lmaze_foveal_visit_bytes": [i32, i64],
        **same("lmaze_foveal_materialise_visit lmaze_foveal_load_visit", [FP, FB, vp, i64, vp]),
        "lmaze_foveal_rollout": [FP, vp, vp, vp, i32, FB] + batch + [vp] * 5,
        "lmaze_foveal_rollout_obs": [FP, vp, vp, vp, i32, FB] + batch + [vp] * 6 + [i32, vp],
        "lmaze_foveal_rollout_policy": foveal_rollout([vp, u32], 1, 7),
        "lmaze_foveal_rollout_sample": foveal_rollout([vp], 1, 7),
        "lmaze_v5_rollout_policy": foveal_rollout([vp, i32, u32, vp, u32], 0, 10),
        "lmaze_v5_rollout_sample": foveal_rollout([vp, i32, vp], 0, 10),
        # learning from rows, and planning
        "lmaze_returns": [vp, vp, vp, f32, vp, i32, i64, vp],
        "lmaze_advantages": [vp] * 4 + [f32, f32, vp, vp, i32, i64, vp],
        "lmaze_advantages_table": [vp] * 5 + [i64, f32, f32, vp, vp, i32, i64, vp],
        "lmaze_table_stats": [vp, vp, vp, i64, i64, i32, vp, vp, vp],
        "lmaze_action_probs": [vp, vp, i64] + law + [i64, vp, vp],
        "lmaze_vtrace": [vp] * 5 + [f32] * 4 + [vp, vp, i32, i64, vp],
        "lmaze_vtrace_table": [vp] * 6 + [i64] + law + law + [f32] * 4 + [vp, vp, vp, i32, i64, vp],
        "lmaze_solve": [P, vp, vp, i64, f32, i32] + [vp] * 7,
        "lmaze_score": [P, vp, vp, i64] + [vp] * 6,
        "lmaze_evaluate": [P, vp, vp, i64, vp, vp, u32, vp, f32, i32, f32] + [vp] * 6,
        "lmaze_occupancy": [P, vp, vp, i64, vp, vp, u32, vp, vp, f32, i32, f32] + [vp] * 6,
        "lmaze_generate": [i32, i64, u64, i64, u32, vp, vp, vp],
        # what a call would launch, as a line of text
        "lmaze_describe_step": describe([P], 2),
        "lmaze_describe_reset_start": describe([P], 1),
        **same("lmaze_describe_rollout lmaze_describe_env_rollout_qlearn", describe([P], 4)),
        **same("lmaze_describe_rollout_policy lmaze_describe_rollout_sample lmaze_describe_env_rollout", describe([P], 5)),
        **same("lmaze_describe_solve lmaze_describe_score lmaze_describe_evaluate lmaze_describe_occupancy", describe([P], 0)),
        "lmaze_describe_foveal_step": describe([FP], 1),
        **same("lmaze_describe_foveal_rollout lmaze_describe_foveal_rollout_policy lmaze_describe_foveal_rollout_sample "
               "lmaze_describe_v5_rollout_policy lmaze_describe_v5_rollout_sample", describe([FP], 3)),
        "lmaze_describe_foveal_rollout_obs": describe([FP], 4),
        "lmaze_describe_table_stats": describe([i64], 1),
        "lmaze_describe_generate": describe([i32], 0),
    }


SIGNATURES = _signatures()
RESTYPES = {"lmaze_strerror": C.c_char_p, "lmaze_foveal_visit_bytes": C.c_int64}      # every other function returns int
SYMBOLS = tuple(SIGNATURES)                                   # every symbol include/lmaze.h declares


def _sources():
    """csrc/*.hip, csrc/*.h and include/lmaze.h: what liblmaze_hip.so is built from."""
    src = os.path.join(HERE, "csrc")
    out = [os.path.join(src, f) for f in sorted(os.listdir(src)) if f.endswith((".hip", ".h"))] if os.path.isdir(src) else []
    hdr = os.path.join(os.path.dirname(HERE), "include", "lmaze.h")
    return out + ([hdr] if os.path.exists(hdr) else [])


def _load():
    if not os.path.exists(LIB_PATH):
        # never built behind the caller's back: under torchrun every rank of a fresh checkout would race to
        # compile and link the same files, and a silent build hides a toolchain problem
        raise ImportError(
            "gym-lmaze_amd: %s is missing. The HIP library is the only compute path (no CPU fallback); "
            "build it with `make -C %s` (hipcc, --offload-arch=gfx950) or `python -c 'import __graft_entry__ as g; "
            "g.build()'`." % (LIB_PATH, os.path.join(HERE, "csrc")))
    if "LMAZE_HIP_LIB" not in os.environ:
        stale = [f for f in _sources() if os.path.getmtime(f) > os.path.getmtime(LIB_PATH)]
        if stale:
            import warnings
            warnings.warn("gym-lmaze_amd: %s is older than %s -- rebuild with `make -C %s`"
                          % (os.path.basename(LIB_PATH), ", ".join(os.path.basename(f) for f in stale),
                             os.path.join(HERE, "csrc")), RuntimeWarning, stacklevel=3)
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = RESTYPES.get(name, C.c_int), argtypes
    if lib.lmaze_abi_version() != ABI_VERSION:
        raise ImportError("liblmaze_hip.so ABI %d != binding %d: rebuild" % (lib.lmaze_abi_version(), ABI_VERSION))
    return lib


lib = _load()


def strerror(code):
    return lib.lmaze_strerror(int(code)).decode("ascii", "replace")


def check(fn, code):
    if code != 0:
        raise LmazeError(fn, code)


def device_info(device=0):
    cu = C.c_int32(0)
    name = C.create_string_buffer(64)
    check("lmaze_device_info", lib.lmaze_device_info(int(device), C.byref(cu), name, 64))
    return {"cu_count": cu.value, "arch": name.value.decode("ascii", "replace")}


def _describe(symbol, *args):
    """The line of the library's `symbol`(*args, text, 256), one of its lmaze_describe_* functions."""
    buf = C.create_string_buffer(256)
    check(symbol, getattr(lib, symbol)(*args, buf, 256))
    return buf.value.decode("ascii", "replace")


def _planes(with_obs):
    return 2 if with_obs == "u8" else (1 if with_obs else 0)


def describe_step(params, n, auto_reset=False, with_obs=True):
    """The kernel / grid / launch policy the library would queue for n envs with these LmazeParams (lmaze_describe_step)."""
    return _describe("lmaze_describe_step", C.byref(params), int(n), 1 if auto_reset else 0, _planes(with_obs))


def describe_rollout(params, n, T, auto_reset=False, with_obs=True, obs_every=None):
    """The kernel / grid / envs per workgroup a grid rollout would queue for n envs and T steps (lmaze_describe_rollout):
    with_obs True / False / "u8" picks lmaze_rollout with obs, without obs, or lmaze_rollout_u8; obs_every (None: the
    plain rollout) the recording entry point with that k."""
    return _describe("lmaze_describe_rollout", C.byref(params), int(n), int(T), 1 if auto_reset else 0, _planes(with_obs),
                     -1 if obs_every is None else int(obs_every))


def describe_foveal_step(params, n, auto_reset=False):
    return _describe("lmaze_describe_foveal_step", C.byref(params), int(n), 1 if auto_reset else 0)


KEY_MODES = {"ball": 0, "goal": 1}
ROW_MODES = {"ball": 0, "env": 1, "goal": 2}                  # lmaze_reset_start's row_mode of reset(key=)


def describe_reset_start(params, n, key="ball"):
    """The kernel / grid / LDS lmaze_reset_start would queue for n envs with these LmazeParams (lmaze_describe_reset_start):
    "reset_start_kernel<v3, rows=goal, table=global> grid=... lds=..."; key "ball" (rows=one), "env" or "goal"; "" for n == 0."""
    return _describe("lmaze_describe_reset_start", C.byref(params), int(n), ROW_MODES[key] if key in ROW_MODES else int(key))


def epsilon_u32(epsilon):
    """The integer lmaze_rollout_policy takes for an exploration rate in [0, 1]: min(floor(eps * 2^32), 2^32 - 1).  Exact:
    a double times a power of two is not rounded."""
    eps = float(epsilon)
    if not 0.0 <= eps <= 1.0:
        raise ValueError("epsilon must be in [0, 1]")
    return min(int(eps * 4294967296.0), 4294967295)


def _describe_closed(symbol, params, n, T, auto_reset, with_obs, obs_every, key):
    return _describe(symbol, C.byref(params), int(n), int(T), 1 if auto_reset else 0, _planes(with_obs), int(obs_every),
                     KEY_MODES[key] if key in KEY_MODES else int(key))


def describe_rollout_policy(params, n, T, auto_reset=True, with_obs=True, obs_every=0, key="ball"):
    """The kernel form / grid / LDS / envs per workgroup a closed-loop rollout would queue (lmaze_describe_rollout_policy):
    with_obs True / False / "u8" as describe_rollout, obs_every >= 0, key "ball" or "goal"."""
    return _describe_closed("lmaze_describe_rollout_policy", params, n, T, auto_reset, with_obs, obs_every, key)


def describe_rollout_sample(params, n, T, auto_reset=True, with_obs=True, obs_every=0, key="ball"):
    """As describe_rollout_policy, for the sampling rollouts (lmaze_describe_rollout_sample): the line names where the
    threshold table lives, table=lds or table=global."""
    return _describe_closed("lmaze_describe_rollout_sample", params, n, T, auto_reset, with_obs, obs_every, key)


ENV_ROLLOUT_FORMS = {"policy": 0, "sample": 1}


def describe_env_rollout(params, n, T, auto_reset=True, with_obs=True, obs_every=0, form="policy"):
    """As describe_rollout_policy, for the rollouts with a table per env (key="env"; lmaze_describe_env_rollout): form
    "policy" (lmaze_env_rollout_policy) or "sample" (lmaze_env_rollout_sample); with_obs True / False -- there are no narrow
    planes.  "rollout_perenv_kernel<v0, policy=env, table=lds, obs_t> T=16 every=3 grid=... lds=... envs_per_workgroup=...":
    table=lds where the workgroup's byte tables are staged behind its layouts, table=global where the env's rows are read
    from global memory (shared layouts, and the sampling form)."""
    return _describe("lmaze_describe_env_rollout", C.byref(params), int(n), int(T), 1 if auto_reset else 0, _planes(with_obs),
                     int(obs_every), ENV_ROLLOUT_FORMS[form] if form in ENV_ROLLOUT_FORMS else int(form))


def describe_env_rollout_qlearn(params, n, T, auto_reset=True, with_obs=True, obs_every=0):
    """As describe_env_rollout, for the Q-learner inside the rollout (lmaze_describe_env_rollout_qlearn):
    "rollout_perenv_kernel<v0, qlearn=env, table=global, obs_t> T=16 every=3 grid=... lds=... envs_per_workgroup=..." -- the
    table is always read and written in global memory."""
    return _describe("lmaze_describe_env_rollout_qlearn", C.byref(params), int(n), int(T), 1 if auto_reset else 0, _planes(with_obs),
                     int(obs_every))


def describe_table_stats(m, keys, actions=4):
    """The kernel / grid / LDS lmaze_table_stats would queue for m samples and a [keys, actions] table
    (lmaze_describe_table_stats): table_stats_kernel<lds> up to 4096 bins, <global> above; "" for m == 0."""
    return _describe("lmaze_describe_table_stats", int(m), int(keys), int(actions))


def describe_solve(params, problems):
    """The kernel form / grid / LDS / problems per workgroup lmaze_solve would queue for `problems` mazes with these LmazeParams
    (lmaze_describe_solve): "solve_kernel<v0, wave, 2> ..." while G*G <= 256, "solve_kernel<v0, workgroup, 4> ..." above; "" for
    no problem."""
    return _describe("lmaze_describe_solve", C.byref(params), int(problems))


def describe_score(params, problems):
    """The kernel form / grid / LDS / problems per workgroup lmaze_score would queue for `problems` tables with these LmazeParams
    (lmaze_describe_score): "score_kernel<v0, wave, 2> ..." while G*G <= 256, "score_kernel<v0, workgroup, 4> ..." above -- the
    plan is lmaze_solve's; "" for no problem."""
    return _describe("lmaze_describe_score", C.byref(params), int(problems))


def describe_evaluate(params, problems):
    """The kernel form / grid / LDS / problems per workgroup lmaze_evaluate would queue for `problems` tables with these
    LmazeParams (lmaze_describe_evaluate): "evaluate_kernel<v0, wave, 2> ..." while G*G <= 256, "evaluate_kernel<v0, workgroup,
    4> ..." above -- the plan is lmaze_solve's; "" for no problem."""
    return _describe("lmaze_describe_evaluate", C.byref(params), int(problems))


def describe_occupancy(params, problems):
    """The kernel form / grid / LDS / problems per workgroup lmaze_occupancy would queue for `problems` tables with these
    LmazeParams (lmaze_describe_occupancy): "occupancy_kernel<v0, wave, 2> ..."; the plan is lmaze_solve's."""
    return _describe("lmaze_describe_occupancy", C.byref(params), int(problems))


def describe_generate(G, mazes):
    """The kernel form / grid / LDS / mazes per workgroup lmaze_generate would queue for `mazes` mazes of G x G cells
    (lmaze_describe_generate): "generate_kernel<wave, 1> ..." while G <= 33, "generate_kernel<workgroup, 4> ..." above (the
    second argument: rooms per lane); "" for no maze."""
    return _describe("lmaze_describe_generate", int(G), int(mazes))


def sampling_thresholds(probs, actions=4):
    """The threshold table lmaze_rollout_sample takes, uint32[S, 4] on probs' device, of a float tensor probs[S, 4] of
    non-negative weights (a row need not sum to 1).  In float64, with this association:
        a0 = p0; a1 = a0 + p1; a2 = a1 + p2; s = a2 + p3;   c_k = min(floor(a_k / s * 2**32 + 0.5), 2**32 - 1)
    and word 3, reserved, is 0.  Action k is then taken with probability (c_k - c_(k-1)) / 2**32, c_(-1) = 0, c_3 = 2**32.
    A cumulative probability of exactly 1 is stored as 1 - 2**-32 (2**32 does not fit the word): a one-hot row lets one
    draw in 2**32 through to action 3 -- deterministic policies belong to rollout_policy().  Refuses negative or
    non-finite entries and rows whose sum is not positive.
    actions=A other than 4 (25: the table lmaze_foveal_rollout_sample takes for v2/v4): probs[S, A], the same definition --
    the running sums a_k = a_(k-1) + p_k by sequential adds, s = a_(A-1) -- and uint32[S, A - 1], no reserved word."""
    A = int(actions)
    if A < 2:
        raise ValueError("actions must be >= 2")
    if not (isinstance(probs, torch.Tensor) and probs.dim() == 2 and probs.shape[1] == A and probs.is_floating_point()):
        raise ValueError("probs must be a float tensor [S, %d]" % A)
    p = probs.detach().to(torch.float64)
    if not bool(torch.isfinite(p).all()) or bool((p < 0).any()):
        raise ValueError("probs must be finite and non-negative")
    sums = [p[:, 0]]
    for k in range(1, A):                          # explicit sequential adds: cumsum's association is not specified
        sums.append(sums[-1] + p[:, k])
    s = sums[-1]
    if not bool(torch.isfinite(s).all()) or bool((s <= 0).any()):
        raise ValueError("every row of probs must have a positive, finite sum")
    c = torch.stack([torch.floor(a / s * 4294967296.0 + 0.5) for a in sums[:-1]] + ([torch.zeros_like(s)] if A == 4 else []), dim=1)
    c = c.clamp_(max=4294967295.0).to(torch.int64)
    return torch.where(c >= 2147483648, c - 4294967296, c).to(torch.int32).view(torch.uint32)   # the same 32 bits


def describe_foveal_rollout(params, n, T, auto_reset=False, two_level=False, obs_every=None):
    """The kernel / grid / launch policy lmaze_foveal_rollout would queue for n envs and T steps; obs_every (None: the plain
    rollout): lmaze_foveal_rollout_obs with that k (lmaze_describe_foveal_rollout_obs)."""
    args = (C.byref(params), int(n), int(T), 1 if auto_reset else 0, 1 if two_level else 0)
    if obs_every is None:
        return _describe("lmaze_describe_foveal_rollout", *args)
    return _describe("lmaze_describe_foveal_rollout_obs", *args, int(obs_every))


def describe_foveal_rollout_policy(params, n, T, auto_reset=False, obs_every=0):
    """The kernel / grid / launch policy lmaze_foveal_rollout_policy would queue for n envs and T steps (obs_every=0: no
    recording), and where its table lives: "... table=lds ..." or "... table=global ..."."""
    return _describe("lmaze_describe_foveal_rollout_policy", C.byref(params), int(n), int(T), 1 if auto_reset else 0, int(obs_every))


def describe_v5_rollout_policy(params, n, T, controller_key=0, obs_every=0):
    """As describe_foveal_rollout_policy, for lmaze_v5_rollout_policy (v5/v6): "foveal_hier_policy_kernel<v5, 32, 18, obs_t>
    controller=lds planner=lds T=...".  controller_key: 0 / "offset" or 1 / "cell"."""
    return _describe("lmaze_describe_v5_rollout_policy", C.byref(params), int(n), int(T), controller_key_id(controller_key),
                     int(obs_every))


def describe_v5_rollout_sample(params, n, T, controller_key=0, obs_every=0):
    """As describe_v5_rollout_policy, for lmaze_v5_rollout_sample (v5/v6): "foveal_hier_sample_kernel<v5, 32, 18, obs_t>
    controller=lds planner=global T=...".  controller_key: 0 / "offset" or 1 / "cell"."""
    return _describe("lmaze_describe_v5_rollout_sample", C.byref(params), int(n), int(T), controller_key_id(controller_key),
                     int(obs_every))


CONTROLLER_KEYS = {"offset": 0, "cell": 1}


def controller_key_id(controller_key):
    """0 / 1 of "offset" / "cell" (the ids themselves pass through)"""
    if isinstance(controller_key, str):
        if controller_key not in CONTROLLER_KEYS:
            raise ValueError("controller_key must be 'offset' or 'cell'")
        return CONTROLLER_KEYS[controller_key]
    return int(controller_key)


def describe_foveal_rollout_sample(params, n, T, auto_reset=False, obs_every=0):
    """As describe_foveal_rollout_policy, for lmaze_foveal_rollout_sample: "foveal_rollout_sample_kernel<...> table=lds ..." or
    "... table=global ..."."""
    return _describe("lmaze_describe_foveal_rollout_sample", C.byref(params), int(n), int(T), 1 if auto_reset else 0, int(obs_every))


def make_params(variant, grid, layout_mode, step_limit, reward_wall, reward_move, reward_goal):
    return LmazeParams(int(variant), int(grid), int(layout_mode), int(step_limit), float(reward_wall),
                       float(reward_move), float(reward_goal), 0)
