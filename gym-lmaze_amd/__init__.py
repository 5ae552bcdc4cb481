"""gym-lmaze_amd: MI355X-native batched L-maze step path (drop-in for gkm2708/gym-lmaze).

The directory name carries a hyphen, so import it with
    importlib.import_module("gym-lmaze_amd")
or, as a user of the reference would, through the alias package `gym_lmaze`
(`import gym_lmaze; gym_lmaze.make("lmaze-v0")`, `from gym_lmaze.envs import LmazeEnv`).

Importing this package loads liblmaze_hip.so and raises if it is missing: the HIP kernels
are the only implementation of the step path.
"""
from . import _abi  # noqa: F401  (fails loudly when the HIP library is absent)
from . import layouts  # noqa: F401
from .compat import make, register, registered_ids  # noqa: F401
from .envs import LmazeEnv, LmazeEnv_v3  # noqa: F401
from .foveal_env import FOVEAL_VARIANTS, LmazeFovealVecEnv  # noqa: F401
from .foveal_envs import LmazeEnv_v1, LmazeEnv_v2, LmazeEnv_v4, LmazeEnv_v5, LmazeEnv_v6  # noqa: F401
from .offpolicy import TablePolicy, action_probs, table_policy, vtrace  # noqa: F401
from .sharding import gather_over_ranks, max_over_ranks, shard_range, sum_over_ranks  # noqa: F401
from .vec_env import (VARIANTS, EvaluatedTables, LmazeVecEnv, OccupancyTables, ScoredTables, SolvedTables, discounted_returns,  # noqa: F401
                      distance_band, evaluate_tables, gae, occupancy_tables, reset_distribution, score_tables, solve_tables, start_thresholds, table_means, table_stats)

__all__ = ["LmazeVecEnv", "LmazeFovealVecEnv", "FOVEAL_VARIANTS", "LmazeEnv", "LmazeEnv_v1", "LmazeEnv_v2", "LmazeEnv_v3", "LmazeEnv_v4", "LmazeEnv_v5", "LmazeEnv_v6", "VARIANTS", "discounted_returns", "distance_band", "evaluate_tables", "EvaluatedTables", "gae", "layouts", "make", "occupancy_tables", "OccupancyTables", "register", "reset_distribution",
           "registered_ids", "score_tables", "ScoredTables", "shard_range", "solve_tables", "SolvedTables", "start_thresholds", "table_means", "table_stats",
           "action_probs", "table_policy", "TablePolicy", "vtrace"]
