"""lmaze_reset_start (include/lmaze.h) restated in numpy, for test_reset_start_cpu.py and test_gpu_reset_start.py: the reset
draw (closed_loop_ref.philox with the reset's counter -- no top bit flipped), k as the count of compares, the v3 goal from
the accepted cells' list and (r.x * count) >> 32, and the exact law of a row.  Importing it needs no GPU."""
import numpy as np

from closed_loop_ref import M32, philox
from occupancy_rollout_ref import spawn_cells

ONE = 1 << 31                      # a complete row ends in this word


def reset_draw(seed, epoch, env_global):
    """The reset draw of (env, epoch), four uint64 arrays of 32-bit words: counter (env lo, env hi, epoch lo, epoch hi), key seed"""
    e = np.asarray(env_global, dtype=np.uint64)
    ep, seed = np.uint64(epoch), np.uint64(seed & (2 ** 64 - 1))
    return philox(e & M32, e >> np.uint64(32), ep & M32, ep >> np.uint64(32), seed & M32, seed >> np.uint64(32))


def ball_draw(seed, epoch, env_global):
    """u int64[n]: the 31-bit draw the ball's row is compared with, r.y >> 1"""
    return (reset_draw(seed, epoch, env_global)[1] >> np.uint64(1)).astype(np.int64)


def count_below(rows, u):
    """k int64[n]: #{ j : rows[i, j] <= u[i] }, whatever the rows hold; rows uint32[n, S] or [S] (the one row of every env)"""
    rows = np.asarray(rows).astype(np.int64) & 0xFFFFFFFF
    return (np.atleast_2d(rows) <= np.asarray(u, np.int64)[:, None]).sum(1)


def row_law(row):
    """int64[S]: the exact mass of every cell of one non-decreasing row, in units of 2^-31"""
    return np.diff(np.r_[0, np.asarray(row).astype(np.int64) & 0xFFFFFFFF])


def v3_goal(lay, rx):
    """The goal cell lmaze_reset draws on one layout uint8[G,G] from r.x (a Python int), -1 when no cell is accepted"""
    cells = spawn_cells(lay, "v3")
    return int(cells[(int(rx) * len(cells)) >> 32]) if len(cells) else -1


def reset_start(variant, lay, thresholds, row_mode, keep_goal, seed, epoch, env_base, st, mask=None):
    """lmaze_reset_start on host state, in place.  lay uint8[G,G] or [n,G,G]; thresholds uint32[S] / [n,S] / [S,S] by row_mode;
    st: dict of ball_xy int32[n,2], goal_xy int32[n,2], step_count int32[n], reward float32[n], done uint8[n].  Returns
    (k, u) of every env, the masked-out ones included."""
    n = st["ball_xy"].shape[0]
    G = lay.shape[-1]
    S = G * G
    thr = np.asarray(thresholds).reshape(-1, S)
    r = reset_draw(seed, epoch, np.arange(n, dtype=np.uint64) + np.uint64(env_base))
    u = (r[1] >> np.uint64(1)).astype(np.int64)
    on = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    if variant == "v3" and not keep_goal:
        shared = spawn_cells(lay, "v3") if lay.ndim == 2 else None
        for i in np.flatnonzero(on):
            cells = shared if shared is not None else spawn_cells(lay[i], "v3")
            if len(cells):
                g = int(cells[(int(r[0][i]) * len(cells)) >> 32])
                st["goal_xy"][i] = (g // G, g % G)
    if row_mode == 0:
        rows = np.broadcast_to(thr[0], (n, S))
    elif row_mode == 1:
        rows = thr
    else:
        g = np.clip(st["goal_xy"].astype(np.int64), 0, G - 1)
        rows = thr[g[:, 0] * G + g[:, 1]]
    k = count_below(rows, u)
    move = on & (k < S)
    st["ball_xy"][move] = np.stack([k[move] // G, k[move] % G], 1).astype(np.int32)
    st["step_count"][on] = 0
    st["reward"][on] = np.float32(-0.0)
    st["done"][on] = 0
    return k, u
