// The selection rule of the closed-loop foveal rollout (lmaze_foveal_rollout_policy: include/lmaze.h), shared by the kernel
// (lmaze_foveal_body.h) and by a host-compiled program (tests/csrc/foveal_select_host.cpp, CPU suite) that runs the same
// text against a numpy restatement.
#ifndef LMAZE_FOVEAL_SELECT_H_
#define LMAZE_FOVEAL_SELECT_H_

#include <stdint.h>

#ifndef LMAZE_HD
#ifdef __HIPCC__
#define LMAZE_HD __host__ __device__ __forceinline__
#else
#define LMAZE_HD static inline
#endif
#endif

LMAZE_HD int lmaze_foveal_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The key of an env: the layout row its step uses and its ball, each clamped into the table (L = 1 for v1).
LMAZE_HD int lmaze_foveal_key(int lid, int bx, int by, int G, int L) {
    return lmaze_foveal_clamp(lid, 0, L - 1) * G * G + lmaze_foveal_clamp(bx, 0, G - 1) * G + lmaze_foveal_clamp(by, 0, G - 1);
}

// One of A actions from a 32-bit draw: floor(ry * A / 2^32).  A = 4: ry >> 30, the grid envs' rule.
LMAZE_HD int lmaze_foveal_explore(uint32_t ry, int A) { return (int)(((uint64_t)ry * (uint64_t)(uint32_t)A) >> 32); }

// The action taken: the table's id, or -- with probability epsilon / 2^32 -- a uniform one.  epsilon == 0 ignores the draw.
LMAZE_HD int lmaze_foveal_choose(int greedy, uint32_t rx, uint32_t ry, uint32_t epsilon, int A) {
    return (epsilon != 0u && rx < epsilon) ? lmaze_foveal_explore(ry, A) : greedy;
}

#endif  // LMAZE_FOVEAL_SELECT_H_
