// The sampling rule of the closed-loop foveal rollout (lmaze_foveal_rollout_sample: include/lmaze.h), shared by the kernel
// (lmaze_foveal_body.h through foveal_smp_action, lmaze_foveal_defs.h) and by a host-compiled program
// (tests/csrc/foveal_sample_host.cpp, CPU suite) that runs the same text against a numpy restatement.
#ifndef LMAZE_FOVEAL_SAMPLE_H_
#define LMAZE_FOVEAL_SAMPLE_H_

#include <stdint.h>

#ifndef LMAZE_HD
#ifdef __HIPCC__
#define LMAZE_HD __host__ __device__ __forceinline__
#else
#define LMAZE_HD static inline
#endif
#endif

// Words of thresholds a key's row holds for A actions: A - 1 compared, and for A = 4 a reserved fourth (the grid format).
LMAZE_HD int lmaze_foveal_sample_row_words(int A) { return A == 4 ? 4 : A - 1; }

// The action of a draw r against the first n = A - 1 words of a row: how many of them r has reached, unsigned.  Nothing
// is validated: a row that is not monotone yields what this sum gives, which a binary search would not.
LMAZE_HD int lmaze_foveal_sample_action(const uint32_t* c, int n, uint32_t r) {
    int act = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < n; ++k) act += (r >= c[k]) ? 1 : 0;
    return act;
}

#endif  // LMAZE_FOVEAL_SAMPLE_H_
