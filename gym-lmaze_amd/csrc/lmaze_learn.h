// The per-element arithmetic of the learner-side kernels (lmaze_advantages, lmaze_table_stats: include/lmaze.h), shared by
// the kernels (lmaze_aux.hip) and by a host-compiled program (tests/csrc/learn_host.cpp, CPU suite) that runs the same text
// against a numpy restatement, bit for bit.  And of the learner inside the rollout (lmaze_env_rollout_qlearn, lmaze_step.hip;
// tests/csrc/qlearn_host.cpp).
#ifndef LMAZE_LEARN_H_
#define LMAZE_LEARN_H_

#include <math.h>
#include <stdint.h>

#ifndef LMAZE_HD
#ifdef __HIPCC__
#define LMAZE_HD __host__ __device__ __forceinline__
#else
#define LMAZE_HD static inline
#endif
#endif

// One step of GAE(lambda), walking backwards: the advantage of row t from its reward, done flag and value, the value of
// row t + 1 and the advantage of row t + 1.  gl = gamma * lambda, one float32 product the caller computed once.  Every
// operation is rounded on its own: as in returns_step (lmaze_aux.hip) the operators stand under a pragma that takes the
// contraction licence away, never an fma.  A compiler that does not know the pragma builds this with -ffp-contract=off.
// A done row restarts both the bootstrap and the trace: r - v, written so (no "+ gamma * 0", which would turn a -0.0 into +0.0).
LMAZE_HD float lmaze_gae_step(float r, int done, float v, float v_next, float gamma, float gl, float adv_next) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (done) return r - v;
    const float boot = gamma * v_next;
    const float target = r + boot;
    const float delta = target - v;
    const float trace = gl * adv_next;
    return delta + trace;
}

// the value target of a row: advantage + value, one rounding
LMAZE_HD float lmaze_gae_target(float adv, float v) { return adv + v; }

// The arithmetic of the in-kernel Q-learner (lmaze_env_rollout_qlearn; tests/csrc/qlearn_host.cpp runs the same text on the
// host).  The same rule as lmaze_gae_step: every operation rounded on its own, never an fma.
// The greedy action of a row and its value: the FIRST maximum, by a strict > from a = 0 on -- solve_cell's rule
// (lmaze_solve.hip).  A NaN never wins a compare, and nothing beats a NaN in q[0]: such a row keeps action 0 and returns the NaN.
LMAZE_HD float lmaze_q_first_max(const float q[4], int* action) {
    float best = q[0];
    int act = 0;
    for (int a = 1; a < 4; ++a)
        if (q[a] > best) { best = q[a]; act = a; }
    *action = act;
    return best;
}

// The one-step target: r for a transition that ended the episode, else r + gamma * v_next -- the product rounded, then the
// sum.  A done row is r itself (no "+ gamma * 0": a -0.0 stays -0.0, an infinite v_next makes no NaN).
LMAZE_HD float lmaze_q_target(float r, int done, float gamma, float v_next) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (done) return r;
    const float boot = gamma * v_next;
    return r + boot;
}

// q(s, a) += alpha * (target - q(s, a)) in three roundings; *delta: the TD error target - q(s, a)
LMAZE_HD float lmaze_q_update(float q_sa, float alpha, float target, float* delta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    *delta = target - q_sa;
    const float step = alpha * *delta;
    return q_sa + step;
}

LMAZE_HD uint32_t lmaze_learn_bits(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }

// A weight lmaze_table_stats accumulates: finite and |w| < 2^31 (0x4f000000 is 2^31; NaN and inf carry a larger exponent
// field).  Integer compare on the bit pattern: the same answer whatever the device does with denormals.
LMAZE_HD int lmaze_q24_ok(float w) { return (lmaze_learn_bits(w) & 0x7fffffffu) < 0x4f000000u; }

// q(w): w * 2^24 rounded to the nearest integer, ties to even.  The product is a scaling by a power of two, exact in
// float32 (|w| < 2^31: below 2^55, no overflow; a denormal w gives less than 2^-102, which rounds to 0 flushed or not), so
// the conversion is the only rounding.  Requires lmaze_q24_ok(w).
LMAZE_HD int64_t lmaze_q24(float w) {
    const float p = w * 16777216.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    return (int64_t)__float2ll_rn(p);
#else
    return (int64_t)llrintf(p);       // the default rounding mode: to nearest, ties to even
#endif
}

// the bin of a sample, or -1 for one that is skipped: key outside [0, keys) or action outside [0, actions), each ONE
// unsigned compare
LMAZE_HD int32_t lmaze_table_bin(int32_t key, int32_t action, uint32_t keys, uint32_t actions) {
    if ((uint32_t)key >= keys || (uint32_t)action >= actions) return -1;
    return (int32_t)((uint32_t)key * actions + (uint32_t)action);
}

#endif
