// The per-element arithmetic of the off-policy entry points (lmaze_action_probs, lmaze_vtrace, lmaze_vtrace_table:
// include/lmaze.h), shared by the kernels (lmaze_offpolicy.hip) and by a host-compiled program
// (tests/csrc/offpolicy_host.cpp, CPU suite) that runs the same text against a numpy restatement, bit for bit.
//
// What is weighed here is the law of the action a rollout RECORDS: the weight, in units of 2^-34, with which a table rule
// writes the id `action` into actions_t at a row keyed `key`.  No pair is excluded and nothing is renormalised: this is not
// lmaze_evaluate's law conditioned on the usable pairs (lmaze_policy_probs.h), which answers a different question.
#ifndef LMAZE_OFFPOLICY_H_
#define LMAZE_OFFPOLICY_H_

#include "lmaze_learn.h"

// the three forms a table comes in, lmaze_evaluate's
#define LMAZE_LAW_THRESHOLDS 0
#define LMAZE_LAW_POLICY 1
#define LMAZE_LAW_Q 2

// A sampling row (lmaze_rollout_sample): the sampler counts the words its draw reaches, so the row's law is that of its
// three words in ascending order s0 <= s1 <= s2, whatever order they are stored in; with s(-1) = 0 and s3 = 2^32 action a in
// 0..3 weighs 4 (s_a - s_(a-1)), any other id 0.  Word 3 of the row is never looked at.
LMAZE_HD uint64_t lmaze_weight_thresholds(uint32_t c0, uint32_t c1, uint32_t c2, int32_t action) {
    const uint32_t lo = c0 < c1 ? c0 : c1, hi = c0 < c1 ? c1 : c0;
    const uint32_t s0 = lo < c2 ? lo : c2, s2 = hi < c2 ? c2 : hi;
    const uint32_t mid = hi < c2 ? hi : c2, s1 = lo < mid ? mid : lo;
    const uint64_t below = action == 1 ? s0 : (action == 2 ? s1 : (action == 3 ? s2 : 0ull));
    const uint64_t upto = action == 0 ? s0 : (action == 1 ? s1 : (action == 2 ? s2 : 0x100000000ull));
    return (uint32_t)action <= 3u ? 4ull * (upto - below) : 0ull;
}

// An epsilon-greedy entry (lmaze_rollout_policy): e on each of the four moves, and the greedy share 4 (2^32 - e) on the id the
// table holds -- also when that id is above 3, "no move", which the rollout records as it stands.
LMAZE_HD uint64_t lmaze_weight_greedy(uint32_t greedy, uint32_t epsilon_u32, int32_t action) {
    const uint64_t e = epsilon_u32;
    return ((uint32_t)action <= 3u ? e : 0ull) + ((uint32_t)action == greedy ? 4ull * (0x100000000ull - e) : 0ull);
}

// The weight of `action` on one table row in any of the three forms.  w0..w3: the 16 bytes of a thresholds or q row as they
// lie in memory; a policy entry is the byte itself in w0.
LMAZE_HD uint64_t lmaze_action_weight(int form, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t epsilon_u32,
                                      int32_t action) {
    if (form == LMAZE_LAW_THRESHOLDS) return lmaze_weight_thresholds(w0, w1, w2, action);
    uint32_t greedy = w0;
    if (form == LMAZE_LAW_Q) {
        union { uint32_t u[4]; float f[4]; } row;
        row.u[0] = w0; row.u[1] = w1; row.u[2] = w2; row.u[3] = w3;
        int first;
        lmaze_q_first_max(row.f, &first);
        greedy = (uint32_t)first;
    }
    return lmaze_weight_greedy(greedy, epsilon_u32, action);
}

// A key outside [0, keys) weighs 0: ONE unsigned compare, as lmaze_advantages_table's lookup.  The row such a key reads is
// row 0 (keys >= 1) -- never past the table, and no load waits on a branch -- and what it holds is discarded.
LMAZE_HD uint32_t lmaze_law_row(int32_t key, uint32_t keys) { return (uint32_t)key < keys ? (uint32_t)key : 0u; }
LMAZE_HD uint64_t lmaze_keyed_weight(int32_t key, uint32_t keys, uint64_t w) { return (uint32_t)key < keys ? w : 0ull; }

// fl(w): round to nearest, ties to even (w <= 2^34)
LMAZE_HD float lmaze_weight_float(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ull2float_rn(w);
#else
    return (float)w;                  // the default rounding mode: to nearest, ties to even
#endif
}

// p = fl(w) 2^-34: the conversion is the only rounding, the scaling by a power of two is exact (w >= 1 gives 2^-34 or more)
LMAZE_HD float lmaze_weight_prob(uint64_t w) { return lmaze_weight_float(w) * 0x1p-34f; }

// The importance ratio of a row: fl(fl(wt) / fl(wb)), ONE correctly rounded division; 0 where the behaviour table cannot
// have produced the row (wb == 0), whatever the target says.  Equal weights give exactly 1.
LMAZE_HD float lmaze_weight_ratio(uint64_t w_target, uint64_t w_behaviour) {
    if (w_behaviour == 0) return 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(lmaze_weight_float(w_target), lmaze_weight_float(w_behaviour));
#else
    return lmaze_weight_float(w_target) / lmaze_weight_float(w_behaviour);
#endif
}

// What the V-trace walk carries from row t + 1 to row t: the value and the corrected value of the row behind, and
// acc = vs - v of the row behind.  Start: {tail, tail, 0}.
struct LmazeVtraceCarry { float v_next, vs_next, acc_next; };

// One step of V-trace (Espeholt et al. 2018), walking backwards: from a row's reward, done flag, value and UNCLIPPED ratio
// to its corrected value vs and its policy-gradient advantage pg = rho (r + gamma vs_next - v).  Every operation is rounded
// on its own, in this order, never an fma (the pragma, as in lmaze_gae_step; -ffp-contract=off where it is not known).  A done
// row cuts the bootstrap and the trace and adds no "gamma * 0": a -0.0 survives.  A NaN ratio fails both compares and is
// clipped to the bars.
// On-policy (ratio 1, both bars >= 1): rho = 1, c = lambda, gc = fl(gamma lambda) is lmaze_gae_step's gl and delta = td, so
// acc is lmaze_gae_step's advantage and vs lmaze_gae_target in every bit.  The order of the operations is what makes it so.
LMAZE_HD void lmaze_vtrace_step(float r, int done, float v, float ratio, float gamma, float lambda, float rho_bar, float c_bar,
                                LmazeVtraceCarry* carry, float* vs_out, float* pg_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float rho = ratio < rho_bar ? ratio : rho_bar;
    const float cc = ratio < c_bar ? ratio : c_bar;
    const float c = lambda * cc;
    // Both kinds of row in one straight line, the done flag picking between values (a lane's rows do not branch apart, and
    // only `trace` and the two sums behind it wait for the row behind): a done row's target is r itself and its acc is
    // delta itself -- never r + gamma * 0 or delta + 0 -- and what the other side computed is dropped, NaN or not.
    const float boot = gamma * carry->v_next;
    const float tg = done ? r : r + boot;
    const float td = tg - v;
    const float delta = rho * td;
    const float gc = gamma * c;
    const float trace = gc * carry->acc_next;
    const float acc = done ? delta : delta + trace;
    const float qb = gamma * carry->vs_next;
    const float qv = done ? r : r + qb;
    const float vs = acc + v;
    const float qa = qv - v;
    *vs_out = vs;
    *pg_out = rho * qa;
    carry->v_next = v;
    carry->vs_next = vs;
    carry->acc_next = acc;
}

#endif
