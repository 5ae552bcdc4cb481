// lmaze_offpolicy.hip -- off-policy learning from rollout rows (lmaze_action_probs, lmaze_vtrace, lmaze_vtrace_table:
// include/lmaze.h): the probability with which a table rule records the action of a row, and V-trace over the rows of a
// rollout whose table is no longer the one being learnt.  The arithmetic is lmaze_offpolicy.h's, the text a host program
// compiles too; here are the loads, the stores and the launches.
#include "lmaze_common.h"
#include "lmaze_offpolicy.h"

namespace lmaze {

// The one table row a (key, action) pair needs, as it lies in memory: 16 bytes of a thresholds or q table, or a policy byte in
// .x.  Unconditional, on row 0 for a key outside [0, keys) (keys >= 1), so nothing is read past the table and no load waits
// on a branch.  FORM, one of lmaze_offpolicy.h's three, is the launch's: the kernels are compiled per form, so that no load of
// a block stands behind a test of it.
template <int FORM>
__device__ __forceinline__ uint4 law_row(const ActionLaw& law, uint32_t keys, int32_t key) {
    const uint32_t at = lmaze_law_row(key, keys);
    if (FORM == LMAZE_LAW_POLICY) return make_uint4(law.policy[at], 0u, 0u, 0u);
    return law.rows[at];
}
// ... and the weight of `action` on it; 0 for a key out of range -- one unsigned compare, as table_value's
template <int FORM>
__device__ __forceinline__ uint64_t law_weight(const ActionLaw& law, uint32_t keys, int32_t key, uint4 row, int32_t action) {
    return lmaze_keyed_weight(key, keys, lmaze_action_weight(FORM, row.x, row.y, row.z, row.w, law.epsilon, action));
}

// ------------------------------------------------------------------------------------
// lmaze_action_probs: one lane per sample of the flattened rows, grid-strided so that any m is one launch.  A sample reads
// its key, its action and one table row and stores one float: 12 bytes of rows and a gather.
// ------------------------------------------------------------------------------------
template <int FORM>
__global__ __launch_bounds__(LMAZE_BLOCK) void action_probs_kernel(const ActionProbsArgs a) {
    const int64_t stride = (int64_t)gridDim.x * LMAZE_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x; j < a.m; j += stride) {
        const int32_t key = a.key_t[j], action = a.actions_t[j];
        const uint4 row = law_row<FORM>(a.law, a.keys, key);
        a.prob_t[j] = lmaze_weight_prob(law_weight<FORM>(a.law, a.keys, key, row, action));
    }
}

hipError_t launch_action_probs(const ActionProbsArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    int64_t blocks = (a.m + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (blocks > (int64_t)0xFFFFFF) blocks = 0xFFFFFF;
    const dim3 grid((unsigned)blocks), block(LMAZE_BLOCK);
    if (a.law.form == LMAZE_LAW_THRESHOLDS) hipLaunchKernelGGL(action_probs_kernel<LMAZE_LAW_THRESHOLDS>, grid, block, 0, s, a);
    else if (a.law.form == LMAZE_LAW_POLICY) hipLaunchKernelGGL(action_probs_kernel<LMAZE_LAW_POLICY>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(action_probs_kernel<LMAZE_LAW_Q>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// V-trace over trajectory rows (lmaze_vtrace / lmaze_vtrace_table): advantages_kernel's shape (lmaze_aux.hip) -- one lane per
// env walks t = T-1 .. 0, the rows are loaded ROWS at a time before the dependent chain (acc, vs, and the value of the row
// behind; the rest of a row's arithmetic hangs on loaded values alone) and stored after it.  The table form: a value is
// values[key] for 0 <= key < keys and 0 otherwise, and the ratio of a row comes from the behaviour and the target table at
// (key, action); the key and action loads of a block, then its value gathers and its two table rows per sample are issued
// before the chain, every gather unconditional on an index that is 0 for a key out of range.  The table form holds 32 bytes
// of table rows per sample in flight and walks four rows a block where the rows form walks eight.  A lane reads the rows of
// its own column before it stores them and touches no other column: any output may be any float input row.
// ------------------------------------------------------------------------------------
#define VTRACE_ROWS 8
#define VTRACE_TABLE_ROWS 4
// BFORM, TFORM: the forms of the behaviour and the target table; VTRACE_NO_TABLE for both is the rows form.
#define VTRACE_NO_TABLE (-1)
// One block of a lane's walk: rows t0, t0 - 1 .. of column i, `count` of them (FULL: all ROWS, and nothing asks).  The walk takes
// its ragged block first, so every later one is FULL and runs without a test per row: measured against the form that tests
// every row of every block (advantages_kernel's), T = 64, 18 us against 34 at 65 536 envs and 279 against 293 at 1 M in the
// rows form, 35 against 54 and 915 against 1150 in the table form (profiles/vtrace/) -- at 98-132 VGPRs against 48-68.
template <int BFORM, int TFORM, bool FULL>
__device__ __forceinline__ void vtrace_block(const VtraceArgs& a, size_t n, size_t i, int t0, int count, LmazeVtraceCarry& carry) {
    constexpr bool TABLE = BFORM != VTRACE_NO_TABLE;
    constexpr int ROWS = TABLE ? VTRACE_TABLE_ROWS : VTRACE_ROWS;
    float r[ROWS], v[ROWS], ratio[ROWS], vs[ROWS], pg[ROWS];
    uint8_t d[ROWS];
    size_t at[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) at[j] = (size_t)((FULL || j < count) ? t0 - j : t0) * n + i;     // a row past the block: row t0 again
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        r[j] = a.reward_t[at[j]];
        d[j] = a.done_t[at[j]];
    }
    if constexpr (TABLE) {
        int32_t k[ROWS], act[ROWS];
        uint4 rb[ROWS], rt[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            k[j] = a.key_t[at[j]];
            act[j] = a.actions_t[at[j]];
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            v[j] = table_value(a.values, a.keys, k[j]);
            rb[j] = law_row<BFORM>(a.behaviour, a.keys, k[j]);
            rt[j] = law_row<TFORM>(a.target, a.keys, k[j]);
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            ratio[j] = lmaze_weight_ratio(law_weight<TFORM>(a.target, a.keys, k[j], rt[j], act[j]),
                                          law_weight<BFORM>(a.behaviour, a.keys, k[j], rb[j], act[j]));
    } else {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) v[j] = a.value_t[at[j]];
        if (a.rho_t) {
#pragma unroll
            for (int j = 0; j < ROWS; ++j) ratio[j] = a.rho_t[at[j]];
        } else {
#pragma unroll
            for (int j = 0; j < ROWS; ++j) ratio[j] = 1.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        if (!FULL && j >= count) break;
        lmaze_vtrace_step(r[j], d[j], v[j], ratio[j], a.gamma, a.lambda, a.rho_bar, a.c_bar, &carry, &vs[j], &pg[j]);
    }
    if (a.vs_t) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            if (FULL || j < count) a.vs_t[at[j]] = vs[j];
    }
    if (a.pg_t) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            if (FULL || j < count) a.pg_t[at[j]] = pg[j];
    }
    if (TABLE && a.rho_out_t) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            if (FULL || j < count) a.rho_out_t[at[j]] = ratio[j];
    }
}

template <int BFORM, int TFORM>
__global__ __launch_bounds__(LMAZE_BLOCK) void vtrace_kernel(const VtraceArgs a) {
    constexpr bool TABLE = BFORM != VTRACE_NO_TABLE;
    constexpr int ROWS = TABLE ? VTRACE_TABLE_ROWS : VTRACE_ROWS;
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    float tail;
    if (TABLE) tail = a.key_tail ? table_value(a.values, a.keys, a.key_tail[i]) : 0.0f;
    else tail = a.tail ? a.tail[i] : 0.0f;
    LmazeVtraceCarry carry = {tail, tail, 0.0f};
    int t0 = a.T - 1;
    const int ragged = a.T % ROWS;
    if (ragged) {
        vtrace_block<BFORM, TFORM, false>(a, (size_t)a.n, (size_t)i, t0, ragged, carry);
        t0 -= ragged;
    }
    for (; t0 >= 0; t0 -= ROWS) vtrace_block<BFORM, TFORM, true>(a, (size_t)a.n, (size_t)i, t0, ROWS, carry);
}

template <int BFORM>
static void launch_vtrace_table(const VtraceArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(LMAZE_BLOCK);
    if (a.target.form == LMAZE_LAW_THRESHOLDS) hipLaunchKernelGGL((vtrace_kernel<BFORM, LMAZE_LAW_THRESHOLDS>), grid, block, 0, s, a);
    else if (a.target.form == LMAZE_LAW_POLICY) hipLaunchKernelGGL((vtrace_kernel<BFORM, LMAZE_LAW_POLICY>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((vtrace_kernel<BFORM, LMAZE_LAW_Q>), grid, block, 0, s, a);
}

hipError_t launch_vtrace(const VtraceArgs& a, hipStream_t s) {
    if (a.T <= 0 || a.n == 0) return hipSuccess;
    const int64_t blocks = (a.n + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)blocks);
    if (!a.values) hipLaunchKernelGGL((vtrace_kernel<VTRACE_NO_TABLE, VTRACE_NO_TABLE>), grid, dim3(LMAZE_BLOCK), 0, s, a);
    else if (a.behaviour.form == LMAZE_LAW_THRESHOLDS) launch_vtrace_table<LMAZE_LAW_THRESHOLDS>(a, grid, s);
    else if (a.behaviour.form == LMAZE_LAW_POLICY) launch_vtrace_table<LMAZE_LAW_POLICY>(a, grid, s);
    else launch_vtrace_table<LMAZE_LAW_Q>(a, grid, s);
    return hipGetLastError();
}

}  // namespace lmaze
