// lmaze_foveal_launch.h -- the one launcher of the foveal one-launch rollouts (host only).  lmaze_foveal.hip (open loop),
// lmaze_foveal_policy.hip (epsilon-greedy closed loop), lmaze_foveal_sample.hip (sampling closed loop) and
// lmaze_hier_policy.hip (the two-level closed loop of v5/v6) keep their kernels
// and describe themselves as a family F; everything a launch decides -- the LDS sum, the launch_hint bits, the default envs per
// workgroup, the describe line -- is decided here, once.  A family is a struct of statics:
//   kKernel            the kernel's name as the describe line prints it
//   kTableLds          bytes of table up to which it is staged in LDS behind the layout characters; 0: the family has no
//                      table, and its describe line no " table=lds|global" suffix
// and, where there is a table,
//   table_bytes<VARIANT>(p), staged_lds(base, table)
//                      the table's size, and foveal_lds with a staged table added the way the family's kernels lay it out
//   table(ro)          the FovealPol / FovealSmp / FovealHier of a family's RO, whose in_lds the launcher sets
// or, a family of two tables (kTables == 2; its kernel has one mode, which the describe line does not name),
//   place<VARIANT>(p, ro, lds), suffix(staged)
//                      which of its tables are staged (the bits of in_lds), their bytes added to lds the way the family's
//                      kernels lay them out; and the describe line's suffix for those bits
// and in every family
//   exists<VARIANT, EPB, GT, AR, REC>()
//                      the instantiations the family has; no other kernel is instantiated, and a call for one that does not
//                      exist is answered hipErrorInvalidConfiguration
//   launch<VARIANT, EPB, GT, AR>(grid, block, lds, s, a, ro)
//                      queues the family's kernel template, which is overloaded on the type of ro
#ifndef LMAZE_FOVEAL_LAUNCH_H_
#define LMAZE_FOVEAL_LAUNCH_H_

#include <cstdio>
#include <type_traits>

#include "lmaze_foveal_defs.h"

namespace lmaze {

// tables a family stages by a placement of its own: 2 where it says so (kTables), else its one table or none
template <class F, class = void>
struct family_tables_of { static constexpr int value = F::kTableLds > 0 ? 1 : 0; };
template <class F>
struct family_tables_of<F, std::void_t<decltype(F::kTables)>> { static constexpr int value = F::kTables; };
template <class F>
constexpr int family_tables() { return family_tables_of<F>::value; }

template <class F, int VARIANT, int EPB, int GT, bool AR, class RO>
static hipError_t queue_foveal_rollout(dim3 grid, dim3 block, size_t lds, hipStream_t s, const FovealArgs& a, const RO& ro) {
    if constexpr (F::template exists<VARIANT, EPB, GT, AR, std::is_base_of<FovealRollObs, RO>::value>()) {
        F::template launch<VARIANT, EPB, GT, AR>(grid, block, lds, s, a, ro);
        return hipGetLastError();
    } else {
        return hipErrorInvalidConfiguration;
    }
}

// Instantiations: envs per workgroup 32 / 64 / 128, GT 14 (v1) or 18 (v2, v4, v5/v6) or 0, AR plain / fused (v5/v6: the
// two-level step), RO plain or recording (a type derived from FovealRollObs), as far as F::exists has them.  The policy bits
// never change results.
template <class F, int VARIANT, int EPB, class RO>
static hipError_t launch_foveal_rollout_one(const FovealArgs& a, const RO& ro0, hipStream_t s) {
    constexpr bool REC = std::is_base_of<FovealRollObs, RO>::value;
    size_t lds0 = foveal_lds<VARIANT>(a.p, EPB);
    int staged = 0;
    if constexpr (family_tables<F>() == 2) {
        staged = F::template place<VARIANT>(a.p, ro0, lds0);   // a rule, not a measurement
    } else if constexpr (F::kTableLds > 0) {
        const size_t table = F::template table_bytes<VARIANT>(a.p);
        staged = table <= (size_t)F::kTableLds ? 1 : 0;        // a rule, not a measurement
        if (staged) lds0 = F::staged_lds(lds0, table);
    }
    // envs per workgroup is a performance knob: a size whose LDS (the staged table included) does not fit the device falls
    // back to the next smaller one instead of failing the launch
    if constexpr (EPB > 32) {
        if (lds0 > lds_limit()) return launch_foveal_rollout_one<F, VARIANT, EPB / 2>(a, ro0, s);
    }
    const int64_t nchunks = (a.n + EPB - 1) / EPB;
    const int m = ((a.p.launch_hint >> 8) & 3) + 1;            // bits 8-9: chunks per workgroup - 1
    const int64_t blocks = (nchunks + m - 1) / m;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    const int per_cu = a.p.launch_hint & 15;                   // bits 0-3: workgroups per CU (lds_for_cap)
    const size_t lds = lds_for_cap(lds0, per_cu);
    FovealArgs b = a;
    b.nt = 0;                 // plain stores: a chunk's observation is rewritten every step, the lines stay in L2
    RO ro = ro0;
    if constexpr (F::kTableLds > 0) F::table(ro).in_lds = staged;
    constexpr int GN = VARIANT == LMAZE_VARIANT_V1 ? 14 : 18;
    const dim3 grid((unsigned)blocks), block(LMAZE_BLOCK);
    if (a.info) {
        char name[96];
        if constexpr (family_tables<F>() == 2)
            snprintf(name, sizeof(name), "%s<v%d, %d, %d%s>%s", F::kKernel, VARIANT, EPB, a.p.grid == GN ? GN : 0, REC ? ", obs_t" : "",
                     F::suffix(staged));
        else
            snprintf(name, sizeof(name), "%s<v%d, %d, %d, %s%s>%s", F::kKernel, VARIANT, EPB, a.p.grid == GN ? GN : 0,
                     a.auto_reset ? (VARIANT == LMAZE_VARIANT_V5 ? "two-level" : "fused-reset") : "plain", REC ? ", obs_t" : "",
                     F::kTableLds > 0 ? (staged ? " table=lds" : " table=global") : "");
        describe_launch(a.info, name, EPB, lds > lds0 ? per_cu : 0, m, false, blocks, LMAZE_BLOCK, lds);
        return hipSuccess;
    }
    if (a.auto_reset) {
        if (a.p.grid == GN) return queue_foveal_rollout<F, VARIANT, EPB, GN, true>(grid, block, lds, s, b, ro);
        return queue_foveal_rollout<F, VARIANT, EPB, 0, true>(grid, block, lds, s, b, ro);
    }
    if (a.p.grid == GN) return queue_foveal_rollout<F, VARIANT, EPB, GN, false>(grid, block, lds, s, b, ro);
    return queue_foveal_rollout<F, VARIANT, EPB, 0, false>(grid, block, lds, s, b, ro);
}

// launch_hint bits 4-7: envs per workgroup, 2: 32, 3: 64, 4: 128; any other code takes the default below
template <class F, int VARIANT, class RO>
static hipError_t launch_foveal_rollout_variant(const FovealArgs& a, const RO& ro, hipStream_t s) {
    // v5/v6 at grids other than 18 exist at 32 envs per workgroup only (lmaze_foveal.hip FovealOpen::exists), in a family
    // that has no larger form there
    if (VARIANT == LMAZE_VARIANT_V5 && a.p.grid != 18 && !F::template exists<LMAZE_VARIANT_V5, 64, 0, true, false>())
        return launch_foveal_rollout_one<F, VARIANT, 32>(a, ro, s);
    switch ((a.p.launch_hint >> 4) & 15) {
        case 2: return launch_foveal_rollout_one<F, VARIANT, 32>(a, ro, s);
        case 3: return launch_foveal_rollout_one<F, VARIANT, 64>(a, ro, s);
        case 4: return launch_foveal_rollout_one<F, VARIANT, 128>(a, ro, s);
        default: break;
    }
    // Default: the workgroup runs T steps of its chunk, so a launch is as many rounds of set-up + T steps as it has
    // chunks per CU; small batches want many small chunks to cover the CUs, large ones the step's sizes
    // (tools/bench_foveal_rollout.py: 4 096-65 536 envs 2.0-4.4 us per step for v1/v2 against 7.0-9.5 as T launches).  v1
    // in the streaming regime: 128 envs per workgroup, 60.6 / 61.4 us (plain / fused, 1M envs, T = 64) against 79.8 / 77.6
    // at 64 envs, 68.1 / 76.0 at 32 and 72.9 / 74.3 as T step launches; v2 fused 70.3 us (T = 256) against 97.6 at 64 envs
    // and 109.9 as T launches, 72.1 / 95.8 / 101.7 at T = 64; v4 fused 299-315 us at 64 or 128 alike, 342-346 as T launches
    // (three interleaved rounds each; all measured on the open loop, the closed loops take its choice)
    if (a.n <= (int64_t)32 * 1024) return launch_foveal_rollout_one<F, VARIANT, 32>(a, ro, s);
    const int C = VARIANT == LMAZE_VARIANT_V1 ? 4 : (VARIANT == LMAZE_VARIANT_V2 ? 5 : 7);
    if (VARIANT != LMAZE_VARIANT_V5 && (size_t)a.n * C * W25 * 4 > kFovealStreamBytes) return launch_foveal_rollout_one<F, VARIANT, 128>(a, ro, s);
    return launch_foveal_rollout_one<F, VARIANT, 64>(a, ro, s);
}

template <class F, class RO>
static hipError_t launch_foveal_rollout(const FovealArgs& a, const RO& ro, hipStream_t s) {
    switch (a.p.variant) {
        case LMAZE_VARIANT_V1: return launch_foveal_rollout_variant<F, LMAZE_VARIANT_V1>(a, ro, s);
        case LMAZE_VARIANT_V2: return launch_foveal_rollout_variant<F, LMAZE_VARIANT_V2>(a, ro, s);
        case LMAZE_VARIANT_V4: return launch_foveal_rollout_variant<F, LMAZE_VARIANT_V4>(a, ro, s);
        default:
            // v5/v6: the two-level step of the open loop and of lmaze_hier_policy.hip; the other closed loops have none, and
            // their entry refuses the variants
            if constexpr (F::template exists<LMAZE_VARIANT_V5, 32, 18, true, false>()) return launch_foveal_rollout_variant<F, LMAZE_VARIANT_V5>(a, ro, s);
            else return hipErrorInvalidValue;
    }
}

// A closed loop's entry fills the recording struct (Rec: FovealRollObs + the table); rec false: the plain kernels, which
// take its FovealRoll and its table alone.
template <class F, class Plain, class Rec>
static hipError_t launch_foveal_rollout_sliced(const FovealArgs& a, const Rec& ro, bool rec, hipStream_t s) {
    if (rec) return launch_foveal_rollout<F>(a, ro, s);
    Plain plain;
    static_cast<FovealRoll&>(plain) = static_cast<const FovealRoll&>(ro);
    F::table(plain) = F::table(ro);
    return launch_foveal_rollout<F>(a, plain, s);
}

}  // namespace lmaze

#endif  // LMAZE_FOVEAL_LAUNCH_H_
