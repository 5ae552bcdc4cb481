// lmaze_foveal_launch.h -- the one launch plan of the foveal kernels and the one launcher of the foveal one-launch rollouts
// (host only).  foveal_plan decides everything a foveal launch decides -- the launch_hint bits, the measured defaults, the
// envs per workgroup and their LDS fallback, the LDS sum and its pad, the block count -- for the step and its sibling modes
// (foveal_kernel, queued by lmaze_foveal.hip) and for the rollouts alike; what sets a caller apart is a FovealForm.
// lmaze_foveal.hip (open loop), lmaze_foveal_policy.hip (epsilon-greedy closed loop), lmaze_foveal_sample.hip (sampling
// closed loop), lmaze_hier_policy.hip (the two-level closed loop of v5/v6) and lmaze_hier_sample.hip (its sampling form) keep
// their rollout kernels and describe
// themselves as a family F, a struct of statics:
//   kKernel            the kernel's name as the describe line prints it
//   kTableLds          bytes of table up to which it is staged in LDS behind the layout characters; 0: the family has no
//                      table, and its describe line no " table=lds|global" suffix
// and, where there is a table,
//   table_bytes(p), staged_lds(base, table)
//                      the table's size, and foveal_lds with a staged table added the way the family's kernels lay it out
//   table(ro)          the FovealPol / FovealSmp / FovealHier / FovealHierSmp of a family's RO, whose in_lds the launcher sets
// or, a family of two tables (kTables == 2; its kernel has one mode, which the describe line does not name),
//   place(p, ro, lds), suffix(staged)
//                      which of its tables are staged (the bits of in_lds), their bytes added to lds the way the family's
//                      kernels lay them out; and the describe line's suffix for those bits
// and in every family
//   exists<VARIANT, EPB, GT, AR, REC>()
//                      the instantiations the family has; no other kernel is instantiated, and a call for one that does not
//                      exist is answered hipErrorInvalidConfiguration
//   launch<VARIANT, EPB, GT, AR>(grid, block, lds, s, a, ro)
//                      queues the family's kernel template, which is overloaded on the type of ro
// The launcher asks the family which tables it stages and for their bytes, plans, and picks the family's instantiation from
// the plan's run-time variant, envs per workgroup, grid side and AR.
#ifndef LMAZE_FOVEAL_LAUNCH_H_
#define LMAZE_FOVEAL_LAUNCH_H_

#include <cstdio>
#include <type_traits>

#include "lmaze_foveal_defs.h"

namespace lmaze {

// What a foveal launch queues (foveal_plan): everything the description and the launch need
struct FovealPlan {
    int variant;           // the kernels' variant: v6 runs v5's
    int mode;              // FovealMode; the rollout kernels run FM_STEP
    int epb;               // envs per workgroup after the hint, the default and the LDS fallback
    int gt;                // the grid side the instantiation is specialised for, 14 / 18, or 0
    bool ar;               // the instantiation with the fused reset (v5/v6: the two-level step)
    int chunks;            // chunks of epb envs a workgroup takes
    int per_cu;            // reported: the workgroups per CU the LDS request asks for, 0 without a cap
    int64_t blocks;
    int block;
    size_t lds0, lds;      // the LDS sum before and after the cap's pad
    int32_t nt;            // what the kernel receives as FovealArgs::nt ...
    int32_t launch_hint;   // ... and as launch_hint: a default the plan substituted stands in it
};

// What sets the callers of foveal_plan apart
struct FovealForm {
    int mode;              // FM_STEP .. FM_PLANNER of foveal_kernel; a rollout: FM_STEP
    bool rollout;          // a one-launch rollout family: size codes 2-4 and defaults of its own, plain stores, and the cap
                           // reported only when the pad took effect (the step reports it whenever it is considered)
    bool v5_64_any_grid;   // rollout: the family has a 64-env form of v5/v6 at grids other than 18
    size_t table_lds;      // rollout: bytes the family's staged tables add to the LDS sum, whatever the envs per workgroup
};

// The plan of a.n > 0 envs; false: the block count is beyond what a launch takes (hipErrorInvalidConfiguration).  The policy
// bits never change results.
static inline bool foveal_plan(const FovealArgs& a, const FovealForm& f, FovealPlan& p) {
    const bool v1 = a.p.variant == LMAZE_VARIANT_V1, v2 = a.p.variant == LMAZE_VARIANT_V2, v4 = a.p.variant == LMAZE_VARIANT_V4;
    const bool v56 = !v1 && !v2 && !v4, step = f.mode == FM_STEP;
    p.variant = v56 ? LMAZE_VARIANT_V5 : a.p.variant;
    p.mode = f.mode;
    p.ar = step && a.auto_reset != 0;
    p.launch_hint = a.p.launch_hint;
    const bool streaming = (size_t)a.n * foveal_channels(p.variant) * W25 * 4 > kFovealStreamBytes;
    if (step && !f.rollout && p.launch_hint == 0 && (!a.auto_reset || v56)) {
        // Default policy of the plain step in the streaming regime (observation larger than the Infinity Cache), as a
        // hint.  Round 2, after workgroups learnt to take several chunks: on a box where every uncapped one-chunk launch of
        // v1 sat at 78.5 us whatever the envs per workgroup (on other boxes 32 envs: 66.8-67.4), 32 envs x 3 chunks ran
        // at 68.0 and x 2 at 68.7; v4 32 x 2 595 against 611; v2 64 envs at 5 workgroups per CU 88.7-89.1 on two
        // boxes against 92-96 uncapped (32 x 2-3: 93-94).
        if (streaming) {
            if (v1) p.launch_hint = 0x220;
            else if (v2) p.launch_hint = 0x35;
            // round 3 (window-only visit map): v4 128 envs per workgroup 305.8 us, 64 envs 311.2 (x 2 chunks 321, at 5 per
            // CU 308.7), 32 envs 406; v5/v6 128 envs 446-449 (x 2 chunks 446), 64 envs 503-511
            // (profiles/r03/foveal_sweep_{a,b}.jsonl, two boxes: v4 128 envs x 2 chunks 296.0 / 297.9 us, x 1 304-307, 64 x 2
            // 299.7 / 301.3; v5/v6 128 envs 422.0 / 434.7, x 2 chunks 438.7 / 453.0, 64 envs 503-511)
            else if (v4) p.launch_hint = 0x140;
            else p.launch_hint = 0x40;
        }
    }
    if (step && !f.rollout && p.launch_hint == 0 && a.auto_reset && (size_t)a.n * W25 * 4 * 4 > kFovealStreamBytes) {
        // fused reset (v1, v2, v4; one measured size each, below), same sweeps: v1 at 5 workgroups per CU 74.0 / 74.0 us
        // against 74.2 / 76.8 uncapped; v2 two chunks 97.3 / 99.2 against 102.9 / 100.2; v4 two chunks 402-406 against 426-430
        // (foveal_sweep_ar_a.jsonl, once the envs-per-workgroup hints applied to the fused reset too: v4 128 envs 377-378 us
        // against 417 at 64 envs x 2 chunks; v2 128 x 2 97.3 against 99.3; v1 64 envs at 4-5 per CU 72.9-73.0 against 74.0)
        if (v1) p.launch_hint = 0x35;
        else if (v2 || v4) p.launch_hint = 0x140;
    }
    // launch_hint bits 4-7 (step and rollouts): envs per workgroup, 2: 32 ... 5: 256 (the rollouts: ... 4: 128); anything else =
    // the default below
    const int code = (p.launch_hint >> 4) & 15;
    if (f.rollout && v56 && a.p.grid != 18 && !f.v5_64_any_grid) {
        // v5/v6 at grids other than 18 exist at 32 envs per workgroup only (lmaze_foveal.hip FovealOpen::exists), in a family
        // that has no larger form there
        p.epb = 32;
    } else if (step && code >= 2 && code <= (f.rollout ? 4 : 5)) {
        p.epb = 8 << code;
    } else if (f.rollout) {
        // Default: the workgroup runs T steps of its chunk, so a launch is as many rounds of set-up + T steps as it has
        // chunks per CU; small batches want many small chunks to cover the CUs, large ones the step's sizes
        // (tools/bench_foveal_rollout.py: 4 096-65 536 envs 2.0-4.4 us per step for v1/v2 against 7.0-9.5 as T launches).  v1
        // in the streaming regime: 128 envs per workgroup, 60.6 / 61.4 us (plain / fused, 1M envs, T = 64) against 79.8 / 77.6
        // at 64 envs, 68.1 / 76.0 at 32 and 72.9 / 74.3 as T step launches; v2 fused 70.3 us (T = 256) against 97.6 at 64 envs
        // and 109.9 as T launches, 72.1 / 95.8 / 101.7 at T = 64; v4 fused 299-315 us at 64 or 128 alike, 342-346 as T launches
        // (three interleaved rounds each; all measured on the open loop, the closed loops take its choice)
        p.epb = a.n <= (int64_t)32 * 1024 ? 32 : (!v56 && streaming ? 128 : 64);
    } else {
        // Defaults, measured at 1M envs with a fresh action row per step (tools/foveal_hint_study.py, tools/foveal_decompose.py;
        // us per step, envs per workgroup 32 / 64 / 128 / 256, round 2, after the render went to bit strings):
        //   v1 (400 B of observation per env)  83 / 78-79 / 84 / 87;  64 envs at 5 workgroups per CU: 73.6-73.7 on three boxes
        //   v2 (500 B)                        119 / 94-96 / 98-104 / 100-106; the cap is flat or worse
        // The bare store loop of these kernels (no set-up, no phase 1) takes 88-93 us on v2 and 72-77 us on v1 whatever
        // the chunk size and the cap: the kernels sit within 3-5 % of what their write pattern -- every workgroup streaming
        // a private, env-aligned chunk -- reaches on this memory system (tools/wbench.hip: 6.1 TB/s for 32-KiB private
        // chunks against 6.9 for a fill in which consecutive workgroups write consecutive 4-KiB pieces).
        // After the set-up went to one barrier with ballot-built row masks (cheap enough for small workgroups), re-measured on
        // two boxes: v1 32 envs per workgroup, uncapped 66.8-67.2 us (0.89 of peak; 64 x 4-5 per CU 71-73, 16 envs 105);
        // v4 32 envs 589-652 against 600-675 with 64 on the same boxes; v2 and v5 stay at 64 (32: 102 / 487 against 88-92 / 441).
        p.epb = 64;
        if (step && !a.auto_reset && v1) p.epb = 32;
        if (step && a.auto_reset && v2) p.epb = 256;
        // 32 envs per workgroup: 41 KiB of visit maps streamed + 22 KiB of observation written
        if (step && !a.auto_reset && v4) p.epb = 32;
    }
    // envs per workgroup is a performance knob: a size whose LDS (the staged tables included) does not fit the device falls
    // back to the next smaller one instead of failing the launch (v4-v6 at 256 envs: 164 KiB)
    while (p.epb > 32 && foveal_lds(p.variant, a.p, p.epb) + f.table_lds > lds_limit()) p.epb /= 2;
    p.lds0 = foveal_lds(p.variant, a.p, p.epb) + f.table_lds;
    // launch_hint bits 8-9 (plain and fused step, rollouts): chunks of epb envs per workgroup - 1 (more than 4, or 16-env
    // chunks: slower)
    p.chunks = step ? ((p.launch_hint >> 8) & 3) + 1 : 1;
    p.blocks = ((a.n + p.epb - 1) / p.epb + p.chunks - 1) / p.chunks;
    p.block = LMAZE_BLOCK;
    // the rollouts store plainly: a chunk's observation is rewritten every step, the lines stay in L2
    p.nt = !f.rollout && streaming && !LMAZE_XP(a, 2);
    // launch_hint bits 0-3 (step and rollouts): at most that many workgroups resident per CU, by padding the dynamic LDS (160
    // KiB per CU), as the step kernel does in its streaming regime (lmaze_step.hip step_plan); 0 = no cap
    const int per_cu = p.launch_hint & 15;
    p.lds = step ? lds_for_cap(p.lds0, per_cu) : p.lds0;
    if (f.rollout) p.per_cu = p.lds > p.lds0 ? per_cu : 0;
    else p.per_cu = step && per_cu >= 1 && per_cu <= 8 && p.lds > (size_t)p.epb * 64 ? per_cu : 0;
    // GT 14 and 18 for every foveal_kernel; the rollouts 14 (v1) or 18 (v2, v4, v5/v6) only
    if (f.rollout) p.gt = a.p.grid == (v1 ? 14 : 18) ? a.p.grid : 0;
    else p.gt = a.p.grid == 18 || a.p.grid == 14 ? a.p.grid : 0;
    return grid_ok(p.blocks);
}

// tables a family stages by a placement of its own: 2 where it says so (kTables), else its one table or none
template <class F, class = void>
struct family_tables_of { static constexpr int value = F::kTableLds > 0 ? 1 : 0; };
template <class F>
struct family_tables_of<F, std::void_t<decltype(F::kTables)>> { static constexpr int value = F::kTables; };
template <class F>
constexpr int family_tables() { return family_tables_of<F>::value; }

// The rollout instantiations, X(variant, envs per workgroup); each at GT 14 (v1) or 18 (v2, v4, v5/v6) or 0, AR plain / fused
// (v5/v6: the two-level step), RO plain or recording (a type derived from FovealRollObs), as far as F::exists has them.
#define LMAZE_FOVEAL_ROLLOUT_SIZES(X)                                                                  \
    X(LMAZE_VARIANT_V1, 32) X(LMAZE_VARIANT_V1, 64) X(LMAZE_VARIANT_V1, 128)                           \
    X(LMAZE_VARIANT_V2, 32) X(LMAZE_VARIANT_V2, 64) X(LMAZE_VARIANT_V2, 128)                           \
    X(LMAZE_VARIANT_V4, 32) X(LMAZE_VARIANT_V4, 64) X(LMAZE_VARIANT_V4, 128)                           \
    X(LMAZE_VARIANT_V5, 32) X(LMAZE_VARIANT_V5, 64) X(LMAZE_VARIANT_V5, 128)

template <class F, int VARIANT, int EPB, int GT, bool AR, class RO>
static hipError_t queue_foveal_instance(const FovealPlan& p, hipStream_t s, const FovealArgs& a, const RO& ro) {
    if constexpr (F::template exists<VARIANT, EPB, GT, AR, std::is_base_of<FovealRollObs, RO>::value>()) {
        F::template launch<VARIANT, EPB, GT, AR>(dim3((unsigned)p.blocks), dim3(p.block), p.lds, s, a, ro);
        return hipGetLastError();
    } else {
        return hipErrorInvalidConfiguration;
    }
}

// The family's instantiation a plan names
template <class F, class RO>
static hipError_t queue_foveal_rollout(const FovealPlan& p, hipStream_t s, const FovealArgs& a, const RO& ro) {
#define X(VARIANT, EPB)                                                                                      \
    if (p.variant == VARIANT && p.epb == EPB) {                                                              \
        constexpr int GN = VARIANT == LMAZE_VARIANT_V1 ? 14 : 18;                                            \
        if (p.ar) return p.gt ? queue_foveal_instance<F, VARIANT, EPB, GN, true>(p, s, a, ro)                \
                              : queue_foveal_instance<F, VARIANT, EPB, 0, true>(p, s, a, ro);                \
        return p.gt ? queue_foveal_instance<F, VARIANT, EPB, GN, false>(p, s, a, ro)                         \
                    : queue_foveal_instance<F, VARIANT, EPB, 0, false>(p, s, a, ro);                         \
    }
    LMAZE_FOVEAL_ROLLOUT_SIZES(X)
#undef X
    return hipErrorInvalidConfiguration;
}

template <class F, class RO>
static hipError_t launch_foveal_rollout(const FovealArgs& a, const RO& ro0, hipStream_t s) {
    constexpr bool REC = std::is_base_of<FovealRollObs, RO>::value;
    const bool v1 = a.p.variant == LMAZE_VARIANT_V1, v56 = !v1 && a.p.variant != LMAZE_VARIANT_V2 && a.p.variant != LMAZE_VARIANT_V4;
    // v5/v6: the two-level step of the open loop, of lmaze_hier_policy.hip and of lmaze_hier_sample.hip; the other closed loops have none, and
    // their entry refuses the variants
    if (v56 && !F::template exists<LMAZE_VARIANT_V5, 32, 18, true, false>()) return hipErrorInvalidValue;
    // which tables are staged is a rule, not a measurement; their bytes by the family's own layout (the envs per workgroup
    // add multiples of 16 bytes to the sum, so the bytes a table adds are the same at every size)
    FovealForm f{FM_STEP, true, F::template exists<LMAZE_VARIANT_V5, 64, 0, true, false>(), 0};
    const size_t base = foveal_lds(v56 ? LMAZE_VARIANT_V5 : a.p.variant, a.p, 32);
    size_t with_tables = base;
    int staged = 0;
    if constexpr (family_tables<F>() == 2) {
        staged = F::place(a.p, ro0, with_tables);
    } else if constexpr (F::kTableLds > 0) {
        const size_t table = F::table_bytes(a.p);
        staged = table <= (size_t)F::kTableLds ? 1 : 0;
        if (staged) with_tables = F::staged_lds(base, table);
    }
    f.table_lds = with_tables - base;
    FovealPlan p;
    if (!foveal_plan(a, f, p)) return hipErrorInvalidConfiguration;
    if (a.info) {
        char name[96];
        if constexpr (family_tables<F>() == 2)
            snprintf(name, sizeof(name), "%s<v%d, %d, %d%s>%s", F::kKernel, p.variant, p.epb, p.gt, REC ? ", obs_t" : "", F::suffix(staged));
        else
            snprintf(name, sizeof(name), "%s<v%d, %d, %d, %s%s>%s", F::kKernel, p.variant, p.epb, p.gt,
                     p.ar ? (v56 ? "two-level" : "fused-reset") : "plain", REC ? ", obs_t" : "",
                     F::kTableLds > 0 ? (staged ? " table=lds" : " table=global") : "");
        describe_launch(a.info, name, p.epb, p.per_cu, p.chunks, false, p.blocks, p.block, p.lds);
        return hipSuccess;
    }
    FovealArgs b = a;
    b.nt = p.nt;
    RO ro = ro0;
    if constexpr (F::kTableLds > 0) F::table(ro).in_lds = staged;
    return queue_foveal_rollout<F>(p, s, b, ro);
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
