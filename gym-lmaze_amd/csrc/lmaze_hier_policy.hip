// lmaze_hier_policy.hip -- the closed-loop one-launch rollout of the two-level variants v5 and v6
// (lmaze_v5_rollout_policy, include/lmaze.h), gfx950.
//
// foveal_rollout_kernel's body (lmaze_foveal_body.h) included with LMAZE_FOVEAL_HIER_SITE defined (its POL switch, 3): phase 1
// of the two-level step takes the planner's goal from a uint8 table keyed by (layout row, ball) and the controller's action
// from a uint8 table keyed by the foveal goal's offset from the ball (controller_key 1: and by the planner key), each staged
// in LDS behind the layout characters when it is at most kFovealPolicyLds bytes and read from global memory otherwise, each
// mixed with two words of ONE exploration draw (policy_draw, lmaze_common.h), and stores the action, key, goal and goal-key
// rows where they are produced.  Everything else is the open-loop two-level rollout's.  v6 runs v5's kernels.  A translation
// unit of its own so that the other foveal code objects stay what they were.  Host side: only what sets this family apart
// (FovealHierPolicy below); the launcher is lmaze_foveal_launch.h's.
#include "lmaze_foveal_launch.h"

namespace lmaze {

// Waves per SIMD asked of the compiler.  The open-loop twin sits at 128 VGPRs, 4 waves; the four draw words, the two keys and
// the row stores of both levels are live across the fused reset and the plannerStep on top of that, so both forms ask for
// one wave less (the project's rule: at most one below the twin).  DESIGN.md 4.5 has the counts.
#ifndef LMAZE_HIER_WAVES
#define LMAZE_HIER_WAVES 3
#endif
#ifndef LMAZE_HIER_WAVES_REC
#define LMAZE_HIER_WAVES_REC 3
#endif

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(LMAZE_HIER_WAVES)))
void foveal_hier_policy_kernel(const FovealArgs a, const FovealRollHier ro) {
    constexpr bool ROLL = true, REC = false;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_HIER_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_HIER_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(LMAZE_HIER_WAVES_REC)))
void foveal_hier_policy_kernel(const FovealArgs a, const FovealRollObsHier ro) {
    constexpr bool ROLL = true, REC = true;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_HIER_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_HIER_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

// ---- host side: the family of lmaze_foveal_launch.h ----
// v5 (and v6 behind it), the two-level step only: 32 / 64 / 128 envs per workgroup x G = 18 or any x row or recording form.
// Two tables, placed one by one: each at most kTableLds bytes is staged, the controller's first; the staged bytes count in the
// LDS sum and so in the halving fallback.
struct FovealHierPolicy {
    static constexpr const char* kKernel = "foveal_hier_policy_kernel";
    static constexpr int kTableLds = kFovealPolicyLds;
    static constexpr int kTables = 2;
    // which tables are staged (FovealHier::in_lds) and the LDS sum with them
    template <class RO>
    static int place(const LmazeFovealParams& p, const RO& ro, size_t& lds) {
        const size_t cbytes = (size_t)hier_controller_bytes(ro.hier.controller_key, p.n_layouts, p.grid);
        const size_t pbytes = (size_t)p.n_layouts * p.grid * p.grid;
        int staged = 0;
        if (cbytes <= (size_t)kTableLds) { staged |= kHierControllerStaged; lds += (cbytes + 15) & ~(size_t)15; }
        if (pbytes <= (size_t)kTableLds) { staged |= kHierPlannerStaged; lds += (pbytes + 15) & ~(size_t)15; }
        return staged;
    }
    static const char* suffix(int staged) {
        static const char* const text[4] = {" controller=global planner=global", " controller=lds planner=global",
                                            " controller=global planner=lds", " controller=lds planner=lds"};
        return text[staged & 3];
    }
    template <class RO>
    static auto& table(RO& ro) { return ro.hier; }
    template <int VARIANT, int EPB, int GT, bool AR, bool REC>
    static constexpr bool exists() { return VARIANT == LMAZE_VARIANT_V5 && AR; }
    template <int VARIANT, int EPB, int GT, bool AR, class RO>
    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const FovealArgs& a, const RO& ro) {
        hipLaunchKernelGGL((foveal_hier_policy_kernel<VARIANT, EPB, GT, AR>), grid, block, lds, s, a, ro);
    }
};

hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsHier& ro, bool rec, hipStream_t s) {
    return launch_foveal_rollout_sliced<FovealHierPolicy, FovealRollHier>(a, ro, rec, s);
}

}  // namespace lmaze
