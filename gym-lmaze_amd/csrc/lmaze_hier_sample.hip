// lmaze_hier_sample.hip -- the SAMPLING closed-loop one-launch rollout of the two-level variants v5 and v6
// (lmaze_v5_rollout_sample, include/lmaze.h), gfx950.
//
// foveal_rollout_kernel's body (lmaze_foveal_body.h) included with LMAZE_FOVEAL_HIER_SAMPLE_SITE defined (its POL switch, 4):
// phase 1 of the two-level step draws the planner's goal from a row of 24 cumulative uint32 thresholds keyed by (layout row,
// ball) and the controller's action from a row of 3 (+ a reserved word) keyed by the foveal goal's offset from the ball
// (controller_key 1: and by the planner key) -- each table staged in LDS behind the layout characters when it is at most
// kFovealSampleLds bytes and read from global memory otherwise -- against the words r.z and r.x of ONE draw per env-step
// (policy_draw, lmaze_common.h; lmaze_hier_sample.h), and stores the action, key, goal and goal-key rows where they are
// produced.  Everything else is the open-loop two-level rollout's.  v6 runs v5's kernels.  A translation unit of its own so that
// the other foveal code objects stay what they were.  Host side: only what sets this family apart (FovealHierSample below);
// the launcher is lmaze_foveal_launch.h's.
#include "lmaze_foveal_launch.h"

namespace lmaze {

// Waves per SIMD asked of the compiler: what the epsilon-greedy twin (lmaze_hier_policy.hip) asks for, in both forms.  Two
// draw words are live across the fused reset instead of four; the planner row's six reads are taken in one group.  DESIGN.md
// 4.5 has the counts.
#ifndef LMAZE_HIER_SAMPLE_WAVES
#define LMAZE_HIER_SAMPLE_WAVES 3
#endif
#ifndef LMAZE_HIER_SAMPLE_WAVES_REC
#define LMAZE_HIER_SAMPLE_WAVES_REC 3
#endif

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(LMAZE_HIER_SAMPLE_WAVES)))
void foveal_hier_sample_kernel(const FovealArgs a, const FovealRollHierSmp ro) {
    constexpr bool ROLL = true, REC = false;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_HIER_SAMPLE_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_HIER_SAMPLE_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(LMAZE_HIER_SAMPLE_WAVES_REC)))
void foveal_hier_sample_kernel(const FovealArgs a, const FovealRollObsHierSmp ro) {
    constexpr bool ROLL = true, REC = true;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_HIER_SAMPLE_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_HIER_SAMPLE_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

// ---- host side: the family of lmaze_foveal_launch.h ----
// v5 (and v6 behind it), the two-level step only: 32 / 64 / 128 envs per workgroup x G = 18 or any x row or recording form.
// Two tables, placed one by one: each at most kTableLds bytes is staged, the controller's first, on the next 16-byte boundary
// behind the layout characters (which the LDS sum already rounds to 16); the staged bytes, multiples of 16, count in the LDS
// sum and so in the halving fallback.
struct FovealHierSample {
    static constexpr const char* kKernel = "foveal_hier_sample_kernel";
    static constexpr int kTableLds = kFovealSampleLds;
    static constexpr int kTables = 2;
    // which tables are staged (FovealHierSmp::in_lds) and the LDS sum with them
    template <class RO>
    static int place(const LmazeFovealParams& p, const RO& ro, size_t& lds) {
        const size_t cbytes = (size_t)hier_sample_controller_bytes(ro.hsmp.controller_key, p.n_layouts, p.grid);
        const size_t pbytes = (size_t)hier_sample_planner_bytes(p.n_layouts, p.grid);
        int staged = 0;
        if (cbytes <= (size_t)kTableLds) staged |= kHierControllerStaged;
        if (pbytes <= (size_t)kTableLds) staged |= kHierPlannerStaged;
        if (staged) lds = ((lds + 15) & ~(size_t)15) + (staged & kHierControllerStaged ? cbytes : 0) + (staged & kHierPlannerStaged ? pbytes : 0);
        return staged;
    }
    static const char* suffix(int staged) {
        static const char* const text[4] = {" controller=global planner=global", " controller=lds planner=global",
                                            " controller=global planner=lds", " controller=lds planner=lds"};
        return text[staged & 3];
    }
    template <class RO>
    static auto& table(RO& ro) { return ro.hsmp; }
    template <int VARIANT, int EPB, int GT, bool AR, bool REC>
    static constexpr bool exists() { return VARIANT == LMAZE_VARIANT_V5 && AR; }
    template <int VARIANT, int EPB, int GT, bool AR, class RO>
    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const FovealArgs& a, const RO& ro) {
        hipLaunchKernelGGL((foveal_hier_sample_kernel<VARIANT, EPB, GT, AR>), grid, block, lds, s, a, ro);
    }
};

hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsHierSmp& ro, bool rec, hipStream_t s) {
    return launch_foveal_rollout_sliced<FovealHierSample, FovealRollHierSmp>(a, ro, rec, s);
}

}  // namespace lmaze
