// lmaze_foveal_policy.hip -- the closed-loop one-launch rollout of the foveal variants v1, v2 and v4
// (lmaze_foveal_rollout_policy, include/lmaze.h), gfx950.
//
// foveal_rollout_kernel's body (lmaze_foveal_body.h) included with LMAZE_FOVEAL_POLICY_SITE defined (its POL switch): phase 1 takes each env's action from a uint8 table
// keyed by (layout row, ball) -- staged in LDS behind the layout characters, or read from global memory when it is larger
// than kFovealPolicyLds -- mixed with the exploration draw of the grid envs' closed loop (policy_draw, lmaze_common.h), and
// stores the action and key rows beside the reward and done rows.  Everything else is the open-loop rollout's.  A
// translation unit of its own so that lmaze_foveal.hip's code objects and compile time stay what they were.  Host side: only
// what sets this family apart (FovealPolicy below); the launcher is lmaze_foveal_launch.h's.
#include "lmaze_foveal_launch.h"

namespace lmaze {

// Waves per SIMD asked of the compiler.  The plain forms ask for 4 as their open-loop twins do and land where their
// registers put them; the recording forms of v1 / v2 ask for one wave less than their twins' 6 (the Philox state and the
// two row values live across the fused reset), and v1's recording form at a grid other than 14 -- which has no open-loop
// twin: it spills at 6 -- asks for 4 instead of being refused.
template <int VARIANT, int GT, bool REC>
constexpr int policy_waves() {
    if (!REC || VARIANT == LMAZE_VARIANT_V4) return 4;
    if (VARIANT == LMAZE_VARIANT_V1 && GT == 0) return 4;
    return 5;
}

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(policy_waves<VARIANT, GT, false>())))
void foveal_rollout_policy_kernel(const FovealArgs a, const FovealRollPol ro) {
    constexpr bool ROLL = true, REC = false;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_POLICY_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_POLICY_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(policy_waves<VARIANT, GT, true>())))
void foveal_rollout_policy_kernel(const FovealArgs a, const FovealRollObsPol ro) {
    constexpr bool ROLL = true, REC = true;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_POLICY_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_POLICY_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

// ---- host side: the family of lmaze_foveal_launch.h ----
// Instantiations, launch_hint bits and defaults as lmaze_foveal_rollout's, for v1, v2 and v4: every form exists, with and
// without recording.  The staged table counts in the LDS sum and so in the halving fallback.
struct FovealPolicy {
    static constexpr const char* kKernel = "foveal_rollout_policy_kernel";
    static constexpr int kTableLds = kFovealPolicyLds;
    static size_t table_bytes(const LmazeFovealParams& p) {
        return (size_t)(p.variant == LMAZE_VARIANT_V1 ? 1 : p.n_layouts) * p.grid * p.grid;                 // one byte per key
    }
    // the staged bytes follow the layout characters at once, rounded up to 16
    static size_t staged_lds(size_t base, size_t table) { return base + ((table + 15) & ~(size_t)15); }
    template <class RO>
    static auto& table(RO& ro) { return ro.pol; }
    template <int VARIANT, int EPB, int GT, bool AR, bool REC>
    static constexpr bool exists() { return VARIANT != LMAZE_VARIANT_V5; }
    template <int VARIANT, int EPB, int GT, bool AR, class RO>
    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const FovealArgs& a, const RO& ro) {
        hipLaunchKernelGGL((foveal_rollout_policy_kernel<VARIANT, EPB, GT, AR>), grid, block, lds, s, a, ro);
    }
};

hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsPol& ro, bool rec, hipStream_t s) {
    return launch_foveal_rollout_sliced<FovealPolicy, FovealRollPol>(a, ro, rec, s);
}

}  // namespace lmaze
