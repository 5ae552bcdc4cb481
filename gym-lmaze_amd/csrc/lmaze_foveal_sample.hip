// lmaze_foveal_sample.hip -- the sampling closed-loop one-launch rollout of the foveal variants v1, v2 and v4
// (lmaze_foveal_rollout_sample, include/lmaze.h), gfx950.
//
// foveal_rollout_kernel's body (lmaze_foveal_body.h) included with LMAZE_FOVEAL_SAMPLE_SITE defined (POL = 2): phase 1 draws
// each env's action from the categorical distribution of its key -- a row of cumulative uint32 thresholds (3 for v1, 24 for
// v2/v4) staged in LDS behind the layout characters, or read from global memory when the table is larger than
// kFovealSampleLds, compared against one word of the closed loop's draw (policy_draw, lmaze_common.h) -- and stores the action
// and key rows beside the reward and done rows.  Everything else is the open-loop rollout's.  A translation unit of its own:
// lmaze_foveal.hip's and lmaze_foveal_policy.hip's code objects stay what they were.  Host side: only what sets this family
// apart (FovealSample below); the launcher is lmaze_foveal_launch.h's.
#include "lmaze_foveal_launch.h"

namespace lmaze {

// Waves per SIMD asked of the compiler: what the epsilon-greedy twins of lmaze_foveal_policy.hip ask for (policy_waves
// there), with one exception.  v1's plain recording form at 32 envs and G = 14 needs 97 VGPRs, one more than 5 waves leave it
// (it spilled 12 bytes per lane when asked for 5): it asks for 4 and runs one wave below its twin.
template <int VARIANT, int EPB, int GT, bool AR, bool REC>
constexpr int sample_waves() {
    if (!REC || VARIANT == LMAZE_VARIANT_V4) return 4;
    if (VARIANT == LMAZE_VARIANT_V1 && (GT == 0 || (EPB == 32 && !AR))) return 4;
    return 5;
}

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(sample_waves<VARIANT, EPB, GT, AR, false>())))
void foveal_rollout_sample_kernel(const FovealArgs a, const FovealRollSmp ro) {
    constexpr bool ROLL = true, REC = false;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_SAMPLE_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_SAMPLE_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(sample_waves<VARIANT, EPB, GT, AR, true>())))
void foveal_rollout_sample_kernel(const FovealArgs a, const FovealRollObsSmp ro) {
    constexpr bool ROLL = true, REC = true;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#define LMAZE_FOVEAL_SAMPLE_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_SAMPLE_SITE
#undef LMAZE_FOVEAL_BODY_SITE
}

// ---- host side: the family of lmaze_foveal_launch.h ----
// Instantiations, launch_hint bits and defaults as lmaze_foveal_rollout's, for v1, v2 and v4: every form exists, with and
// without recording.  The staged table counts in the LDS sum and so in the halving fallback.
struct FovealSample {
    static constexpr const char* kKernel = "foveal_rollout_sample_kernel";
    static constexpr int kTableLds = kFovealSampleLds;
    static size_t table_bytes(const LmazeFovealParams& p) {
        const bool v1 = p.variant == LMAZE_VARIANT_V1;
        return (size_t)(v1 ? 1 : p.n_layouts) * p.grid * p.grid * (v1 ? 16 : 96);   // a multiple of 16
    }
    // the staged rows start on the next 16-byte boundary behind the layout characters
    static size_t staged_lds(size_t base, size_t table) { return ((base + 15) & ~(size_t)15) + table; }
    template <class RO>
    static auto& table(RO& ro) { return ro.smp; }
    template <int VARIANT, int EPB, int GT, bool AR, bool REC>
    static constexpr bool exists() { return VARIANT != LMAZE_VARIANT_V5; }
    template <int VARIANT, int EPB, int GT, bool AR, class RO>
    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const FovealArgs& a, const RO& ro) {
        hipLaunchKernelGGL((foveal_rollout_sample_kernel<VARIANT, EPB, GT, AR>), grid, block, lds, s, a, ro);
    }
};

hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsSmp& ro, bool rec, hipStream_t s) {
    return launch_foveal_rollout_sliced<FovealSample, FovealRollSmp>(a, ro, rec, s);
}

}  // namespace lmaze
