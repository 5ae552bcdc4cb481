// lmaze_foveal_sample.hip -- the sampling closed-loop one-launch rollout of the foveal variants v1, v2 and v4
// (lmaze_foveal_rollout_sample, include/lmaze.h), gfx950.
//
// foveal_rollout_kernel's body (lmaze_foveal_body.h) included with LMAZE_FOVEAL_SAMPLE_SITE defined (POL = 2): phase 1 draws
// each env's action from the categorical distribution of its key -- a row of cumulative uint32 thresholds (3 for v1, 24 for
// v2/v4) staged in LDS behind the layout characters, or read from global memory when the table is larger than
// kFovealSampleLds, compared against one word of the closed loop's draw (policy_draw, lmaze_common.h) -- and stores the action
// and key rows beside the reward and done rows.  Everything else is the open-loop rollout's.  A translation unit of its own:
// lmaze_foveal.hip's and lmaze_foveal_policy.hip's code objects stay what they were.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "lmaze_foveal_defs.h"

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

// ---- host side ----
// Instantiations, launch_hint bits and defaults as lmaze_foveal_rollout_policy's: envs per workgroup 32 / 64 / 128, GT 14
// (v1) or 18 (v2, v4) or 0, AR plain / fused, with and without recording.  The staged table counts in the LDS sum and so in
// the halving fallback.  The policy bits never change results.
template <int VARIANT, int EPB, class RO>
static hipError_t launch_sample_one(const FovealArgs& a, const RO& ro0, hipStream_t s) {
    constexpr bool REC = std::is_same<RO, FovealRollObsSmp>::value;
    const int L = VARIANT == LMAZE_VARIANT_V1 ? 1 : a.p.n_layouts;
    const size_t table = (size_t)L * a.p.grid * a.p.grid * (VARIANT == LMAZE_VARIANT_V1 ? 16 : 96);   // bytes, a multiple of 16
    RO ro = ro0;
    ro.smp.in_lds = table <= (size_t)kFovealSampleLds ? 1 : 0;             // a rule, not a measurement
    // the staged rows start on the next 16-byte boundary behind the layout characters
    const size_t lds0 = ro.smp.in_lds ? ((foveal_lds<VARIANT>(a.p, EPB) + 15) & ~(size_t)15) + table : foveal_lds<VARIANT>(a.p, EPB);
    size_t lds = lds0;
    if constexpr (EPB > 32) {
        if (lds > lds_limit()) return launch_sample_one<VARIANT, EPB / 2>(a, ro0, s);
    }
    const int64_t nchunks = (a.n + EPB - 1) / EPB;
    const int m = ((a.p.launch_hint >> 8) & 3) + 1;            // bits 8-9: chunks per workgroup - 1
    const int64_t blocks = (nchunks + m - 1) / m;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    const int per_cu = a.p.launch_hint & 15;
    lds = lds_for_cap(lds, per_cu);
    FovealArgs b = a;
    b.nt = 0;                 // plain stores, as the open-loop rollout
    constexpr int GN = VARIANT == LMAZE_VARIANT_V1 ? 14 : 18;
    const dim3 grid((unsigned)blocks), block(LMAZE_BLOCK);
    if (a.info) {
        char name[96];
        snprintf(name, sizeof(name), "foveal_rollout_sample_kernel<v%d, %d, %d, %s%s> table=%s", VARIANT, EPB, a.p.grid == GN ? GN : 0,
                 a.auto_reset ? "fused-reset" : "plain", REC ? ", obs_t" : "", ro.smp.in_lds ? "lds" : "global");
        describe_launch(a.info, name, EPB, lds > lds0 ? per_cu : 0, m, false, blocks, LMAZE_BLOCK, lds);
        return hipSuccess;
    }
    if (a.auto_reset) {
        if (a.p.grid == GN) hipLaunchKernelGGL((foveal_rollout_sample_kernel<VARIANT, EPB, GN, true>), grid, block, lds, s, b, ro);
        else hipLaunchKernelGGL((foveal_rollout_sample_kernel<VARIANT, EPB, 0, true>), grid, block, lds, s, b, ro);
    } else {
        if (a.p.grid == GN) hipLaunchKernelGGL((foveal_rollout_sample_kernel<VARIANT, EPB, GN, false>), grid, block, lds, s, b, ro);
        else hipLaunchKernelGGL((foveal_rollout_sample_kernel<VARIANT, EPB, 0, false>), grid, block, lds, s, b, ro);
    }
    return hipGetLastError();
}

// the open-loop rollout's choice of envs per workgroup (lmaze_foveal.hip launch_rollout_variant)
template <int VARIANT, class RO>
static hipError_t launch_sample_variant(const FovealArgs& a, const RO& ro, hipStream_t s) {
    switch ((a.p.launch_hint >> 4) & 15) {
        case 2: return launch_sample_one<VARIANT, 32>(a, ro, s);
        case 3: return launch_sample_one<VARIANT, 64>(a, ro, s);
        case 4: return launch_sample_one<VARIANT, 128>(a, ro, s);
        default: break;
    }
    if (a.n <= (int64_t)32 * 1024) return launch_sample_one<VARIANT, 32>(a, ro, s);
    const int C = VARIANT == LMAZE_VARIANT_V1 ? 4 : (VARIANT == LMAZE_VARIANT_V2 ? 5 : 7);
    if ((size_t)a.n * C * W25 * 4 > kFovealStreamBytes) return launch_sample_one<VARIANT, 128>(a, ro, s);
    return launch_sample_one<VARIANT, 64>(a, ro, s);
}

template <class RO>
static hipError_t launch_sample(const FovealArgs& a, const RO& ro, hipStream_t s) {
    switch (a.p.variant) {
        case LMAZE_VARIANT_V1: return launch_sample_variant<LMAZE_VARIANT_V1>(a, ro, s);
        case LMAZE_VARIANT_V2: return launch_sample_variant<LMAZE_VARIANT_V2>(a, ro, s);
        case LMAZE_VARIANT_V4: return launch_sample_variant<LMAZE_VARIANT_V4>(a, ro, s);
        default: return hipErrorInvalidValue;                   // v5/v6: refused by the entry point
    }
}

hipError_t launch_foveal_rollout_sample(const FovealArgs& a, const FovealRollObsSmp& ro, bool rec, hipStream_t s) {
    if (rec) return launch_sample(a, ro, s);
    FovealRollSmp plain;
    static_cast<FovealRoll&>(plain) = static_cast<const FovealRoll&>(ro);
    plain.smp = ro.smp;
    return launch_sample(a, plain, s);
}

}  // namespace lmaze
