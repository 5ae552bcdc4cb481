// lmaze_foveal_policy.hip -- the closed-loop one-launch rollout of the foveal variants v1, v2 and v4
// (lmaze_foveal_rollout_policy, include/lmaze.h), gfx950.
//
// foveal_rollout_kernel's body (lmaze_foveal_body.h) included with LMAZE_FOVEAL_POLICY_SITE defined (its POL switch): phase 1 takes each env's action from a uint8 table
// keyed by (layout row, ball) -- staged in LDS behind the layout characters, or read from global memory when it is larger
// than kFovealPolicyLds -- mixed with the exploration draw of the grid envs' closed loop (policy_draw, lmaze_common.h), and
// stores the action and key rows beside the reward and done rows.  Everything else is the open-loop rollout's.  A
// translation unit of its own so that lmaze_foveal.hip's code objects and compile time stay what they were.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "lmaze_foveal_defs.h"

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

// ---- host side ----
// Instantiations as lmaze_foveal_rollout's: envs per workgroup 32 / 64 / 128 (launch_hint bits 4-7 = 2 / 3 / 4; any other
// code takes the default), GT 14 (v1) or 18 (v2, v4) or 0, AR plain / fused, with and without recording.  The policy bits
// never change results.
template <int VARIANT, int EPB, class RO>
static hipError_t launch_policy_one(const FovealArgs& a, const RO& ro0, hipStream_t s) {
    constexpr bool REC = std::is_same<RO, FovealRollObsPol>::value;
    const int L = VARIANT == LMAZE_VARIANT_V1 ? 1 : a.p.n_layouts;
    const size_t table = (size_t)L * a.p.grid * a.p.grid;
    RO ro = ro0;
    ro.pol.in_lds = table <= (size_t)kFovealPolicyLds ? 1 : 0;             // a rule, not a measurement
    const size_t lds0 = foveal_lds<VARIANT>(a.p, EPB) + (ro.pol.in_lds ? ((table + 15) & ~(size_t)15) : 0);
    size_t lds = lds0;
    if constexpr (EPB > 32) {
        if (lds > lds_limit()) return launch_policy_one<VARIANT, EPB / 2>(a, ro0, s);
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
        snprintf(name, sizeof(name), "foveal_rollout_policy_kernel<v%d, %d, %d, %s%s> table=%s", VARIANT, EPB, a.p.grid == GN ? GN : 0,
                 a.auto_reset ? "fused-reset" : "plain", REC ? ", obs_t" : "", ro.pol.in_lds ? "lds" : "global");
        describe_launch(a.info, name, EPB, lds > lds0 ? per_cu : 0, m, false, blocks, LMAZE_BLOCK, lds);
        return hipSuccess;
    }
    if (a.auto_reset) {
        if (a.p.grid == GN) hipLaunchKernelGGL((foveal_rollout_policy_kernel<VARIANT, EPB, GN, true>), grid, block, lds, s, b, ro);
        else hipLaunchKernelGGL((foveal_rollout_policy_kernel<VARIANT, EPB, 0, true>), grid, block, lds, s, b, ro);
    } else {
        if (a.p.grid == GN) hipLaunchKernelGGL((foveal_rollout_policy_kernel<VARIANT, EPB, GN, false>), grid, block, lds, s, b, ro);
        else hipLaunchKernelGGL((foveal_rollout_policy_kernel<VARIANT, EPB, 0, false>), grid, block, lds, s, b, ro);
    }
    return hipGetLastError();
}

// the open-loop rollout's choice of envs per workgroup (lmaze_foveal.hip launch_rollout_variant)
template <int VARIANT, class RO>
static hipError_t launch_policy_variant(const FovealArgs& a, const RO& ro, hipStream_t s) {
    switch ((a.p.launch_hint >> 4) & 15) {
        case 2: return launch_policy_one<VARIANT, 32>(a, ro, s);
        case 3: return launch_policy_one<VARIANT, 64>(a, ro, s);
        case 4: return launch_policy_one<VARIANT, 128>(a, ro, s);
        default: break;
    }
    if (a.n <= (int64_t)32 * 1024) return launch_policy_one<VARIANT, 32>(a, ro, s);
    const int C = VARIANT == LMAZE_VARIANT_V1 ? 4 : (VARIANT == LMAZE_VARIANT_V2 ? 5 : 7);
    if ((size_t)a.n * C * W25 * 4 > kFovealStreamBytes) return launch_policy_one<VARIANT, 128>(a, ro, s);
    return launch_policy_one<VARIANT, 64>(a, ro, s);
}

template <class RO>
static hipError_t launch_policy(const FovealArgs& a, const RO& ro, hipStream_t s) {
    switch (a.p.variant) {
        case LMAZE_VARIANT_V1: return launch_policy_variant<LMAZE_VARIANT_V1>(a, ro, s);
        case LMAZE_VARIANT_V2: return launch_policy_variant<LMAZE_VARIANT_V2>(a, ro, s);
        case LMAZE_VARIANT_V4: return launch_policy_variant<LMAZE_VARIANT_V4>(a, ro, s);
        default: return hipErrorInvalidValue;                   // v5/v6: refused by the entry point
    }
}

hipError_t launch_foveal_rollout_policy(const FovealArgs& a, const FovealRollObsPol& ro, bool rec, hipStream_t s) {
    if (rec) return launch_policy(a, ro, s);
    FovealRollPol plain;
    static_cast<FovealRoll&>(plain) = static_cast<const FovealRoll&>(ro);
    plain.pol = ro.pol;
    return launch_policy(a, plain, s);
}

}  // namespace lmaze
