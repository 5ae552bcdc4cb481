// lmaze_foveal.hip -- the foveal variants of the step path (5x5 window observations), gfx950.
//
//   v1 = gym_lmaze/envs/lmaze_env_v1.py:114-200   4-neighbour move, two reward streams, foveal goal
//   v2 = gym_lmaze/envs/lmaze_env_v2.py:127-225   25-way teleport inside the fovea, 5 layouts
//   v4 = gym_lmaze/envs/lmaze_env_v4.py:167-272   v2 + float visit-map plane (whole-plane halving)
//
//   v5/v6 = lmaze_env_v5.py:158-292 (plannerStep + step), lmaze_env_v6.py:505-523 (safeFovealGoal)
//
// Same two-phase shape as lmaze_step.hip: one lane per env runs the transition against the
// layout table held in LDS and leaves the env's observation in LDS as 25-bit plane masks; then the
// workgroup's lanes stripe its contiguous observation range float[envs*C*25] with 16-byte stores.
// v4-v6 add a middle phase on the visit map, kept CLOCK-RELATIVE and TILED (include/lmaze.h "The visit map"): the
// reference halves the whole G x G plane on every update (v4:211-214, v5:313-318); here that is `clock += 1` and a
// step only gathers the 2 x 2 tiles (4 x 4 cells, 64 B each) under the window it shows, adds, and writes them back.
// HBM bytes per env-step: v1 454, v2 545, v4 about 1 000 instead of round 2's 3 337.
// The step and reset launchers are here; the one-launch rollout is launched by lmaze_foveal_launch.h (FovealOpen below).
#include <cstdio>
#include <cstring>

#include "lmaze_foveal_launch.h"

namespace lmaze {

#ifdef LMAZE_FOVEAL_WAVES   // experiment builds only (tools/_exp): force a register budget
#define LMAZE_FOVEAL_ATTR __attribute__((amdgpu_waves_per_eu(LMAZE_FOVEAL_WAVES)))
#else
#define LMAZE_FOVEAL_ATTR
#endif
// The step kernels and the rollout kernel share one body, lmaze_foveal_body.h, included into each (a kernel of its own
// rather than a __device__ function: through a function the existing step kernels compiled to other code -- their kernel
// argument loads lost their no-clobber marks, and v5's two-level step went from 127 to 129 VGPRs, one wave per SIMD less).
// ROLL = false: one step over one chunk per workgroup round, as ever; everything the rollout adds is dead code.
template <int VARIANT, int MODE, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) LMAZE_FOVEAL_ATTR void foveal_kernel(const FovealArgs a) {
    constexpr bool ROLL = false, REC = false;
    const FovealRoll ro{};
#define LMAZE_FOVEAL_BODY_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_BODY_SITE
}

// T steps of the plain (AR false) or fused step (AR: v1/v2/v4 fused reset, v5/v6 two-level step) in one launch: every
// chunk runs ro.T steps before the workgroup moves on (FovealRoll).  At least 4 waves per SIMD, the floor of the v4-v6
// steps: left to itself v5's rollout takes 121-152 VGPRs (3 waves at 64 envs per workgroup); v1/v2/v4 stay below the budget
template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void foveal_rollout_kernel(const FovealArgs a, const FovealRoll ro) {
    constexpr bool ROLL = true, REC = false;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_BODY_SITE
}

// the recording form (lmaze_foveal_rollout_obs): the same kernel, with FovealRollObs.  v1 / v2 held to 6 waves per SIMD,
// the floor of their plain rollouts (left to itself the slot stores take them to 84-89 VGPRs, 5 waves)
template <int VARIANT, int EPB, int GT, bool AR>
__global__ __launch_bounds__(LMAZE_BLOCK)
__attribute__((amdgpu_waves_per_eu(VARIANT == LMAZE_VARIANT_V1 || VARIANT == LMAZE_VARIANT_V2 ? 6 : 4)))
void foveal_rollout_kernel(const FovealArgs a, const FovealRollObs ro) {
    constexpr bool ROLL = true, REC = true;
    constexpr int MODE = FM_STEP;
#define LMAZE_FOVEAL_BODY_SITE
#include "lmaze_foveal_body.h"
#undef LMAZE_FOVEAL_BODY_SITE
}

// v6 safeFovealGoal (v6:505-523): one lane per env
__global__ __launch_bounds__(LMAZE_BLOCK) void safe_goal_kernel(const FovealArgs a, int32_t* out_goal) {
    const int64_t e = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    if (e >= a.n) return;
    const int G = a.p.grid;
    const uint8_t* lay = a.layouts + (size_t)clampi(a.b.layout_id[e], 0, a.p.n_layouts - 1) * G * G;
    const int bx = a.b.ball_xy[2 * e], by = a.b.ball_xy[2 * e + 1];
    const uint4 d = env_draw(a.seed, a.epoch, a.env_base + e);
    unsigned ok = 0;
    for (int c = 0; c < W25; ++c) {
        const int x = bx - 2 + c / FOV, y = by - 2 + c % FOV;
        const bool in = x >= 0 && y >= 0 && x < G && y < G;
        if (in && lay[x * G + y] != 'W') ok |= 1u << c;
    }
    int pick = 12;
    const int cnt = __popc(ok);
    if (cnt > 0) {
        int k = (int)__umulhi(d.x, (uint32_t)cnt);
        for (int c = 0; c < W25; ++c)
            if (ok & (1u << c)) {
                if (k == 0) { pick = c; break; }
                --k;
            }
    }
    out_goal[e] = pick;
}

// ------------------------------------------------------------------------------------
// xE nearest-neighbour on float planes (v1:258-277, v2:197-203): one workgroup per env
// ------------------------------------------------------------------------------------
struct ExpandPlanesArgs {
    const float* planes;
    float* out;
    int64_t n;
    int32_t channels, g, expansion;
};

__global__ __launch_bounds__(LMAZE_BLOCK) void expand_planes_kernel(const ExpandPlanesArgs a) {
    extern __shared__ int4 lds4[];
    const int g = a.g, E = a.expansion, C = a.channels;
    const int PC = g * g, S = g * E, PLANE = S * S, L = C * PLANE;
    float* src = reinterpret_cast<float*>(lds4);                    // [C*g*g]
    uint16_t* rowmap = reinterpret_cast<uint16_t*>(src + C * PC);   // [S] row -> (row / E) * g
    uint16_t* colmap = rowmap + S;                                  // [S] col -> col / E
    const int tid = threadIdx.x;
    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        __syncthreads();
        for (int k = tid; k < C * PC; k += LMAZE_BLOCK) src[k] = a.planes[(size_t)i * C * PC + k];
        for (int k = tid; k < S; k += LMAZE_BLOCK) {
            rowmap[k] = (uint16_t)((k / E) * g);
            colmap[k] = (uint16_t)(k / E);
        }
        __syncthreads();
        const size_t B = (size_t)i * L;
        const size_t a0 = (B + 3) & ~(size_t)3, a1 = (B + L) & ~(size_t)3;
        auto value = [&](int local) -> float {
            const int c = local / PLANE;
            const int rem = local - c * PLANE;
            const int row = rem / S, col = rem - row * S;
            return src[c * PC + rowmap[row] + colmap[col]];
        };
        if (tid < (int)(a0 - B)) a.out[B + tid] = value(tid);
        if (tid < (int)(B + L - a1)) a.out[a1 + tid] = value((int)(a1 - B) + tid);
        const int nq = (int)((a1 - a0) >> 2);
        float4* out4 = reinterpret_cast<float4*>(a.out + a0);
        const int head = (int)(a0 - B);
        for (int q = tid; q < nq; q += LMAZE_BLOCK) {
            const int local = head + (q << 2);
            int c = local / PLANE;
            int rem = local - c * PLANE;
            int row = rem / S, col = rem - row * S;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = src[c * PC + rowmap[row] + colmap[col]];
                if (++col == S) {
                    col = 0;
                    if (++row == S) { row = 0; ++c; }
                }
            }
            out4[q] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// The foveal shape itself (5x5 window, x7; every foveal variant): g and E at compile time, so the flat index
// decodes by multiplication, and the output treated as what it is -- ONE contiguous stream of N*C planes of
// 35x35 floats.  Workgroup w writes the aligned stretch [w*CH, (w+1)*CH) floats of it (an env is 19.6-34 KB
// and starts on a 16-byte boundary only: per-env workgroups straddle cache lines with every wave store).
template <int GT, int ET, bool NT>
__global__ __launch_bounds__(LMAZE_BLOCK) void expand_planes_stream_kernel(const ExpandPlanesArgs a, int chunk_floats) {
    constexpr int PC = GT * GT, S = GT * ET, PLANE = S * S;
    extern __shared__ int4 lds4[];
    float* src = reinterpret_cast<float*>(lds4);                    // [planes touched][PC]
    const int tid = threadIdx.x;
    const int64_t total = a.n * (int64_t)a.channels * PLANE;
    const int64_t f0 = (int64_t)blockIdx.x * chunk_floats;
    const int len = (int)min((int64_t)chunk_floats, total - f0);
    const int64_t p0 = f0 / PLANE;                                  // first plane of the stretch (plane = env*C + c)
    const int off0 = (int)(f0 - p0 * PLANE);
    const int np = (off0 + len + PLANE - 1) / PLANE;
    for (int k = tid; k < np * PC; k += LMAZE_BLOCK) src[k] = a.planes[(size_t)p0 * PC + k];
    __syncthreads();
    float* dst = a.out + f0;
    static_assert(ET >= 4, "four consecutive output columns span at most two cells");
    for (int q = tid; (q << 2) < len; q += LMAZE_BLOCK) {
        const int local = off0 + (q << 2);
        const int p = local / PLANE;
        const int rem = local - p * PLANE;
        const int row = rem / S, col = rem - row * S;
        // one path for every lane (S = 35: every wave holds float4s that straddle an output row): the value
        // under the first column, the next one of the same window row, and the first of the following row
        const float* r0 = src + p * PC + (row / ET) * GT;
        const int k0 = col / ET;
        const float v0 = r0[k0], v1 = r0[k0 + 1];                      // r0[GT] is read but never selected
        int row1 = row + 1, p1 = p;
        if (row1 == S) { row1 = 0; ++p1; }
        const float vw = src[p1 * PC + (row1 / ET) * GT];
        const int edge = (k0 + 1) * ET;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cj = col + j;
            v[j] = cj >= S ? vw : (cj >= edge ? v1 : v0);
        }
        const int count = len - (q << 2);
        if (count >= 4) {
            if (NT) {
                typedef float f4 __attribute__((ext_vector_type(4)));
                f4 t = {v[0], v[1], v[2], v[3]};
                stream_store16(reinterpret_cast<f4*>(dst) + q, t);
            } else {
                reinterpret_cast<float4*>(dst)[q] = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
            for (int j = 0; j < count; ++j) dst[(q << 2) + j] = v[j];
        }
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------

// The instantiations of foveal_kernel, X(variant, mode, envs per workgroup): the step at the four sizes launch_hint bits 4-7
// name, the other modes at their one size and its LDS fallback; each at GT 18 / 14 / 0 and, the step, plain and with the
// fused reset (v5: the two-level step).  v6 runs v5's.  No plan names the planner mode of v1 / v2 / v4, the 32-env fallback
// of the other modes on a device with 160 KiB of LDS, or the last line's sizes of v2; the code object has always held them.
#define LMAZE_FOVEAL_VARIANTS(X, MODE, EPB) \
    X(LMAZE_VARIANT_V1, MODE, EPB) X(LMAZE_VARIANT_V2, MODE, EPB) X(LMAZE_VARIANT_V4, MODE, EPB) X(LMAZE_VARIANT_V5, MODE, EPB)
#define LMAZE_FOVEAL_KERNELS(X)                                                             \
    LMAZE_FOVEAL_VARIANTS(X, FM_STEP, 32) LMAZE_FOVEAL_VARIANTS(X, FM_STEP, 64)             \
    LMAZE_FOVEAL_VARIANTS(X, FM_STEP, 128) LMAZE_FOVEAL_VARIANTS(X, FM_STEP, 256)           \
    LMAZE_FOVEAL_VARIANTS(X, FM_RESET, 32) LMAZE_FOVEAL_VARIANTS(X, FM_RESET, 64)           \
    X(LMAZE_VARIANT_V1, FM_SETGOAL, 32) X(LMAZE_VARIANT_V1, FM_SETGOAL, 64)                 \
    LMAZE_FOVEAL_VARIANTS(X, FM_PLANNER, 32) LMAZE_FOVEAL_VARIANTS(X, FM_PLANNER, 64)       \
    X(LMAZE_VARIANT_V2, FM_RESET, 128) X(LMAZE_VARIANT_V2, FM_RESET, 256)                   \
    X(LMAZE_VARIANT_V2, FM_PLANNER, 128) X(LMAZE_VARIANT_V2, FM_PLANNER, 256)

// The kernel of a planned launch: every instantiation of foveal_kernel is named here and nowhere else
using FovealKernel = void (*)(const FovealArgs);
template <int VARIANT, int MODE, int EPB>
static FovealKernel foveal_kernel_of(int gt, bool ar) {
    if constexpr (MODE == FM_STEP) {
        if (ar) return gt == 18 ? foveal_kernel<VARIANT, MODE, EPB, 18, true> : gt == 14 ? foveal_kernel<VARIANT, MODE, EPB, 14, true>
                                                                                         : foveal_kernel<VARIANT, MODE, EPB, 0, true>;
    }
    return gt == 18 ? foveal_kernel<VARIANT, MODE, EPB, 18, false> : gt == 14 ? foveal_kernel<VARIANT, MODE, EPB, 14, false>
                                                                              : foveal_kernel<VARIANT, MODE, EPB, 0, false>;
}

static const void* foveal_kernel_of(const FovealPlan& p) {
#define X(VARIANT, MODE, EPB) \
    if (p.variant == VARIANT && p.mode == MODE && p.epb == EPB) return (const void*)foveal_kernel_of<VARIANT, MODE, EPB>(p.gt, p.ar);
    LMAZE_FOVEAL_KERNELS(X)
#undef X
    return nullptr;
}

// One launch of foveal_kernel in `mode` over a.n envs as foveal_plan decides (lmaze_foveal_launch.h).  a.info != null: the
// plan is described instead of queued.
static hipError_t launch_foveal(const FovealArgs& a, int mode, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    FovealPlan p;
    if (!foveal_plan(a, FovealForm{mode, false, false, 0}, p)) return hipErrorInvalidConfiguration;
    if (a.info) {
        static const char* const modes[] = {"step", "reset", "setgoal", "planner"};
        char name[96];
        snprintf(name, sizeof(name), "foveal_kernel<v%d, %s, %d, %d, %s>", p.variant, modes[mode], p.epb, p.gt, p.ar ? "fused-reset" : "plain");
        describe_launch(a.info, name, p.epb, p.per_cu, p.chunks, p.nt != 0, p.blocks, p.block, p.lds);
        return hipSuccess;
    }
    const void* kernel = foveal_kernel_of(p);
    if (!kernel) return hipErrorInvalidConfiguration;
    FovealArgs b = a;
    b.nt = p.nt;
    b.p.launch_hint = p.launch_hint;
    void* args[] = {&b};
    (void)hipLaunchKernel(kernel, dim3((unsigned)p.blocks), dim3(p.block), args, p.lds, s);   // read back as after hipLaunchKernelGGL
    return hipGetLastError();
}

// ---- the one-launch rollout (lmaze_foveal_rollout): the open-loop family of lmaze_foveal_launch.h ----
struct FovealOpen {
    static constexpr const char* kKernel = "foveal_rollout_kernel";
    static constexpr int kTableLds = 0;
    template <int VARIANT, int EPB, int GT, bool AR, bool REC>
    static constexpr bool exists() {
        // v5/v6: the two-level step only (the plain v5/v6 step spills at 4 waves per SIMD: lmaze_foveal_rollout refuses it), and
        // for grids other than 18 only at 32 envs per workgroup (64: 8 bytes of scratch) and not recording (at G = 0 that
        // needs 12 bytes of scratch at 4 waves per SIMD, so lmaze_foveal_rollout_obs refuses other grids for v5/v6: LMAZE_E_GRID)
        if (VARIANT == LMAZE_VARIANT_V5) return AR && (GT == 18 || (EPB == 32 && !REC));
        // v1's recording form only at G = 14: at G = 0 it spills (12 bytes) at the 6 waves per SIMD of v1's rollouts, so
        // lmaze_foveal_rollout_obs refuses other grids for v1 (LMAZE_E_GRID)
        if (VARIANT == LMAZE_VARIANT_V1 && REC) return GT == 14;
        return true;
    }
    template <int VARIANT, int EPB, int GT, bool AR, class RO>
    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const FovealArgs& a, const RO& ro) {
        hipLaunchKernelGGL((foveal_rollout_kernel<VARIANT, EPB, GT, AR>), grid, block, lds, s, a, ro);
    }
};

// The reference's float[N,G,G] out of / into the clock-relative tiles (include/lmaze.h): one thread per cell.
__global__ __launch_bounds__(LMAZE_BLOCK) void visit_materialise_kernel(const uint32_t* tiles, const int32_t* clock, float* out,
                                                                        int64_t n, int G) {
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    const int CELLS = G * G;
    if (i >= n * CELLS) return;
    const int64_t e = i / CELLS;
    const int c = (int)(i - e * CELLS), x = c / G, y = c - x * G;
    const int TB = visit_tiles(G);
    const uint32_t b = tiles[((size_t)e * TB * TB + (x / VT) * TB + (y / VT)) * (VT * VT) + (x % VT) * VT + (y % VT)];
    out[i] = __uint_as_float(visit_true(b, clock[e] & 0xff));
}

__global__ __launch_bounds__(LMAZE_BLOCK) void visit_load_kernel(uint32_t* tiles, int32_t* clock, const float* in, int64_t n, int G) {
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    const int TB = visit_tiles(G), PER = TB * TB * VT * VT;
    if (i >= n * PER) return;
    const int64_t e = i / PER;
    const int r = (int)(i - e * PER), tile = r / (VT * VT), c = r - tile * (VT * VT);
    const int x = (tile / TB) * VT + c / VT, y = (tile % TB) * VT + c % VT;
    tiles[i] = (x < G && y < G) ? __float_as_uint(in[(size_t)e * G * G + x * G + y]) : 0u;
    if (r == 0) clock[e] = VISIT_BIAS;        // stored == true value in this frame; record tag cleared: the next step reads the tiles
}


}  // namespace lmaze

using namespace lmaze;

// The variants a foveal entry takes
enum { TAKES_V1 = 1, TAKES_V2_V4 = 2, TAKES_V5_V6 = 4, TAKES_ALL = 7 };
static bool takes_variant(int takes, int variant) {
    const bool v56 = variant == LMAZE_VARIANT_V5 || variant == LMAZE_VARIANT_V6;
    return (takes & (variant == LMAZE_VARIANT_V1 ? TAKES_V1 : (v56 ? TAKES_V5_V6 : TAKES_V2_V4))) != 0;
}

// Every entry that queues foveal_kernel -- the plain, the fused and the two-level step, reset, setFovealGoal, plannerStep --
// and, info != null, the step's describe (which has judged the params itself: nothing is refused here then, and bufs is
// null).  mode: the FovealMode; takes: the variants the entry accepts; action: the mode's int32 input (action ids, ij,
// goals); own: false if one of the entry's own pointers is missing; fr: its draws, fused reset and epoch words.  The
// refusals stand in this order: check_foveal's, the entry's variant, its own pointers (LMAZE_E_NULL), the epoch words
// (LMAZE_E_ALIGN); n == 0 returns 0 after all of them.
static int foveal_entry(const LmazeFovealParams* params, int mode, int takes, const uint8_t* layouts, const int32_t* action,
                        const int32_t* goal2, bool own, const uint8_t* mask, int32_t place, const FovealReset& fr,
                        const LmazeFovealBuffers* bufs, int64_t n, LaunchInfo* info, void* stream) {
    if (!info) {
        const int rc = check_foveal(params, layouts, bufs, n);
        if (rc) return rc;
        if (!takes_variant(takes, params->variant)) return LMAZE_E_VARIANT;
        if (!own) return LMAZE_E_NULL;
        if (bad_epoch_words(fr.epoch_in, fr.epoch_out)) return LMAZE_E_ALIGN;
    }
    FovealArgs a = make_foveal_args(params, layouts, bufs, n, fr);
    a.action = action;
    a.goal2 = goal2;
    a.mask = mask;
    a.place = place;
    a.info = info;
    return (int)launch_foveal(a, mode, (hipStream_t)stream);
}

extern "C" {

int lmaze_foveal_step(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* action,
                      const LmazeFovealBuffers* bufs, int64_t n, void* stream) {
    return foveal_entry(params, FM_STEP, TAKES_ALL, layouts, action, nullptr, action != nullptr, nullptr, 0,
                        kNoFovealReset, bufs, n, nullptr, stream);
}

int lmaze_foveal_step_autoreset(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* action,
                                const LmazeFovealBuffers* bufs, int64_t n, uint64_t seed, uint64_t epoch,
                                int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev, void* stream) {
    return foveal_entry(params, FM_STEP, TAKES_V1 | TAKES_V2_V4, layouts, action, nullptr, action != nullptr, nullptr, 0,
                        FovealReset{1, seed, epoch, env_base, epoch_in_dev, epoch_out_dev}, bufs, n, nullptr, stream);
}

int lmaze_v5_hier_step(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* action,
                       const int32_t* planner_goal, const LmazeFovealBuffers* bufs, int64_t n, uint64_t seed,
                       uint64_t epoch, int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev,
                       void* stream) {
    return foveal_entry(params, FM_STEP, TAKES_V5_V6, layouts, action, planner_goal, action && planner_goal, nullptr, 0,
                        FovealReset{1, seed, epoch, env_base, epoch_in_dev, epoch_out_dev}, bufs, n, nullptr, stream);
}

// the argument checks of lmaze_foveal_rollout that need no buffers (answered before anything else is looked at)
static int check_rollout_call(const LmazeFovealParams* params, const int32_t* planner_goals, int32_t T, int64_t n,
                              int32_t auto_reset) {
    if (T < 0 || n < 0 || n > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    if (!params) return LMAZE_E_NULL;
    const bool v56 = params->variant == LMAZE_VARIANT_V5 || params->variant == LMAZE_VARIANT_V6;
    if (!v56 && planner_goals) return LMAZE_E_VARIANT;                 // the two-level step is v5/v6's
    if (v56 && auto_reset && !planner_goals) return LMAZE_E_NULL;      // their episodes restart through plannerStep
    if (v56 && !planner_goals) return LMAZE_E_VARIANT;                 // their plain step has no one-launch form (see below)
    return 0;
}

// lmaze_foveal_rollout and, rec != null, lmaze_foveal_rollout_obs (rec: the caller's obs_t, obs_local_t and every)
static int foveal_rollout(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* actions,
                          const int32_t* planner_goals, int32_t T, const LmazeFovealBuffers* bufs, int64_t n, int32_t auto_reset,
                          uint64_t seed, uint64_t epoch, int64_t env_base, float* reward_t, uint8_t* done_t,
                          float* foveal_reward_t, uint8_t* foveal_done_t, const FovealRollObs* rec, void* stream) {
    int32_t slots = 0;
    if (rec) {                                                         // the recording request first: its refusals need nothing else
        if (rec->every < 1) return LMAZE_E_COUNT;
        slots = T > 0 ? T / rec->every : 0;
        if (slots > 0 && !rec->obs_t) return LMAZE_E_NULL;
        if (((uintptr_t)rec->obs_t & 15) || ((uintptr_t)rec->obs_local_t & 15)) return LMAZE_E_ALIGN;
    }
    if (T == 0 || n == 0) return (T < 0 || n < 0 || n > LMAZE_MAX_ENVS) ? LMAZE_E_COUNT : 0;   // nothing to do, nothing read
    int rc = check_rollout_call(params, planner_goals, T, n, auto_reset);
    if (rc) return rc;
    rc = check_foveal(params, layouts, bufs, n);
    if (rc) return rc;
    if (!actions) return LMAZE_E_NULL;
    const bool v56 = params->variant == LMAZE_VARIANT_V5 || params->variant == LMAZE_VARIANT_V6;
    if (rec) {
        if (rec->obs_local_t && !v56) return LMAZE_E_VARIANT;          // only v5/v6 have a local observation
        if (v56 && params->grid != 18) return LMAZE_E_GRID;            // their recording form exists at G = 18 only
        if (params->variant == LMAZE_VARIANT_V1 && params->grid != 14) return LMAZE_E_GRID;   // v1's at G = 14 only
    }
    FovealArgs a = make_foveal_args(params, layouts, bufs, n,
                                    FovealReset{planner_goals || (!v56 && auto_reset), seed, epoch, env_base, nullptr, nullptr});
    a.action = actions;
    a.goal2 = planner_goals;
    const FovealRoll ro{T, reward_t, done_t, foveal_reward_t, foveal_done_t};
    if (!rec) return (int)launch_foveal_rollout<FovealOpen>(a, ro, (hipStream_t)stream);
    const FovealRollObs rr{ro, slots > 0 ? rec->obs_t : nullptr, slots > 0 ? rec->obs_local_t : nullptr, rec->every};
    return (int)launch_foveal_rollout<FovealOpen>(a, rr, (hipStream_t)stream);
}

int lmaze_foveal_rollout(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* actions,
                         const int32_t* planner_goals, int32_t T, const LmazeFovealBuffers* bufs, int64_t n,
                         int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, float* reward_t,
                         uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t, void* stream) {
    return foveal_rollout(params, layouts, actions, planner_goals, T, bufs, n, auto_reset, seed, epoch, env_base, reward_t, done_t,
                          foveal_reward_t, foveal_done_t, nullptr, stream);
}

int lmaze_foveal_rollout_obs(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* actions,
                             const int32_t* planner_goals, int32_t T, const LmazeFovealBuffers* bufs, int64_t n,
                             int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, float* reward_t,
                             uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t, float* obs_t,
                             float* obs_local_t, int32_t obs_every, void* stream) {
    const FovealRollObs rec{{}, obs_t, obs_local_t, obs_every};
    return foveal_rollout(params, layouts, actions, planner_goals, T, bufs, n, auto_reset, seed, epoch, env_base, reward_t, done_t,
                          foveal_reward_t, foveal_done_t, &rec, stream);
}

// lmaze_describe_foveal_rollout and, obs_every != null, lmaze_describe_foveal_rollout_obs
static int describe_foveal_rollout(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t two_level,
                                   const int32_t* obs_every, char* text_host, int32_t len) {
    if (!params || !text_host || len < 1) return LMAZE_E_NULL;
    if (obs_every && *obs_every < 1) return LMAZE_E_COUNT;                 // the recording request first, as the entry point
    const bool v56 = params->variant == LMAZE_VARIANT_V5 || params->variant == LMAZE_VARIANT_V6;
    // v5/v6: the two-level step only.  The same code as an unknown variant's, which is judged next: their order does not show
    if ((two_level != 0) != v56) return LMAZE_E_VARIANT;
    int rc = check_foveal_params(params);
    if (!rc) rc = T < 0 ? LMAZE_E_COUNT : check_foveal_count(n);
    if (rc) return rc;
    text_host[0] = 0;
    if (n == 0 || T == 0) return 0;
    if (obs_every) {
        if (v56 && params->grid != 18) return LMAZE_E_GRID;                // their recording form exists at G = 18 only
        if (params->variant == LMAZE_VARIANT_V1 && params->grid != 14) return LMAZE_E_GRID;   // v1's at G = 14 only
    }
    LaunchInfo info{};
    // nothing is dereferenced: the launcher fills `info`
    FovealArgs a = make_foveal_args(params, nullptr, nullptr, n, FovealReset{two_level || (!v56 && auto_reset), 0, 0, 0, nullptr, nullptr});
    a.info = &info;
    const FovealRollObs rr{{T, nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr, obs_every ? *obs_every : 1};
    rc = obs_every ? (int)launch_foveal_rollout<FovealOpen>(a, rr, nullptr)
                   : (int)launch_foveal_rollout<FovealOpen>(a, static_cast<const FovealRoll&>(rr), nullptr);
    return rc ? rc : format_launch(info, text_host, len, T);
}

int lmaze_describe_foveal_rollout(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                  int32_t two_level, char* text_host, int32_t len) {
    return describe_foveal_rollout(params, n, T, auto_reset, two_level, nullptr, text_host, len);
}

int lmaze_describe_foveal_rollout_obs(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                      int32_t two_level, int32_t obs_every, char* text_host, int32_t len) {
    return describe_foveal_rollout(params, n, T, auto_reset, two_level, &obs_every, text_host, len);
}

int lmaze_foveal_reset(const LmazeFovealParams* params, const uint8_t* layouts, const uint8_t* mask, int32_t place,
                       uint64_t seed, uint64_t epoch, int64_t env_base, const LmazeFovealBuffers* bufs, int64_t n,
                       void* stream) {
    return foveal_entry(params, FM_RESET, TAKES_ALL, layouts, nullptr, nullptr, true, mask, place,
                        FovealReset{0, seed, epoch, env_base, nullptr, nullptr}, bufs, n, nullptr, stream);
}

int lmaze_v1_set_foveal_goal(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* ij,
                             const uint8_t* mask, const LmazeFovealBuffers* bufs, int64_t n, void* stream) {
    return foveal_entry(params, FM_SETGOAL, TAKES_V1, layouts, ij, nullptr, ij != nullptr, mask, 0,
                        kNoFovealReset, bufs, n, nullptr, stream);
}

int lmaze_v5_planner_step(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* goal,
                          const uint8_t* mask, const LmazeFovealBuffers* bufs, int64_t n, void* stream) {
    return foveal_entry(params, FM_PLANNER, TAKES_V5_V6, layouts, goal, nullptr, goal != nullptr, mask, 0,
                        kNoFovealReset, bufs, n, nullptr, stream);
}

int lmaze_v6_safe_foveal_goal(const LmazeFovealParams* params, const uint8_t* layouts, uint64_t seed, uint64_t epoch,
                              int64_t env_base, const LmazeFovealBuffers* bufs, int32_t* out_goal, int64_t n,
                              void* stream) {
    int rc = check_foveal(params, layouts, bufs, n);
    if (rc) return rc;
    if (!takes_variant(TAKES_V5_V6, params->variant)) return LMAZE_E_VARIANT;
    if (!out_goal) return LMAZE_E_NULL;
    if (n == 0) return 0;
    const FovealArgs a = make_foveal_args(params, layouts, bufs, n, FovealReset{0, seed, epoch, env_base, nullptr, nullptr});
    if (!grid_ok((n + LMAZE_BLOCK - 1) / LMAZE_BLOCK)) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(safe_goal_kernel, dim3((unsigned)((n + LMAZE_BLOCK - 1) / LMAZE_BLOCK)), dim3(LMAZE_BLOCK), 0,
                       (hipStream_t)stream, a, out_goal);
    return (int)hipGetLastError();
}

int lmaze_describe_foveal_step(const LmazeFovealParams* params, int64_t n, int32_t auto_reset, char* text_host, int32_t len) {
    if (!params || !text_host || len < 1) return LMAZE_E_NULL;
    int rc = check_foveal_params(params);
    if (!rc) rc = check_foveal_count(n);
    if (rc) return rc;
    text_host[0] = 0;
    if (n == 0) return 0;
    LaunchInfo info{};
    // nothing is dereferenced: the launcher fills `info`
    rc = foveal_entry(params, FM_STEP, TAKES_ALL, nullptr, nullptr, nullptr, true, nullptr, 0, FovealReset{auto_reset, 0, 0, 0, nullptr, nullptr},
                      nullptr, n, &info, nullptr);
    return rc ? rc : format_launch(info, text_host, len);
}

int64_t lmaze_foveal_visit_bytes(int32_t grid, int64_t n) {
    if (grid < 1 || grid > LMAZE_MAX_GRID || n < 0) return 0;
    const int64_t tb = visit_tiles(grid);
    return n * (tb * tb * (VT * VT) + VPC) * 4;      // tiles, then one "previous window" record per env
}

static int check_visit(const LmazeFovealParams* p, const LmazeFovealBuffers* b, const void* other, int64_t n) {
    if (!p || !b || !other || !b->visit || !b->visit_clock) return LMAZE_E_NULL;
    if (!foveal_grid_ok(p->grid)) return LMAZE_E_GRID;
    if (check_foveal_count(n)) return LMAZE_E_COUNT;
    if (((uintptr_t)b->visit & 63) || ((uintptr_t)other & 3)) return LMAZE_E_ALIGN;
    return 0;
}

int lmaze_foveal_materialise_visit(const LmazeFovealParams* params, const LmazeFovealBuffers* bufs, float* out, int64_t n,
                                   void* stream) {
    int rc = check_visit(params, bufs, out, n);
    if (rc) return rc;
    if (n == 0) return 0;
    const int64_t blocks = (n * params->grid * params->grid + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (!grid_ok(blocks)) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(visit_materialise_kernel, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(bufs->visit), bufs->visit_clock, out, n, params->grid);
    return (int)hipGetLastError();
}

int lmaze_foveal_load_visit(const LmazeFovealParams* params, const LmazeFovealBuffers* bufs, const float* in, int64_t n,
                            void* stream) {
    int rc = check_visit(params, bufs, in, n);
    if (rc) return rc;
    if (n == 0) return 0;
    const int64_t tb = visit_tiles(params->grid);
    const int64_t blocks = (n * tb * tb * (VT * VT) + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (!grid_ok(blocks)) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(visit_load_kernel, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, (hipStream_t)stream,
                       reinterpret_cast<uint32_t*>(bufs->visit), bufs->visit_clock, in, n, params->grid);
    return (int)hipGetLastError();
}

int lmaze_expand_planes(const float* planes, int32_t channels, int32_t g, int32_t expansion, float* out, int64_t n,
                        void* stream) {
    if (!planes || !out) return LMAZE_E_NULL;
    if (g < 1 || g > LMAZE_MAX_GRID) return LMAZE_E_GRID;
    if (expansion < 1 || expansion > 16 || channels < 1 || channels > 16) return LMAZE_E_EXPANSION;
    if (n < 0 || n > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    if (((uintptr_t)out & 15) || ((uintptr_t)planes & 3)) return LMAZE_E_ALIGN;
    if (n == 0) return 0;
    ExpandPlanesArgs a;
    a.planes = planes;
    a.out = out;
    a.n = n;
    a.channels = channels;
    a.g = g;
    a.expansion = expansion;
    if (g == FOV && expansion == 7 && !((uintptr_t)out & 63)) {
        // measured (262 144 envs, C = 4/5/7), round 1: 32 KiB x 8 per CU 5.2 TB/s; 48 KiB x 2 per CU + non-temporal 6.2-6.4
        // round 2 (C = 4 / 5 / 7, TB/s): 16 KiB x 3 per CU + non-temporal 6.50 / 6.45 / 6.57, 16 KiB x 4 6.26 / 6.54 / 6.27,
        // 48 KiB x 2 (round 1's choice) 6.48 / 6.37 / 6.23, 32 KiB x 2 6.26 / 6.26 / 6.21
        const int chunk = 4096;
        const int64_t total = n * (int64_t)channels * (FOV * 7) * (FOV * 7);
        const int64_t chunks = (total + chunk - 1) / chunk;
        if (grid_ok(chunks)) {
            size_t lds = ((size_t)(chunk / ((FOV * 7) * (FOV * 7)) + 3) * W25 * 4 + 15) & ~(size_t)15;   // planes touched + one of slack
            if (total * 4 > ((int64_t)192 << 20)) {
                const size_t cap = 160 * 1024, want = ((cap / 3 + cap / 4) / 2) & ~(size_t)255;      // 3 workgroups per CU
                if (want > lds) lds = want;
                hipLaunchKernelGGL((expand_planes_stream_kernel<FOV, 7, true>), dim3((unsigned)chunks), dim3(LMAZE_BLOCK), lds,
                                   (hipStream_t)stream, a, chunk);
            } else {
                hipLaunchKernelGGL((expand_planes_stream_kernel<FOV, 7, false>), dim3((unsigned)chunks), dim3(LMAZE_BLOCK), lds,
                                   (hipStream_t)stream, a, chunk);
            }
            return (int)hipGetLastError();
        }
    }
    const int S = g * expansion;
    const size_t lds = (((size_t)channels * g * g * 4 + (size_t)S * 4) + 15) & ~(size_t)15;
    const unsigned blocks = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(expand_planes_kernel, dim3(blocks), dim3(LMAZE_BLOCK), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
