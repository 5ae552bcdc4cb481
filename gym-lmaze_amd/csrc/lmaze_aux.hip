// lmaze_aux.hip -- the kernels either side of the step path: masked on-device reset
// (reference reset(): lmaze_env.py:64-110, lmaze_env_v3.py:134-167) and the
// reference-layout x E nearest-neighbour render (lmaze_env.py:217-234).
#include <stdio.h>

#include "lmaze_common.h"
#include "lmaze_learn.h"

namespace lmaze {


__device__ __forceinline__ void write_reset(const ResetArgs& a, int64_t e) {
    a.step_count[e] = 0;  // v0:110
    a.reward[e] = -0.0f;  // v0:109
    a.done[e] = 0;
}

// Shared layout: wave 0 compacts the accepted cells (row-major) into LDS once per
// workgroup, then one lane per env indexes the list.
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void reset_shared_kernel(const ResetArgs a) {
    extern __shared__ int4 lds4[];
    uint16_t* list = reinterpret_cast<uint16_t*>(lds4);
    __shared__ int count_s;
    const int G = a.grid, CELLS = G * G;
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int count = wave_build_spawn_list<VARIANT>(a.layout, G, CELLS, list, tid);
        if (tid == 0) count_s = count;
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * LMAZE_BLOCK + tid;
    if (e >= a.n) return;
    if (a.mask && !a.mask[e]) return;
    int ball_cell, goal_cell;
    place_from_list<VARIANT>(list, count_s, env_draw(a.seed, a.epoch, a.env_base + e), ball_cell, goal_cell);
    if (goal_cell >= 0) a.goal[e] = make_int2(goal_cell / G, goal_cell % G);
    if (ball_cell >= 0) a.ball[e] = make_int2(ball_cell / G, ball_cell % G);
    write_reset(a, e);
}

// Per-env layouts: one wave per env scans that env's G*G bytes (coalesced) with ballots.
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void reset_perenv_kernel(const ResetArgs a) {
    const int G = a.grid, CELLS = G * G;
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (LMAZE_BLOCK / 64) + (threadIdx.x >> 6);
    if (e >= a.n) return;
    if (a.mask && !a.mask[e]) return;
    int ball_cell, goal_cell;
    wave_place<VARIANT>(a.layout + (size_t)e * CELLS, G, CELLS, env_draw(a.seed, a.epoch, a.env_base + e), lane,
                        ball_cell, goal_cell);
    if (lane == 0) {
        if (goal_cell >= 0) a.goal[e] = make_int2(goal_cell / G, goal_cell % G);
        if (ball_cell >= 0) a.ball[e] = make_int2(ball_cell / G, ball_cell % G);
        write_reset(a, e);
    }
}

// Per-env layouts with G*G a multiple of 256: the layout is read once as dwords into registers
// (256 B per wave instruction) and ranked there (wave_place_regs), one wave per env.
template <int VARIANT, int G>
__global__ __launch_bounds__(LMAZE_BLOCK) void reset_perenv_wave_kernel(const ResetArgs a) {
    constexpr int CELLS = G * G, NJ = CELLS / 256;
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (LMAZE_BLOCK / 64) + (threadIdx.x >> 6);
    if (e >= a.n) return;
    if (a.mask && !a.mask[e]) return;
    const uint32_t* lay32 = reinterpret_cast<const uint32_t*>(a.layout + (size_t)e * CELLS);
    uint32_t w[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) w[j] = lay32[j * 64 + lane];
    int ball_cell, goal_cell;
    wave_place_regs<VARIANT, G, NJ>(w, env_draw(a.seed, a.epoch, a.env_base + e), lane, ball_cell, goal_cell);
    if (lane == 0) {
        if (goal_cell >= 0) a.goal[e] = make_int2(goal_cell / G, goal_cell % G);
        if (ball_cell >= 0) a.ball[e] = make_int2(ball_cell / G, ball_cell % G);
        write_reset(a, e);
    }
}

template <int G>
static bool launch_reset_wave(bool v3, const ResetArgs& a, unsigned blocks, hipStream_t s) {
    if (v3) hipLaunchKernelGGL((reset_perenv_wave_kernel<LMAZE_VARIANT_V3, G>), dim3(blocks), dim3(LMAZE_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((reset_perenv_wave_kernel<LMAZE_VARIANT_V0, G>), dim3(blocks), dim3(LMAZE_BLOCK), 0, s, a);
    return true;
}

hipError_t launch_reset(int variant, const ResetArgs& a, int layout_mode, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const bool v3 = variant == LMAZE_VARIANT_V3;
    if (layout_mode == LMAZE_LAYOUT_SHARED) {
        if (!grid_ok((a.n + LMAZE_BLOCK - 1) / LMAZE_BLOCK)) return hipErrorInvalidConfiguration;
        const unsigned blocks = (unsigned)((a.n + LMAZE_BLOCK - 1) / LMAZE_BLOCK);
        const size_t lds = ((size_t)a.grid * a.grid * 2 + 15) & ~(size_t)15;
        if (v3) hipLaunchKernelGGL(reset_shared_kernel<LMAZE_VARIANT_V3>, dim3(blocks), dim3(LMAZE_BLOCK), lds, s, a);
        else hipLaunchKernelGGL(reset_shared_kernel<LMAZE_VARIANT_V0>, dim3(blocks), dim3(LMAZE_BLOCK), lds, s, a);
    } else {
        const int epb = LMAZE_BLOCK / 64;
        if (!grid_ok((a.n + epb - 1) / epb)) return hipErrorInvalidConfiguration;
        const unsigned blocks = (unsigned)((a.n + epb - 1) / epb);
        const bool wave = (a.grid == 16 && launch_reset_wave<16>(v3, a, blocks, s)) ||
                          (a.grid == 32 && launch_reset_wave<32>(v3, a, blocks, s)) ||
                          (a.grid == 48 && launch_reset_wave<48>(v3, a, blocks, s)) ||
                          (a.grid == 64 && launch_reset_wave<64>(v3, a, blocks, s));
        if (wave) return hipGetLastError();
        if (v3) hipLaunchKernelGGL(reset_perenv_kernel<LMAZE_VARIANT_V3>, dim3(blocks), dim3(LMAZE_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(reset_perenv_kernel<LMAZE_VARIANT_V0>, dim3(blocks), dim3(LMAZE_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Reset from a start law (lmaze_reset_start): the ball cell is k = #{ j : row[j] <= u }, u the upper 31 bits of the reset
// draw's y, over a row of S cumulative words in units of 2^-31; k == S leaves the ball.  The v3 goal is lmaze_reset's own
// draw (or kept), and the row may be the goal's.  Nothing is read to validate a row: every index below is in [0, S).
// ------------------------------------------------------------------------------------

// the row of a v3 env under row_mode 2: its goal clamped onto the grid, as the closed-loop keys clamp it
__device__ __forceinline__ int goal_row(int2 g, int G) { return clampi(g.x, 0, G - 1) * G + clampi(g.y, 0, G - 1); }

// k for a non-decreasing row, without a branch: the largest k in [0, S] with row[k - 1] <= u, ceil(log2(S + 1)) probes
// from `top`, the power of two above S halved.  Any other row gives some k in [0, S].
__device__ __forceinline__ int row_search(const uint32_t* row, int S, int top, uint32_t u) {
    int k = 0;
    for (int b = top; b > 0; b >>= 1) {
        const int t = k + b;
        const uint32_t w = row[min(t, S) - 1];
        k = (t <= S && w <= u) ? t : k;
    }
    return k;
}

__device__ __forceinline__ void write_start(const ResetStartArgs& a, int64_t e, int k, int goal_cell) {
    const int G = a.r.grid;
    if (goal_cell >= 0) a.r.goal[e] = make_int2(goal_cell / G, goal_cell % G);
    if (k < G * G) a.r.ball[e] = make_int2(k / G, k % G);
    write_reset(a.r, e);
}

// Shared layout, one row (ROWS 0: staged in LDS once per workgroup) or the goal's row (ROWS 2: v3, read from global memory):
// one lane per env, as reset_shared_kernel.  LDS: the row's S words (ROWS 0), then, v3, the spawn list.
template <int VARIANT, int ROWS>
__global__ __launch_bounds__(LMAZE_BLOCK) void reset_start_kernel(const ResetStartArgs a) {
    extern __shared__ int4 lds4[];
    __shared__ int count_s;
    const int G = a.r.grid, S = G * G;
    const int tid = threadIdx.x;
    uint32_t* row_s = reinterpret_cast<uint32_t*>(lds4);
    uint16_t* list = reinterpret_cast<uint16_t*>(lds4 + (ROWS == 0 ? (S * 4 + 15) / 16 : 0));
    if (ROWS == 0)
        for (int j = tid; j < S; j += LMAZE_BLOCK) row_s[j] = a.thresholds[j];
    const bool draw_goal = VARIANT == LMAZE_VARIANT_V3 && !a.keep_goal;
    if (draw_goal && tid < 64) {
        const int count = wave_build_spawn_list<VARIANT>(a.r.layout, G, S, list, tid);
        if (tid == 0) count_s = count;
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * LMAZE_BLOCK + tid;
    if (e >= a.r.n) return;
    if (a.r.mask && !a.r.mask[e]) return;
    const uint4 r = env_draw(a.r.seed, a.r.epoch, a.r.env_base + e);
    int goal_cell = -1;
    if (draw_goal && count_s > 0) goal_cell = list[__umulhi(r.x, (uint32_t)count_s)];
    const uint32_t* row = row_s;
    if (ROWS == 2) row = a.thresholds + (size_t)(goal_cell >= 0 ? goal_cell : goal_row(a.r.goal[e], G)) * S;
    write_start(a, e, row_search(row, S, a.top, r.y >> 1), goal_cell);
}

// A row per env (row_mode 1), and every row mode on per-env layouts: one wave per env, as reset_perenv_kernel.  The wave
// reads the env's S words coalesced, compares them with u and sums the ballots' popcounts -- the count itself, whatever
// the row holds.  The v3 goal is ranked on the env's own layout.  Only lane 0 writes.
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void reset_start_wave_kernel(const ResetStartArgs a) {
    const int G = a.r.grid, S = G * G;
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (LMAZE_BLOCK / 64) + (threadIdx.x >> 6);
    if (e >= a.r.n) return;
    if (a.r.mask && !a.r.mask[e]) return;
    const uint4 r = env_draw(a.r.seed, a.r.epoch, a.r.env_base + e);
    int goal_cell = -1;
    if (VARIANT == LMAZE_VARIANT_V3 && !a.keep_goal) {
        const uint8_t* lay = a.r.layout + (a.per_env ? (size_t)e * S : (size_t)0);
        const int count = wave_count_cells<VARIANT>(lay, G, S, lane);
        if (count > 0) goal_cell = wave_kth_cell<VARIANT>(lay, G, S, (int)__umulhi(r.x, (uint32_t)count), lane);
    }
    size_t at = 0;
    if (a.row_mode == 1) at = (size_t)e;
    if (a.row_mode == 2) at = (size_t)(goal_cell >= 0 ? goal_cell : goal_row(a.r.goal[e], G));
    const uint32_t* row = a.thresholds + at * S;
    const uint32_t u = r.y >> 1;
    int k = 0;
    for (int base = 0; base < S; base += 256) {              // four loads in flight per lane; past the row: word 0, not counted
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = base + q * 64 + lane;
            w[q] = row[j < S ? j : 0];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) k += __popcll(__ballot(base + q * 64 + lane < S && w[q] <= u));
    }
    if (lane == 0) write_start(a, e, k, goal_cell);
}

// What lmaze_reset_start queues and lmaze_describe_reset_start prints: the lane-per-env kernel on a shared layout with one
// row (in LDS) or the goal's row (global), the wave-per-env kernel otherwise.
hipError_t launch_reset_start(int variant, const ResetStartArgs& args, int layout_mode, hipStream_t s, LaunchInfo* info) {
    if (args.r.n == 0) return hipSuccess;
    ResetStartArgs a = args;
    const bool v3 = variant == LMAZE_VARIANT_V3;
    const int S = a.r.grid * a.r.grid;
    a.per_env = layout_mode == LMAZE_LAYOUT_PER_ENV ? 1 : 0;
    a.top = 1;
    while (a.top * 2 <= S) a.top *= 2;                       // the largest power of two <= S: the first probe
    const bool lanes = !a.per_env && a.row_mode != 1;
    const int epb = lanes ? LMAZE_BLOCK : LMAZE_BLOCK / 64;
    const int64_t blocks = (a.r.n + epb - 1) / epb;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    const bool in_lds = lanes && a.row_mode == 0;
    const size_t lds = !lanes ? 0 : (in_lds ? ((size_t)S * 4 + 15) & ~(size_t)15 : 0) + (v3 ? ((size_t)S * 2 + 15) & ~(size_t)15 : 0);
    if (info) {
        char name[96];
        snprintf(name, sizeof(name), "reset_start_kernel<%s, rows=%s, table=%s>", v3 ? "v3" : "v0",
                 a.row_mode == 0 ? "one" : (a.row_mode == 1 ? "env" : "goal"), in_lds ? "lds" : "global");
        describe_launch(info, name, epb, 0, 1, false, blocks, LMAZE_BLOCK, lds);
        return hipSuccess;
    }
    const dim3 grid((unsigned)blocks), block(LMAZE_BLOCK);
    if (!lanes) {
        if (v3) hipLaunchKernelGGL(reset_start_wave_kernel<LMAZE_VARIANT_V3>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(reset_start_wave_kernel<LMAZE_VARIANT_V0>, grid, block, 0, s, a);
    } else if (a.row_mode == 0) {
        if (v3) hipLaunchKernelGGL((reset_start_kernel<LMAZE_VARIANT_V3, 0>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((reset_start_kernel<LMAZE_VARIANT_V0, 0>), grid, block, lds, s, a);
    } else {
        hipLaunchKernelGGL((reset_start_kernel<LMAZE_VARIANT_V3, 2>), grid, block, lds, s, a);   // the goal's row: v3 only
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Reference-layout render: out[i, c, x*E+xx, y*E+yy] = float((obs[i,x,y] & mask[c]) != 0)
// (lmaze_env.py:217-234, lmaze_env_v3.py:295-301).  Pure write stream: 4*C*(G*E)^2 bytes per env.
// ------------------------------------------------------------------------------------

// Any shape: one workgroup per env, the env's cells and two row/column maps in LDS, lanes stripe the
// env's contiguous C*S*S floats with 16-byte stores, index arithmetic by division.
__global__ __launch_bounds__(LMAZE_BLOCK) void render_expanded_generic_kernel(const ExpandArgs a) {
    extern __shared__ int4 lds4[];
    const int G = a.grid, E = a.expansion, C = a.channels;
    const int CELLS = G * G, S = G * E, PLANE = S * S, L = C * PLANE;
    int* cells = reinterpret_cast<int*>(lds4);                      // [CELLS]
    int* maskl = cells + CELLS;                                     // [LMAZE_MAX_CHANNELS]
    uint16_t* rowmap = reinterpret_cast<uint16_t*>(maskl + LMAZE_MAX_CHANNELS);  // [S] row -> (row / E) * G
    uint16_t* colmap = rowmap + S;                                  // [S] col -> col / E
    const int tid = threadIdx.x;
    if (tid < LMAZE_MAX_CHANNELS) maskl[tid] = tid < C ? a.mask[tid] : 0;
    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        __syncthreads();
        for (int k = tid; k < CELLS; k += LMAZE_BLOCK) cells[k] = a.obs[(size_t)i * CELLS + k];
        for (int k = tid; k < S; k += LMAZE_BLOCK) {
            rowmap[k] = (uint16_t)((k / E) * G);
            colmap[k] = (uint16_t)(k / E);
        }
        __syncthreads();
        const size_t B = (size_t)i * L;
        const size_t a0 = (B + 3) & ~(size_t)3, a1 = (B + L) & ~(size_t)3;
        const int head = (int)(a0 - B), nq = (int)((a1 - a0) >> 2);
        float4* out4 = reinterpret_cast<float4*>(a.out + a0);
        for (int q = tid - 1; q <= nq; q += LMAZE_BLOCK) {           // q = -1 / nq: the ragged head / tail
            const int first = q < 0 ? 0 : head + (q << 2);
            const int count = q < 0 ? head : (q == nq ? (int)(B + L - a1) : 4);
            int c = first / PLANE;
            const int rem = first - c * PLANE;
            int row = rem / S, col = rem - row * S;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < count) v[j] = (cells[rowmap[row] + colmap[col]] & maskl[c]) ? 1.0f : 0.0f;
                if (++col == S) {
                    col = 0;
                    if (++row == S) { row = 0; ++c; }
                }
            }
            if (count == 4) out4[q] = make_float4(v[0], v[1], v[2], v[3]);
            else
                for (int j = 0; j < count; ++j) a.out[B + first + j] = v[j];
        }
    }
}

// The reference's shapes (G, E at compile time: the flat index decodes by multiplication).  The output of
// the whole batch is ONE contiguous stream of N*C*S*S floats; workgroup w writes the aligned stretch
// [w*CH, (w+1)*CH) of it, whatever envs that covers (at most two, CH <= one env): an env is 94 864 B at
// 11x11 x7, so per-env workgroups start on 16-byte boundaries only and every 1-KB wave store straddles
// cache lines (5.3 TB/s); aligned 32-KB stretches reach 6 TB/s and more.
// LDS: for each of the two envs, cell bits by (grid row, output column): one read per output float.
template <int GT, int ET, bool NT>
__global__ __launch_bounds__(LMAZE_BLOCK) void render_expanded_stream_kernel(const ExpandArgs a) {
    constexpr int CELLS = GT * GT, S = GT * ET, PLANE = S * S;
    extern __shared__ int4 lds4[];
    int* cells = reinterpret_cast<int*>(lds4);                      // [2][CELLS]: the (at most) two envs of the stretch
    int* maskl = cells + 2 * CELLS;                                 // [LMAZE_MAX_CHANNELS]
    const int C = a.channels, L = C * PLANE, tid = threadIdx.x;
    const int64_t total = a.n * (int64_t)L;
    const int64_t f0 = (int64_t)blockIdx.x * a.chunk_floats;        // first float of this workgroup's stretch
    const int len = (int)min((int64_t)a.chunk_floats, total - f0);
    int64_t env0 = (int64_t)((double)f0 / (double)L);               // floor(f0 / L), fixed up below
    if (env0 * L > f0) --env0;
    if ((env0 + 1) * L <= f0) ++env0;
    const int off0 = (int)(f0 - env0 * L);
    const bool two = off0 + len > L;                                // the stretch runs into env0 + 1
    if (tid < LMAZE_MAX_CHANNELS) maskl[tid] = tid < C ? a.mask[tid] : 0;
    for (int k = tid; k < (two ? 2 * CELLS : CELLS); k += LMAZE_BLOCK) cells[k] = a.obs[(size_t)env0 * CELLS + k];
    __syncthreads();
    float* dst = a.out + f0;
    static_assert(ET >= 4, "four consecutive output columns span at most two cells");
    for (int q = tid; (q << 2) < len; q += LMAZE_BLOCK) {
        int local = off0 + (q << 2);
        const int* cl = cells;
        if (local >= L) { local -= L; cl += CELLS; }
        const int c = local / PLANE;
        const int rem = local - c * PLANE;
        const int row = rem / S, col = rem - row * S;
        // One path for every lane (with S = 77 every wave holds float4s that straddle an output row, so a
        // branch would cost both sides): the cell under the first column, the next cell of the same grid
        // row, and the first cell of the following output row -- which may belong to the next plane / env.
        const int* r0 = cl + (row / ET) * GT;
        const int k0 = col / ET;
        const int m0 = maskl[c];
        const int b0 = r0[k0] & m0, b1 = r0[k0 + 1] & m0;             // r0[GT] is read but never selected
        int row1 = row + 1, c1 = c;
        const int* cl1 = cl;
        if (row1 == S) {
            row1 = 0;
            if (++c1 == C) { c1 = 0; cl1 = cells + CELLS; }              // ragged C*S*S only
        }
        const int bw = cl1[(row1 / ET) * GT] & maskl[c1];
        const int edge = (k0 + 1) * ET;                                // first column of the next cell
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cj = col + j;
            v[j] = (cj >= S ? bw : (cj >= edge ? b1 : b0)) ? 1.0f : 0.0f;
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
// Episode statistics: four integer sums over the batch (grid-stride, wave shuffles, one 64-bit
// atomic per workgroup and counter)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(LMAZE_BLOCK) void episode_stats_kernel(const uint8_t* done, const float* reward,
                                                                    const int32_t* step_count, const int32_t* goal_count,
                                                                    float reward_goal, int64_t n,
                                                                    unsigned long long* out4) {
    long long acc[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LMAZE_BLOCK) {
        const bool d = done[i] != 0;
        acc[0] += d;
        acc[1] += reward[i] == reward_goal;
        acc[2] += d ? step_count[i] : 0;
        if (goal_count) acc[3] += goal_count[i];
    }
    __shared__ long long part[4][LMAZE_BLOCK / 64];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        long long v = 0;
        for (int w = 0; w < LMAZE_BLOCK / 64; ++w) v += part[threadIdx.x][w];
        if (v) atomicAdd(out4 + threadIdx.x, (unsigned long long)v);
    }
}

hipError_t launch_episode_stats(const uint8_t* done, const float* reward, const int32_t* step_count,
                                const int32_t* goal_count, float reward_goal, int64_t n, int64_t* out4, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out4, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess || n == 0) return e;
    int64_t blocks = (n + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(episode_stats_kernel, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, s, done, reward, step_count,
                       goal_count, reward_goal, n, reinterpret_cast<unsigned long long*>(out4));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Discounted returns-to-go over trajectory rows (lmaze_returns): ret[t] = r[t] where done[t], else r[t] + gamma * ret[t+1],
// ret[T] = tail (0 when null) -- a reverse scan with a restart at every done.  One lane per env walks t = T-1 .. 0; the
// product and the sum are rounded separately (never an fma), so a float32 loop on the host reproduces every bit.  Only
// ret is a dependent chain: the rows are loaded RETURNS_ROWS at a time before it, all in flight at once, and stored after.
// A lane reads row t of its own column before it stores it and touches no other column, so returns_t may be reward_t.
// ------------------------------------------------------------------------------------
#define RETURNS_ROWS 8
// r + gamma * ret as two roundings, __fadd_rn(r, __fmul_rn(gamma, ret)) in effect: those two are inline functions whose
// operators carry the translation unit's contraction licence and fuse into one v_fma_f32, so the operators stand here
// themselves, under a pragma that takes the licence away
__device__ __forceinline__ float returns_step(float r, float gamma, float ret) {
#pragma clang fp contract(off)
    const float discounted = gamma * ret;
    return r + discounted;
}
__global__ __launch_bounds__(LMAZE_BLOCK) void returns_kernel(const float* reward_t, const uint8_t* done_t, const float* tail,
                                                              float gamma, float* returns_t, int32_t T, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    if (i >= n) return;
    float ret = tail ? tail[i] : 0.0f;
    for (int t0 = T - 1; t0 >= 0; t0 -= RETURNS_ROWS) {
        float r[RETURNS_ROWS];
        uint8_t d[RETURNS_ROWS];
#pragma unroll
        for (int j = 0; j < RETURNS_ROWS; ++j) {
            const bool in = t0 - j >= 0;
            const size_t at = (size_t)(in ? t0 - j : 0) * n + i;
            r[j] = in ? reward_t[at] : 0.0f;
            d[j] = in ? done_t[at] : (uint8_t)0;
        }
#pragma unroll
        for (int j = 0; j < RETURNS_ROWS; ++j) {
            if (t0 - j < 0) break;
            ret = d[j] ? r[j] : returns_step(r[j], gamma, ret);
            returns_t[(size_t)(t0 - j) * n + i] = ret;
        }
    }
}

hipError_t launch_returns(const float* reward_t, const uint8_t* done_t, const float* tail, float gamma, float* returns_t,
                          int32_t T, int64_t n, hipStream_t s) {
    if (T <= 0 || n == 0) return hipSuccess;
    const int64_t blocks = (n + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(returns_kernel, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, s, reward_t, done_t, tail, gamma, returns_t, T, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// GAE(lambda) over trajectory rows (lmaze_advantages / lmaze_advantages_table): returns_kernel's shape -- one lane per env
// walks t = T-1 .. 0, the rows are loaded ADV_ROWS at a time before the dependent chain (adv, and the value of the row
// behind) and stored after it.  TABLE: a value is values[key] for 0 <= key < keys and 0 otherwise; the eight key loads, then
// the eight gathers are issued before the chain, each gather unconditional on an index that is 0 for a key out of range
// (keys >= 1), so nothing is read past the table and no load waits on a branch.  A lane reads the rows of its own column
// before it stores them and touches no other column: adv_t may be reward_t and target_t may be value_t.
// ------------------------------------------------------------------------------------
#define ADV_ROWS 8
template <bool TABLE>
__global__ __launch_bounds__(LMAZE_BLOCK) void advantages_kernel(const AdvantageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const size_t n = (size_t)a.n;
    float v_next;
    if (TABLE) v_next = a.key_tail ? table_value(a.values, a.keys, a.key_tail[i]) : 0.0f;
    else v_next = a.tail ? a.tail[i] : 0.0f;
    float adv = 0.0f;
    for (int t0 = a.T - 1; t0 >= 0; t0 -= ADV_ROWS) {
        float r[ADV_ROWS], v[ADV_ROWS], out[ADV_ROWS];
        uint8_t d[ADV_ROWS];
        int32_t k[ADV_ROWS];
#pragma unroll
        for (int j = 0; j < ADV_ROWS; ++j) {
            const bool in = t0 - j >= 0;
            const size_t at = (size_t)(in ? t0 - j : 0) * n + i;
            r[j] = in ? a.reward_t[at] : 0.0f;
            d[j] = in ? a.done_t[at] : (uint8_t)0;
            if (TABLE) k[j] = in ? a.key_t[at] : -1;
            else v[j] = in ? a.value_t[at] : 0.0f;
        }
        if (TABLE) {
#pragma unroll
            for (int j = 0; j < ADV_ROWS; ++j) v[j] = table_value(a.values, a.keys, k[j]);
        }
#pragma unroll
        for (int j = 0; j < ADV_ROWS; ++j) {
            if (t0 - j < 0) break;
            adv = lmaze_gae_step(r[j], d[j], v[j], v_next, a.gamma, a.gl, adv);
            out[j] = adv;
            v_next = v[j];
        }
#pragma unroll
        for (int j = 0; j < ADV_ROWS; ++j) {
            if (t0 - j < 0) break;
            const size_t at = (size_t)(t0 - j) * n + i;
            a.adv_t[at] = out[j];
            if (a.target_t) a.target_t[at] = lmaze_gae_target(out[j], v[j]);
        }
    }
}

hipError_t launch_advantages(const AdvantageArgs& a, hipStream_t s) {
    if (a.T <= 0 || a.n == 0) return hipSuccess;
    const int64_t blocks = (a.n + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    if (a.values) hipLaunchKernelGGL(advantages_kernel<true>, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(advantages_kernel<false>, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Counts and Q24 sums per (key, action) (lmaze_table_stats).  Integer accumulation: the sums do not depend on the order
// the samples arrive in, so the two paths and any two runs give the same 64 bits.
//   LDS:    every workgroup keeps count[bins] and sum[bins] (8 bytes each) in LDS, grid-strides over the samples with LDS
//           atomics and flushes its non-zero bins with one 64-bit global atomic add each.
//   global: 64-bit global atomics per sample.
// The rows are read as 16-byte vectors between a scalar head (up to the first 16-byte boundary of key_t) and a scalar tail
// where the given rows share key_t's offset within 16 bytes; otherwise (rows sliced differently) sample by sample.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void table_add(unsigned long long* cnt, unsigned long long* sum, const TableStatsArgs& a, int32_t key,
                                          int32_t action, float w) {
    const int32_t bin = lmaze_table_bin(key, action, a.keys, a.actions);
    if (bin < 0) return;
    if (sum && !lmaze_q24_ok(w)) return;
    atomicAdd(cnt + bin, 1ull);
    if (sum) atomicAdd(sum + bin, (unsigned long long)lmaze_q24(w));
}

template <bool LDS>
__global__ __launch_bounds__(LMAZE_BLOCK) void table_stats_kernel(const TableStatsArgs a, int32_t bins, int32_t head, int64_t nvec) {
    extern __shared__ int4 lds4[];
    unsigned long long* cnt = a.count;
    unsigned long long* sum = a.total;
    if (LDS) {
        unsigned long long* tab = reinterpret_cast<unsigned long long*>(lds4);       // count[bins], sum[bins]
        for (int b = threadIdx.x; b < 2 * bins; b += LMAZE_BLOCK) tab[b] = 0;
        __syncthreads();
        cnt = tab;
        sum = a.total ? tab + bins : nullptr;
    }
    const int64_t tid = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * LMAZE_BLOCK;
    const int64_t vend = head + 4 * nvec, nscalar = a.m - 4 * nvec;   // samples [0, head) and [vend, m) one by one
    for (int64_t s = tid; s < nscalar; s += stride) {
        const int64_t at = s < head ? s : s - head + vend;
        table_add(cnt, sum, a, a.key_t[at], a.actions_t ? a.actions_t[at] : 0, a.weight_t ? a.weight_t[at] : 0.0f);
    }
    const int4* k4 = reinterpret_cast<const int4*>(a.key_t + head);
    const int4* a4 = a.actions_t ? reinterpret_cast<const int4*>(a.actions_t + head) : nullptr;
    const float4* w4 = a.weight_t ? reinterpret_cast<const float4*>(a.weight_t + head) : nullptr;
    for (int64_t q = tid; q < nvec; q += stride) {
        const int4 k = k4[q];
        const int4 ac = a4 ? a4[q] : make_int4(0, 0, 0, 0);
        const float4 w = w4 ? w4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        table_add(cnt, sum, a, k.x, ac.x, w.x);
        table_add(cnt, sum, a, k.y, ac.y, w.y);
        table_add(cnt, sum, a, k.z, ac.z, w.z);
        table_add(cnt, sum, a, k.w, ac.w, w.w);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < bins; b += LMAZE_BLOCK) {
            const unsigned long long c = cnt[b];
            if (!c) continue;                                    // a bin no sample of this workgroup fell into
            atomicAdd(a.count + b, c);
            if (sum && sum[b]) atomicAdd(a.total + b, sum[b]);
        }
    }
}

// Where the table lives is a rule (include/lmaze.h): up to LMAZE_TABLE_LDS_BINS bins in LDS, sized to the table.  One
// launch for any m: a lane takes four samples per turn and the grid is capped, as episode_stats_kernel's.
TableStatsPlan plan_table_stats(int64_t m, int64_t keys, int32_t actions) {
    TableStatsPlan p;
    p.bins = keys * actions;
    p.lds = p.bins <= LMAZE_TABLE_LDS_BINS;
    p.lds_bytes = p.lds ? 16 * p.bins : 0;
    p.grid = (m + 4 * LMAZE_BLOCK - 1) / (4 * LMAZE_BLOCK);
    const int64_t cap = p.lds ? 1024 : 2048;                     // LDS: every workgroup also flushes its table
    if (p.grid > cap) p.grid = cap;
    if (p.grid < 1) p.grid = 1;
    return p;
}

hipError_t launch_table_stats(const TableStatsArgs& a, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const TableStatsPlan p = plan_table_stats(a.m, a.keys, (int32_t)a.actions);
    const uintptr_t off = (uintptr_t)a.key_t & 15;
    const bool vec = (!a.actions_t || ((uintptr_t)a.actions_t & 15) == off) && (!a.weight_t || ((uintptr_t)a.weight_t & 15) == off);
    int64_t head = vec ? (int64_t)(((16 - off) & 15) >> 2) : 0;
    if (head > a.m) head = a.m;
    const int64_t nvec = vec ? (a.m - head) >> 2 : 0;
    if (p.lds)
        hipLaunchKernelGGL(table_stats_kernel<true>, dim3((unsigned)p.grid), dim3(LMAZE_BLOCK), (size_t)p.lds_bytes, s, a,
                           (int32_t)p.bins, (int32_t)head, nvec);
    else
        hipLaunchKernelGGL(table_stats_kernel<false>, dim3((unsigned)p.grid), dim3(LMAZE_BLOCK), 0, s, a, (int32_t)p.bins,
                           (int32_t)head, nvec);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// measured ceilings of the box ("a measured fill/copy-kernel ceiling on the same box"):
// ONE 16-byte access per thread in launch order, the pattern that reaches the highest write rate here.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LMAZE_BLOCK) void probe_fill_kernel(int4* dst, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    if (i < n16) dst[i] = make_int4((int)i, 1, 2, 3);
}

__global__ __launch_bounds__(LMAZE_BLOCK) void probe_copy_kernel(const int4* __restrict__ src, int4* __restrict__ dst,
                                                                 int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * LMAZE_BLOCK + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

hipError_t launch_probe(const void* src, void* dst, int64_t bytes, hipStream_t s) {
    const int64_t n16 = bytes / 16;
    if (n16 == 0) return hipSuccess;
    const int64_t blocks = (n16 + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
    if (!grid_ok(blocks)) return hipErrorInvalidConfiguration;
    if (src)
        hipLaunchKernelGGL(probe_copy_kernel, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, s,
                           static_cast<const int4*>(src), static_cast<int4*>(dst), n16);
    else
        hipLaunchKernelGGL(probe_fill_kernel, dim3((unsigned)blocks), dim3(LMAZE_BLOCK), 0, s, static_cast<int4*>(dst), n16);
    return hipGetLastError();
}

static hipError_t launch_expand_generic(const ExpandArgs& a, hipStream_t s) {
    const int S = a.grid * a.expansion;
    const unsigned blocks = (unsigned)(a.n < 65536 ? a.n : 65536);
    const size_t lds = (((size_t)a.grid * a.grid * 4 + LMAZE_MAX_CHANNELS * 4 + (size_t)S * 4) + 15) & ~(size_t)15;
    hipLaunchKernelGGL(render_expanded_generic_kernel, dim3(blocks), dim3(LMAZE_BLOCK), lds, s, a);
    return hipGetLastError();
}

// E = 1: the reference's unexpanded planes float32[N,C,G,G] (what it calls retState, lmaze_env.py:208-215) --
// the layout a policy network takes.  Any G.  Same aligned-stretch scheme: the workgroup stages the cells of
// the few envs its stretch covers (contiguous in obs; 16-byte loads when aligned, four dword loads in flight
// per lane otherwise) and every lane turns four consecutive output floats into one 16-byte store.  (Reading
// the cells per lane straight from obs instead: 2.0-3.6 TB/s.)  The two divisions of the index decode are
// multiplications by reciprocals the host computed (exact for the < 2^17 values that occur).
template <bool NT>
__global__ __launch_bounds__(LMAZE_BLOCK) void render_planes_stream_kernel(const ExpandArgs a) {
    extern __shared__ int4 lds4[];
    int* cells = reinterpret_cast<int*>(lds4);                      // [envs of the stretch][CELLS] (+ slack)
    const int G = a.grid, C = a.channels, CELLS = G * G, L = C * CELLS, tid = threadIdx.x;
    const int64_t total = a.n * (int64_t)L;
    const int64_t f0 = (int64_t)blockIdx.x * a.chunk_floats;
    const int len = (int)min((int64_t)a.chunk_floats, total - f0);
    int64_t env0 = (int64_t)((double)f0 / (double)L);               // floor(f0 / L), fixed up below
    if (env0 * L > f0) --env0;
    if ((env0 + 1) * L <= f0) ++env0;
    const int off0 = (int)(f0 - env0 * L);
    const int ne = (int)min((int64_t)((off0 + len + L - 1) / L), a.n - env0);
    __shared__ int maskl[LMAZE_MAX_CHANNELS + 1];
    if (tid <= LMAZE_MAX_CHANNELS) maskl[tid] = tid < C ? a.mask[tid] : 0;
    {
        const int32_t* src = a.obs + (size_t)env0 * CELLS;
        const int nint = ne * CELLS;
        if ((((uintptr_t)src) & 15) == 0) {                          // 16-byte loads when the first env starts aligned
            const int n4 = nint >> 2;
            for (int k = tid; k < n4; k += LMAZE_BLOCK) reinterpret_cast<int4*>(cells)[k] = reinterpret_cast<const int4*>(src)[k];
            for (int k = (n4 << 2) + tid; k < nint; k += LMAZE_BLOCK) cells[k] = src[k];
        } else {
            for (int k = tid; k < nint; k += 4 * LMAZE_BLOCK) {      // four loads in flight per lane
                int v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (k + u * LMAZE_BLOCK < nint) ? src[k + u * LMAZE_BLOCK] : 0;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u * LMAZE_BLOCK < nint) cells[k + u * LMAZE_BLOCK] = v[u];
            }
        }
    }
    __syncthreads();
    float* dst = a.out + f0;
    for (int q = tid; (q << 2) < len; q += LMAZE_BLOCK) {
        const uint32_t local = (uint32_t)(off0 + (q << 2));
        const uint32_t le = (uint32_t)(((uint64_t)local * a.inv_l) >> 32);           // env of the stretch
        const uint32_t rem = local - le * (uint32_t)L;
        const uint32_t c = (uint32_t)(((uint64_t)rem * a.inv_cells) >> 32);          // plane
        const int cell = (int)(rem - c * (uint32_t)CELLS);
        const bool last = (int)c + 1 == C;
        const int* r0 = cells + le * CELLS;
        const int* r1 = last ? r0 + CELLS : r0;
        const int m0 = maskl[c], m1 = maskl[last ? 0 : c + 1];
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cj = cell + j;
            v[j] = (cj < CELLS ? (r0[cj] & m0) : (r1[cj - CELLS] & m1)) ? 1.0f : 0.0f;
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

// LDS bytes that make exactly `k` workgroups fit a CU's 160 KiB (as for the step kernel, lmaze_step.hip)
static size_t expand_lds_for_workgroups_per_cu(int k) {
    const size_t cap = 160 * 1024;
    return ((cap / k + cap / (k + 1)) / 2) & ~(size_t)255;
}

// Launch policy, measured on MI355X (65 536 envs, 6.2 GB of output; TB/s):
//   stretch x workgroups per CU      32 KiB x 8   32 KiB x 3 + NT   48 KiB x 3 + NT   64 KiB x 3
//   11x11 x7                            5.7            6.2               5.4              6.4 / erratic
//   12x12 x7                            5.4            6.2               5.6              6.3 / erratic
//   18x18 x4                            6.2            6.2               6.0              4.6
//   32x32 x7                            5.3            5.7               6.2              3.8
// The same narrow optimum as the step kernel: ~96 KiB of non-temporal stores in flight per CU.
template <int GT, int ET>
static hipError_t launch_expand_stream(const ExpandArgs& a, hipStream_t s) {
    constexpr int S = GT * ET;
    const int64_t L = (int64_t)a.channels * S * S, total = a.n * L;
    ExpandArgs b = a;
    // Round 2 (65 536 envs, two processes, TB/s; stretch x workgroups per CU, non-temporal): 11x11 x7 16 KiB x 5 6.61,
    // 16 KiB x 6 6.35, 32 KiB x 3 (round 1's choice) 6.2; 12x12 x7 6.56-6.59 / 6.54-6.58 / 6.22; 18x18 x4 6.62 / 6.88-6.92 /
    // 6.2-6.3; 32x32 x7 5.95 / 5.8 / 5.7 against 48 KiB x 3 6.21-6.26.  Plain stores reach 6.6-6.8 on single shapes and
    // fall to 3.6-4.8 on others; 4- and 8-KiB stretches lose to the per-workgroup index set-up (2.0-4.5).
    b.chunk_floats = GT >= 32 ? 12288 : 4096;                        // 48 / 16 KiB per workgroup
    const int per_cu = GT >= 32 ? 3 : (GT == 18 ? 6 : 5);
    if (b.chunk_floats > L) b.chunk_floats = (int32_t)(L & ~(int64_t)1023);   // a stretch covers two envs at most
    if (b.chunk_floats < 1024) return launch_expand_generic(a, s);
    const int64_t chunks = (total + b.chunk_floats - 1) / b.chunk_floats;
    // out must start on a cache line for the stretches to be aligned
    if (!grid_ok(chunks) || ((uintptr_t)a.out & 63)) return launch_expand_generic(a, s);
    size_t lds = ((size_t)2 * GT * GT * 4 + LMAZE_MAX_CHANNELS * 4 + 15) & ~(size_t)15;
    const bool nt = total * 4 > ((int64_t)192 << 20);                // cannot stay in the 256 MiB Infinity Cache
    if (nt) {
        const size_t want = expand_lds_for_workgroups_per_cu(per_cu);
        if (want > lds) lds = want;
        hipLaunchKernelGGL((render_expanded_stream_kernel<GT, ET, true>), dim3((unsigned)chunks), dim3(LMAZE_BLOCK), lds, s, b);
    } else {
        hipLaunchKernelGGL((render_expanded_stream_kernel<GT, ET, false>), dim3((unsigned)chunks), dim3(LMAZE_BLOCK), lds, s, b);
    }
    return hipGetLastError();
}

static hipError_t launch_planes_stream(const ExpandArgs& a, hipStream_t s) {
    const int64_t cells = (int64_t)a.grid * a.grid, L = a.channels * cells, total = a.n * L;
    ExpandArgs b = a;
    b.chunk_floats = 4096;                                           // 16 KiB per workgroup (round 2: 6.14 / 6.40 TB/s at
                                                                     // 1M x 11x11 / 256K x 32x32 against 5.93 / 6.03 with 32 KiB)
    const int64_t chunks = (total + b.chunk_floats - 1) / b.chunk_floats;
    if (cells < 4 || !grid_ok(chunks) || ((uintptr_t)a.out & 63)) return launch_expand_generic(a, s);
    b.inv_l = (((uint64_t)1 << 32) + (uint64_t)L - 1) / (uint64_t)L;
    b.inv_cells = (((uint64_t)1 << 32) + (uint64_t)cells - 1) / (uint64_t)cells;
    size_t lds = ((size_t)(b.chunk_floats / L + 3) * cells * 4 + 15) & ~(size_t)15;
    // read + write stream (the input is 20 % of the traffic): as for the per-env step kernel, capping the
    // occupancy only hurts -- 1M x 11x11: 5.9 TB/s uncapped, 5.0 at 4 workgroups per CU, 4.1 at 3
    if (total * 4 > ((int64_t)192 << 20)) {
        hipLaunchKernelGGL((render_planes_stream_kernel<true>), dim3((unsigned)chunks), dim3(LMAZE_BLOCK), lds, s, b);
    } else {
        hipLaunchKernelGGL((render_planes_stream_kernel<false>), dim3((unsigned)chunks), dim3(LMAZE_BLOCK), lds, s, b);
    }
    return hipGetLastError();
}

hipError_t launch_expand(const ExpandArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (a.expansion == 1) return launch_planes_stream(a, s);
    // the reference's own shapes (v0 12x12 x7, v3 18x18 x4) and BASELINE's grids at x7
    if (a.expansion == 7) {
        if (a.grid == 12) return launch_expand_stream<12, 7>(a, s);
        if (a.grid == 11) return launch_expand_stream<11, 7>(a, s);
        if (a.grid == 8) return launch_expand_stream<8, 7>(a, s);
        if (a.grid == 32) return launch_expand_stream<32, 7>(a, s);
    }
    if (a.expansion == 4 && a.grid == 18) return launch_expand_stream<18, 4>(a, s);
    return launch_expand_generic(a, s);
}

}  // namespace lmaze
