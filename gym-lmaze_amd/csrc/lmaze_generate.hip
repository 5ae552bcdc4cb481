// lmaze_generate.hip -- spanning-tree mazes, one per env (lmaze_generate / lmaze_describe_generate, include/lmaze.h).
//
// One maze = R*R rooms on the odd cells of a G x G grid, R = (G - 1) / 2, and the up to 2 R (R - 1) wall cells between
// neighbouring rooms.  Every room draws once (Philox, counter (maze, room, 0x40000000)): a weight and a loop draw for the
// edge below it and for the edge to its right.  The edges that are opened are the minimum spanning tree under the keys
// (weight & 0xFFFFF800) | edge -- distinct within a maze, so the tree is unique and any schedule that finds it finds the same
// bytes -- plus the non-tree edges whose loop draw is below loops_u32.
//
// The tree is found by Boruvka rounds in LDS.  A round: every edge whose two rooms carry different labels offers its key to
// both labels (ds_min_u32: the minimum does not depend on the order); every component hooks onto the component across its
// minimum edge, the smaller label of a pair that picked each other staying root; pointers are jumped until every component
// points at its root; rooms take their root's label.  A round at least halves the number of components and a jump pass at
// least halves the depth of the hook forest, so both loops run at most ceil(log2(R*R)) times, a count fixed before they
// start; a uniform vote that nothing is left ends them sooner.  A mistake here writes wrong bytes and still returns.
//
// A maze lives in LDS from its draws to its bytes: keys, labels, minima, pointers, the cell index of every room, and the
// G*G bytes, which start as 'W' and are opened in place.  Global memory is only written.  Two forms, picked from G alone
// (plan_generate):
//   wave        G <= 33 (R*R <= 256): a wave per maze, four mazes per workgroup, 1-4 rooms per lane; phases are separated by
//               a wave-level fence, no workgroup barrier, and a wave without a maze (the ragged last workgroup) leaves at once.
//   workgroup   above: a workgroup per maze, 1-4 rooms per lane, __syncthreads() between phases; a vote is a word per wave,
//               written before a barrier and read by every thread after it, two parities of words keeping a fast wave's next
//               vote off a slow wave's read.
#include <stdio.h>

#include "lmaze_common.h"

namespace lmaze {

#define GEN_NONE 0xFFFFFFFFu          // no edge / no offer: no key ends in eleven set bits (edge indices stay below 1922)
#define GEN_STREAM 0x40000000u        // last counter word of the generator's draws
#define GEN_KEY_MASK 0xFFFFF800u
#define GEN_VOTE_BYTES 32             // workgroup form: 2 x 4 vote words
#define GEN_WALLS 0x57575757u         // four 'W'

// Where one maze's arrays stand in its share of the LDS, every offset a multiple of 16
struct GenerateLds {
    int32_t key, comp, best, parent, rcell, cells, bytes;
};
__host__ __device__ inline int up16(int bytes) { return (bytes + 15) & ~15; }
__host__ __device__ inline GenerateLds generate_lds(int G) {
    const int R = (G - 1) / 2, RR = R * R, S = G * G;
    GenerateLds L;
    L.key = 0;                                  // uint32[2 RR]  key of edge k, GEN_NONE where the edge does not exist
    L.comp = L.key + up16(8 * RR);                // int32[RR]     label of a room: the room that is its component's root
    L.best = L.comp + up16(4 * RR);               // uint32[RR]    by label: the least key offered this round
    L.parent = L.best + up16(4 * RR);             // int32[RR]     by label: the label hooked onto
    L.rcell = L.parent + up16(4 * RR);            // uint16[RR]    cell index of a room
    L.cells = L.rcell + up16(2 * RR);             // uint8[3 + S + 3]  the bytes, shifted by the maze's offset mod 4 in `layouts`
    L.bytes = L.cells + up16(S + 6);
    return L;
}

template <bool WAVE>
__device__ __forceinline__ void generate_sync() {
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// "does any thread of the maze say so": the same answer in every thread of the maze, and a generate_sync on the way
template <bool WAVE>
__device__ __forceinline__ bool generate_any(bool mine, uint32_t* vote, int& votes, int lane, int wave) {
    const bool any = __ballot(mine) != 0ull;
    if constexpr (WAVE) {
        generate_sync<true>();
        return any;
    } else {
        uint32_t* const v = vote + (votes++ & 1) * 4;
        if (lane == 0) v[wave] = any ? 1u : 0u;
        __syncthreads();
        return (v[0] | v[1] | v[2] | v[3]) != 0u;
    }
}

template <bool WAVE, int RPL>
__global__ __launch_bounds__(LMAZE_BLOCK) void generate_kernel(const GenerateArgs a) {
    constexpr int TPP = WAVE ? 64 : LMAZE_BLOCK;        // threads per maze
    constexpr int MPW = LMAZE_BLOCK / TPP;              // mazes per workgroup
    extern __shared__ __align__(16) unsigned char generate_lds_base[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = WAVE ? lane : (int)threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * MPW + (WAVE ? wave : 0);
    // wave form: a whole wave without a maze, and no barrier in that form waits for it; workgroup form: never
    if (p >= a.mazes) return;
    const int G = a.grid, S = G * G, R = (G - 1) >> 1, RR = R * R;
    const GenerateLds L = generate_lds(G);
    unsigned char* const mine = generate_lds_base + (WAVE ? wave : 0) * L.bytes;
    uint32_t* const key = reinterpret_cast<uint32_t*>(mine + L.key);
    int32_t* const comp = reinterpret_cast<int32_t*>(mine + L.comp);
    uint32_t* const best = reinterpret_cast<uint32_t*>(mine + L.best);
    int32_t* const parent = reinterpret_cast<int32_t*>(mine + L.parent);
    uint16_t* const rcell = reinterpret_cast<uint16_t*>(mine + L.rcell);
    uint32_t* const cellw = reinterpret_cast<uint32_t*>(mine + L.cells);
    uint32_t* const vote = reinterpret_cast<uint32_t*>(generate_lds_base + (size_t)MPW * L.bytes);   // workgroup form only
    // byte s of the maze goes to layouts[first + s]; in LDS it stands `mis` bytes into cellw, so that an aligned dword of
    // global memory is an aligned dword of LDS
    const int64_t first = p * S;
    const int mis = (int)(first & 3);
    uint8_t* const cells = reinterpret_cast<uint8_t*>(cellw) + mis;
    const uint64_t m = (uint64_t)(a.maze_base + p);
    const uint2 k2 = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));

    for (int w = t; w < ((mis + S + 3) >> 2); w += TPP) cellw[w] = GEN_WALLS;
    generate_sync<WAVE>();
    // The draws.  Slot r < RR is room r: keys, the room's own cell, the loops.  Slot RR is the goal's draw; it rides in a spare
    // turn of a lane wherever the maze's threads have one (RPL * TPP > RR: every R but 8 and 16) and is thread 0's extra turn
    // otherwise -- a whole wave would pay for a Philox call of its own.  q / R == (q * rdiv) >> 16 for q < 1024, R <= 31: the
    // excess of rdiv over 65536 / R is below 1, so the quotient gains less than 1024 / 65536 < 1 / R.
    const uint32_t rdiv = (65536u + (uint32_t)R - 1u) / (uint32_t)R;
    int goal_cell = -1, gx = 0, gy = 0;
#pragma unroll
    for (int j = 0; j <= RPL; ++j) {
        const int r = t + j * TPP;
        if (r <= RR) {
            const uint4 d = philox4x32_10(make_uint4((uint32_t)m, (uint32_t)(m >> 32), (uint32_t)r, GEN_STREAM), k2);
            const int q = r < RR ? r : (int)__umulhi(d.x, (uint32_t)RR);        // the room whose cell this slot names
            const int qi = (int)(((uint32_t)q * rdiv) >> 16), qj = q - qi * R;
            const int cx = 1 + 2 * qi, cy = 1 + 2 * qj, c = cx * G + cy;
            if (r == RR) {
                goal_cell = c;
                gx = cx;
                gy = cy;
            } else {
                const bool down = qi + 1 < R, right = qj + 1 < R;
                key[2 * r] = down ? ((d.x & GEN_KEY_MASK) | (uint32_t)(2 * r)) : GEN_NONE;
                key[2 * r + 1] = right ? ((d.y & GEN_KEY_MASK) | (uint32_t)(2 * r + 1)) : GEN_NONE;
                comp[r] = r;
                rcell[r] = (uint16_t)c;
                cells[c] = 'B';
                if (down && d.z < a.loops_u32) cells[c + G] = 'B';      // loops_u32 == 0: never
                if (right && d.w < a.loops_u32) cells[c + 1] = 'B';
            }
        }
    }
    generate_sync<WAVE>();

    const int bound = 32 - __clz(RR - 1);               // ceil(log2(RR)), RR >= 4
    int votes = 0;
    for (int round = 0; round < bound; ++round) {
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int r = t + j * TPP;
            if (r < RR) best[r] = GEN_NONE;
        }
        generate_sync<WAVE>();
        // every edge between two components offers its key to both
        bool outgoing = false;
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int r = t + j * TPP;
            if (r < RR) {
                const int cu = comp[r];
                const uint32_t kd = key[2 * r], kr = key[2 * r + 1];
                if (kd != GEN_NONE) {
                    const int cv = comp[r + R];
                    if (cv != cu) {
                        atomicMin(&best[cu], kd);
                        atomicMin(&best[cv], kd);
                        outgoing = true;
                    }
                }
                if (kr != GEN_NONE) {
                    const int cv = comp[r + 1];
                    if (cv != cu) {
                        atomicMin(&best[cu], kr);
                        atomicMin(&best[cv], kr);
                        outgoing = true;
                    }
                }
            }
        }
        if (!generate_any<WAVE>(outgoing, vote, votes, lane, wave)) break;     // one component: the tree is complete
        // hook: a root opens its minimum edge and points across it; of two that picked each other the smaller stays root
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int r = t + j * TPP;
            if (r < RR && comp[r] == r) {
                const uint32_t b = best[r];
                int par = r;
                if (b != GEN_NONE) {
                    const int k = (int)(b & ~GEN_KEY_MASK), u = k >> 1, v = (k & 1) ? u + 1 : u + R;
                    const int cu = comp[u], cv = comp[v];
                    const int other = cu == r ? cv : cu;
                    cells[rcell[u] + ((k & 1) ? 1 : G)] = 'B';
                    par = (best[other] == b && r < other) ? r : other;
                }
                parent[r] = par;
            }
        }
        generate_sync<WAVE>();
        // pointer jumping, in place: a pointer read while another thread moves it is an ancestor either way, and a root's
        // pointer never moves, so "nothing moved" means every component points at its root
        for (int pass = 0; pass < bound; ++pass) {
            bool moved = false;
#pragma unroll
            for (int j = 0; j < RPL; ++j) {
                const int r = t + j * TPP;
                if (r < RR && comp[r] == r) {
                    const int p1 = parent[r], p2 = parent[p1];
                    if (p2 != p1) {
                        parent[r] = p2;
                        moved = true;
                    }
                }
            }
            if (!generate_any<WAVE>(moved, vote, votes, lane, wave)) break;
        }
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int r = t + j * TPP;
            if (r < RR) comp[r] = parent[comp[r]];      // comp[r] was a root, parent[root] is its new root; own entry only
        }
        // the next round's sync (after it resets `best`, which nothing reads here) orders these labels before their readers
    }
    generate_sync<WAVE>();
    if (goal_cell >= 0) {                               // the one thread that drew the goal
        cells[goal_cell] = 'X';
        if (a.goal_xy) a.goal_xy[p] = make_int2(gx, gy);
    }
    generate_sync<WAVE>();

    // write-out: the maze's S bytes cut at the aligned dwords of global memory; nothing outside [first, first + S)
    uint8_t* const out = a.layouts + first;
    const int head = min((4 - mis) & 3, S);
    const int nd = (S - head) >> 2, body = head + 4 * nd;
    uint32_t* const outw = reinterpret_cast<uint32_t*>(out + head);
    const uint32_t* const srcw = cellw + ((mis + head) >> 2);
    for (int w = t; w < nd; w += TPP) outw[w] = srcw[w];
    if (t < head) out[t] = cells[t];
    if (t < S - body) out[body + t] = cells[body + t];
}

GeneratePlan plan_generate(int32_t G, int64_t mazes) {
    const int R = (G - 1) / 2, RR = R * R;
    GeneratePlan p;
    p.wave = G <= 33;
    if (p.wave) p.rooms_per_lane = RR <= 64 ? 1 : (RR <= 128 ? 2 : 4);
    else p.rooms_per_lane = RR <= 256 ? 1 : (RR <= 512 ? 2 : 4);
    p.mazes_per_workgroup = p.wave ? LMAZE_BLOCK / 64 : 1;
    p.grid = (mazes + p.mazes_per_workgroup - 1) / p.mazes_per_workgroup;
    p.lds_bytes = (int64_t)p.mazes_per_workgroup * generate_lds(G).bytes + (p.wave ? 0 : GEN_VOTE_BYTES);
    return p;
}

int describe_generate(const GeneratePlan& p, char* text, int32_t len) {
    if (!text || len < 1) return LMAZE_E_NULL;
    snprintf(text, (size_t)len, "generate_kernel<%s, %d> grid=%lld block=%d lds=%lld mazes_per_workgroup=%d", p.wave ? "wave" : "workgroup",
             p.rooms_per_lane, (long long)p.grid, LMAZE_BLOCK, (long long)p.lds_bytes, p.mazes_per_workgroup);
    return 0;
}

template <bool WAVE, int RPL>
static hipError_t generate_launch(const GenerateArgs& a, const GeneratePlan& p, hipStream_t s) {
    hipLaunchKernelGGL((generate_kernel<WAVE, RPL>), dim3((unsigned)p.grid), dim3(LMAZE_BLOCK), (size_t)p.lds_bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_generate(const GenerateArgs& a, hipStream_t s) {
    if (a.mazes == 0) return hipSuccess;
    const GeneratePlan p = plan_generate(a.grid, a.mazes);
    if (!grid_ok(p.grid)) return hipErrorInvalidConfiguration;
    if (p.wave) {
        switch (p.rooms_per_lane) {
            case 1: return generate_launch<true, 1>(a, p, s);
            case 2: return generate_launch<true, 2>(a, p, s);
            default: return generate_launch<true, 4>(a, p, s);
        }
    }
    switch (p.rooms_per_lane) {
        case 1: return generate_launch<false, 1>(a, p, s);
        case 2: return generate_launch<false, 2>(a, p, s);
        default: return generate_launch<false, 4>(a, p, s);
    }
}

}  // namespace lmaze
