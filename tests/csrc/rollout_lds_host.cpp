// Host build of gym-lmaze_amd/csrc/lmaze_rollout_lds.h: the text from which the rollout kernels take their LDS pointers and
// rollout_plan the bytes a launch requests, run as a stand-alone program (tests/test_rollout_lds_cpu.py builds it with
// -fsanitize=address,undefined).  For every body, G, envs per workgroup and table kind it allocates exactly `total` bytes
// and writes the whole extent of every array the body indexes, through a pointer of the array's own element type at the
// header's offset: an overrun or a misaligned array is the sanitizers' to report.  One line per case on stdout:
//   <body> <G> <epb> <kind> <total> then "<array> <offset> <bytes>" for every array written
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../gym-lmaze_amd/csrc/lmaze_rollout_lds.h"

struct alignas(16) Row { uint32_t w[4]; };      // one key's staged thresholds: a 16-byte LDS access

template <typename V>
static void put(V& v, size_t i) { v = (V)i; }
static void put(Row& v, size_t i) { v = Row{{(uint32_t)i, 1, 2, 3}}; }
template <typename V>
static uint64_t get(const V& v) { return (uint64_t)v; }
static uint64_t get(const Row& v) { return (uint64_t)v.w[0] + v.w[3]; }

static uint64_t g_read_back;                    // printed at the end: no store below is dead

template <typename V>
static void fill(char* base, const char* name, int offset, size_t count) {
    V* p = reinterpret_cast<V*>(base + offset);
    for (size_t i = 0; i < count; ++i) put(p[i], i);
    for (size_t i = 0; i < count; ++i) g_read_back += get(p[i]);
    printf(" %s %d %zu", name, offset, count * sizeof(V));
}

static void table(char* base, const LmazeRolloutLds& l, int cells, int kind) {
    if (kind == LMAZE_TAB_BYTES) fill<uint8_t>(base, "tab", l.tab, (size_t)cells);
    if (kind == LMAZE_TAB_ROWS) fill<Row>(base, "tab", l.tab, (size_t)cells);
}

int main() {
    const int kinds[] = {LMAZE_TAB_NONE, LMAZE_TAB_BYTES, LMAZE_TAB_ROWS, LMAZE_TAB_GLOBAL};
    for (int G = 3; G <= 64; ++G) {
        const int cells = G * G;
        for (int kind : kinds) {
            for (int epb = 4; epb <= 256; epb <<= 1) {               // rollout_shared_kernel: launch_hint asks for up to 256
                const LmazeRolloutLds l = lmaze_rollout_lds_shared(cells, epb, kind);
                char* base = static_cast<char*>(malloc((size_t)l.total));
                printf("shared %d %d %d %d", G, epb, kind, l.total);
                fill<int>(base, "pat", l.pat, (size_t)cells);
                fill<int>(base, "ballflat", l.ballflat, (size_t)epb);
                fill<int>(base, "goalflat", l.goalflat, (size_t)epb);
                fill<uint8_t>(base, "lay", l.lay, (size_t)cells);
                fill<uint16_t>(base, "spawn", l.spawn, (size_t)cells);
                table(base, l, cells, kind);
                printf("\n");
                free(base);
            }
            for (int epb = 4; epb <= 64; epb <<= 1) {                // rollout_perenv_kernel: every env's lane sits in wave 0
                const LmazeRolloutLds l = lmaze_rollout_lds_perenv(cells, epb, kind);
                char* base = static_cast<char*>(malloc((size_t)l.total));
                printf("perenv %d %d %d %d", G, epb, kind, l.total);
                fill<int>(base, "ballflat", l.ballflat, (size_t)epb);
                fill<int>(base, "goalflat", l.goalflat, (size_t)epb);
                fill<uint32_t>(base, "lay", l.lay, ((size_t)epb * cells) >> 2);   // the dword copy: epb is a multiple of 4
                fill<uint8_t>(base, "lay", l.lay, (size_t)epb * cells);
                table(base, l, cells, kind);
                printf("\n");
                free(base);
            }
            for (int epb = 16; epb <= 256 && G >= 4; epb <<= 1) {    // rollout_shared_u8_kernel
                const LmazeRolloutLds l = lmaze_rollout_lds_u8(cells, epb, kind);
                char* base = static_cast<char*>(malloc((size_t)l.total));
                printf("u8 %d %d %d %d", G, epb, kind, l.total);
                fill<uint32_t>(base, "pat", l.pat, (size_t)4 * lmaze_rollout_u8_pw(cells));
                fill<int>(base, "ballflat", l.ballflat, (size_t)epb + 1);
                fill<int>(base, "goalflat", l.goalflat, (size_t)epb + 1);
                fill<uint16_t>(base, "spawn", l.spawn, (size_t)cells);
                fill<uint8_t>(base, "lay", l.lay, (size_t)cells);
                table(base, l, cells, kind);
                printf("\n");
                free(base);
            }
        }
    }
    printf("read_back %llu\n", (unsigned long long)g_read_back);
    return 0;
}
