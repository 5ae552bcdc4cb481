// Host build of gym-lmaze_amd/csrc/lmaze_rollout_lds.h for the table kind of the rollouts with a table per env,
// LMAZE_TAB_ENV_BYTES (body 3, rollout_perenv_kernel: the workgroup's byte tables staged behind its layouts), run as a
// stand-alone program (tests/test_env_rollout_cpu.py builds it with -fsanitize=address,undefined).  For G = 3..64 and every
// envs per workgroup of the body it allocates exactly `total` bytes and writes the whole extent of every array the body
// indexes -- the layouts and the tables both by the dword copy and by bytes -- through a pointer of the array's own element
// type at the header's offset: an overrun or a misaligned array is the sanitizers' to report.  One line per case on stdout:
//   perenv <G> <epb> <kind> <total> then "<array> <offset> <bytes>" for every array written
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../gym-lmaze_amd/csrc/lmaze_rollout_lds.h"

static uint64_t g_read_back;                    // printed at the end: no store below is dead

template <typename V>
static void fill(char* base, const char* name, int offset, size_t count) {
    V* p = reinterpret_cast<V*>(base + offset);
    for (size_t i = 0; i < count; ++i) p[i] = (V)i;
    for (size_t i = 0; i < count; ++i) g_read_back += (uint64_t)p[i];
    printf(" %s %d %zu", name, offset, count * sizeof(V));
}

int main() {
    for (int G = 3; G <= 64; ++G) {
        const int cells = G * G;
        for (int epb = 4; epb <= 64; epb <<= 1) {
            const LmazeRolloutLds l = lmaze_rollout_lds_perenv(cells, epb, LMAZE_TAB_ENV_BYTES);
            char* base = static_cast<char*>(malloc((size_t)l.total));
            printf("perenv %d %d %d %d", G, epb, (int)LMAZE_TAB_ENV_BYTES, l.total);
            fill<int>(base, "ballflat", l.ballflat, (size_t)epb);
            fill<int>(base, "goalflat", l.goalflat, (size_t)epb);
            fill<uint32_t>(base, "lay", l.lay, ((size_t)epb * cells) >> 2);   // the dword copy: epb is a multiple of 4
            fill<uint8_t>(base, "lay", l.lay, (size_t)epb * cells);
            fill<uint32_t>(base, "tab", l.tab, ((size_t)epb * cells) >> 2);   // the same copy, for the tables
            fill<uint8_t>(base, "tab", l.tab, (size_t)epb * cells);
            printf("\n");
            free(base);
        }
    }
    printf("read_back %llu\n", (unsigned long long)g_read_back);
    return 0;
}
