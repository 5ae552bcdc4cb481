// Host build of gym-lmaze_amd/csrc/lmaze_foveal_select.h: the text the closed-loop foveal rollout compiles, run as a
// stand-alone program on files the test writes (tests/test_foveal_rollout_policy_cpu.py builds it with
// -fsanitize=address,undefined and compares what it writes with a numpy restatement).
//   foveal_select_host IN OUT
//     IN:  int64 m, int32 G, int32 L, int32 A, uint32 epsilon, uint8 table[L*G*G],
//          int32 lid[m], int32 bx[m], int32 by[m], uint32 rx[m], uint32 ry[m]
//     OUT: int32 key[m], int32 action[m] (table[key] mixed with the draw), int32 uniform[m] (the explored action alone)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../gym-lmaze_amd/csrc/lmaze_foveal_select.h"

template <typename V>
static bool get(FILE* f, V* dst, size_t count) { return count == 0 || fread(dst, sizeof(V), count, f) == count; }
template <typename V>
static bool put(FILE* f, const V* src, size_t count) { return count == 0 || fwrite(src, sizeof(V), count, f) == count; }

static int run(FILE* in, FILE* out) {
    int64_t m;
    int32_t G, L, A;
    uint32_t eps;
    if (!get(in, &m, 1) || !get(in, &G, 1) || !get(in, &L, 1) || !get(in, &A, 1) || !get(in, &eps, 1)) return 2;
    if (m < 0 || G < 1 || L < 1 || A < 1) return 2;
    const size_t M = (size_t)m;
    std::vector<uint8_t> table((size_t)L * G * G);       // exactly the table: a key outside it is the sanitizer's to report
    std::vector<int32_t> lid(M), bx(M), by(M), key(M), action(M), uniform(M);
    std::vector<uint32_t> rx(M), ry(M);
    if (!get(in, table.data(), table.size()) || !get(in, lid.data(), M) || !get(in, bx.data(), M) || !get(in, by.data(), M) ||
        !get(in, rx.data(), M) || !get(in, ry.data(), M))
        return 2;
    for (size_t j = 0; j < M; ++j) {
        key[j] = lmaze_foveal_key(lid[j], bx[j], by[j], G, L);
        action[j] = lmaze_foveal_choose(table[(size_t)key[j]], rx[j], ry[j], eps, A);
        uniform[j] = lmaze_foveal_explore(ry[j], A);
    }
    return put(out, key.data(), M) && put(out, action.data(), M) && put(out, uniform.data(), M) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: foveal_select_host IN OUT\n");
        return 1;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    int rc = 1;
    if (in && out) rc = run(in, out);
    if (out && fclose(out) != 0) rc = 3;
    if (in) fclose(in);
    return rc;
}
