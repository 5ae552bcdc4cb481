// Host build of gym-lmaze_amd/csrc/lmaze_foveal_sample.h: the text the sampling closed-loop foveal rollout compiles, run as
// a stand-alone program on files the test writes (tests/test_foveal_rollout_sample_cpu.py builds it with
// -fsanitize=address,undefined and compares what it writes with a numpy restatement).
//   foveal_sample_host IN OUT
//     IN:  int64 m, int32 A, uint32 rows[m * W] (W = lmaze_foveal_sample_row_words(A)), uint32 r[m]
//     OUT: int32 W, int32 action[m]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../gym-lmaze_amd/csrc/lmaze_foveal_sample.h"

template <typename V>
static bool get(FILE* f, V* dst, size_t count) { return count == 0 || fread(dst, sizeof(V), count, f) == count; }
template <typename V>
static bool put(FILE* f, const V* src, size_t count) { return count == 0 || fwrite(src, sizeof(V), count, f) == count; }

static int run(FILE* in, FILE* out) {
    int64_t m;
    int32_t A;
    if (!get(in, &m, 1) || !get(in, &A, 1)) return 2;
    if (m < 0 || A < 2) return 2;
    const size_t M = (size_t)m;
    const int32_t W = lmaze_foveal_sample_row_words(A);
    std::vector<uint32_t> r(M);
    std::vector<int32_t> action(M);
    if (!get(in, r.data(), 0)) return 2;
    // every row in an allocation of its own, exactly W words: a word read past a row is the sanitizer's to report
    std::vector<std::vector<uint32_t>> rows(M, std::vector<uint32_t>((size_t)W));
    for (size_t j = 0; j < M; ++j)
        if (!get(in, rows[j].data(), (size_t)W)) return 2;
    if (!get(in, r.data(), M)) return 2;
    for (size_t j = 0; j < M; ++j) action[j] = lmaze_foveal_sample_action(rows[j].data(), A - 1, r[j]);
    return put(out, &W, 1) && put(out, action.data(), M) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: foveal_sample_host IN OUT\n");
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
