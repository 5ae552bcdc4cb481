// Host build of gym-lmaze_amd/csrc/lmaze_learn.h: the text the kernels compile, run as a stand-alone program on files the
// test writes (tests/test_tabular_cpu.py builds it with -fsanitize=address,undefined -ffp-contract=off and compares what it
// writes with a numpy restatement, bit for bit).
//   learn_host gae IN OUT   IN:  int32 T, int32 n, float gamma, float lambda, float reward[T*n], uint8 done[T*n],
//                                float value[(T+1)*n] (row T: the value behind the last row)
//                           OUT: float adv[T*n], float target[T*n]
//   learn_host q24 IN OUT   IN:  int64 m, float w[m]
//                           OUT: uint8 ok[m], int64 q[m] (0 where not ok)
//   learn_host bin IN OUT   IN:  int64 m, uint32 keys, uint32 actions, int32 key[m], int32 action[m]
//                           OUT: int32 bin[m]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gym-lmaze_amd/csrc/lmaze_learn.h"

template <typename V>
static bool get(FILE* f, V* dst, size_t count) { return count == 0 || fread(dst, sizeof(V), count, f) == count; }
template <typename V>
static bool put(FILE* f, const V* src, size_t count) { return count == 0 || fwrite(src, sizeof(V), count, f) == count; }

static int run_gae(FILE* in, FILE* out) {
    int32_t T, n;
    float gamma, lambda;
    if (!get(in, &T, 1) || !get(in, &n, 1) || !get(in, &gamma, 1) || !get(in, &lambda, 1) || T < 0 || n < 0) return 2;
    const size_t N = (size_t)n, rows = (size_t)T * N;
    std::vector<float> reward(rows), value(rows + N), adv(rows), target(rows);
    std::vector<uint8_t> done(rows);
    if (!get(in, reward.data(), rows) || !get(in, done.data(), rows) || !get(in, value.data(), rows + N)) return 2;
    const float gl = gamma * lambda;
    for (size_t i = 0; i < N; ++i) {
        float a = 0.0f, v_next = value[rows + i];
        for (int32_t t = T - 1; t >= 0; --t) {
            const size_t at = (size_t)t * N + i;
            a = lmaze_gae_step(reward[at], done[at], value[at], v_next, gamma, gl, a);
            adv[at] = a;
            target[at] = lmaze_gae_target(a, value[at]);
            v_next = value[at];
        }
    }
    return put(out, adv.data(), rows) && put(out, target.data(), rows) ? 0 : 3;
}

static int run_q24(FILE* in, FILE* out) {
    int64_t m;
    if (!get(in, &m, 1) || m < 0) return 2;
    std::vector<float> w((size_t)m);
    if (!get(in, w.data(), (size_t)m)) return 2;
    std::vector<uint8_t> ok((size_t)m);
    std::vector<int64_t> q((size_t)m);
    for (size_t j = 0; j < (size_t)m; ++j) {
        ok[j] = lmaze_q24_ok(w[j]) ? 1 : 0;
        q[j] = ok[j] ? lmaze_q24(w[j]) : 0;
    }
    return put(out, ok.data(), (size_t)m) && put(out, q.data(), (size_t)m) ? 0 : 3;
}

static int run_bin(FILE* in, FILE* out) {
    int64_t m;
    uint32_t keys, actions;
    if (!get(in, &m, 1) || !get(in, &keys, 1) || !get(in, &actions, 1) || m < 0) return 2;
    std::vector<int32_t> key((size_t)m), action((size_t)m), bin((size_t)m);
    if (!get(in, key.data(), (size_t)m) || !get(in, action.data(), (size_t)m)) return 2;
    for (size_t j = 0; j < (size_t)m; ++j) bin[j] = lmaze_table_bin(key[j], action[j], keys, actions);
    return put(out, bin.data(), (size_t)m) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: learn_host gae|q24|bin IN OUT\n");
        return 1;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = in ? fopen(argv[3], "wb") : nullptr;
    int rc = 1;
    if (in && out) {
        const std::string mode = argv[1];
        rc = mode == "gae" ? run_gae(in, out) : (mode == "q24" ? run_q24(in, out) : (mode == "bin" ? run_bin(in, out) : 1));
    }
    if (out && fclose(out) != 0) rc = 3;
    if (in) fclose(in);
    return rc;
}
