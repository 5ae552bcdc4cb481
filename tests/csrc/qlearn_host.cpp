// Host build of the Q-learning arithmetic of gym-lmaze_amd/csrc/lmaze_learn.h: the text the rollout kernels compile, run as a
// stand-alone program on files the test writes (tests/test_qlearn_cpu.py builds it with -fsanitize=address,undefined
// -ffp-contract=off and compares what it writes with the numpy restatement of tests/qlearn_ref.py, bit for bit).
//   qlearn_host max IN OUT      IN:  int64 m, float q[m*4]
//                               OUT: float best[m], int32 action[m]
//   qlearn_host update IN OUT   IN:  int64 m, float alpha, float gamma, float q_sa[m], float r[m], uint8 done[m], float v_next[m]
//                               OUT: float target[m], float delta[m], float q_new[m]
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../gym-lmaze_amd/csrc/lmaze_learn.h"

template <typename V>
static bool get(FILE* f, V* dst, size_t count) { return count == 0 || fread(dst, sizeof(V), count, f) == count; }
template <typename V>
static bool put(FILE* f, const V* src, size_t count) { return count == 0 || fwrite(src, sizeof(V), count, f) == count; }

static int run_max(FILE* in, FILE* out) {
    int64_t m;
    if (!get(in, &m, 1) || m < 0) return 2;
    const size_t M = (size_t)m;
    std::vector<float> q(M * 4), best(M);
    std::vector<int32_t> action(M);
    if (!get(in, q.data(), M * 4)) return 2;
    for (size_t j = 0; j < M; ++j) {
        int a = -1;
        best[j] = lmaze_q_first_max(&q[j * 4], &a);
        action[j] = a;
    }
    return put(out, best.data(), M) && put(out, action.data(), M) ? 0 : 3;
}

static int run_update(FILE* in, FILE* out) {
    int64_t m;
    float alpha, gamma;
    if (!get(in, &m, 1) || !get(in, &alpha, 1) || !get(in, &gamma, 1) || m < 0) return 2;
    const size_t M = (size_t)m;
    std::vector<float> q_sa(M), r(M), v_next(M), target(M), delta(M), q_new(M);
    std::vector<uint8_t> done(M);
    if (!get(in, q_sa.data(), M) || !get(in, r.data(), M) || !get(in, done.data(), M) || !get(in, v_next.data(), M)) return 2;
    for (size_t j = 0; j < M; ++j) {
        target[j] = lmaze_q_target(r[j], done[j], gamma, v_next[j]);
        q_new[j] = lmaze_q_update(q_sa[j], alpha, target[j], &delta[j]);
    }
    return put(out, target.data(), M) && put(out, delta.data(), M) && put(out, q_new.data(), M) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: qlearn_host max|update IN OUT\n");
        return 1;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = in ? fopen(argv[3], "wb") : nullptr;
    int rc = 1;
    if (in && out) {
        const std::string mode = argv[1];
        rc = mode == "max" ? run_max(in, out) : (mode == "update" ? run_update(in, out) : 1);
    }
    if (out && fclose(out) != 0) rc = 3;
    if (in) fclose(in);
    return rc;
}
