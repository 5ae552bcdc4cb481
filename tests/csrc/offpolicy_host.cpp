// Host build of gym-lmaze_amd/csrc/lmaze_offpolicy.h: the text the kernels compile, run as a stand-alone program on files the
// test writes (tests/test_offpolicy_cpu.py builds it with -fsanitize=address,undefined -ffp-contract=off and compares what it
// writes with a numpy restatement, bit for bit).
//   offpolicy_host weights IN OUT   IN:  int64 m, int64 keys, int32 form, uint32 epsilon_u32, the table (form 1: uint8[keys],
//                                        else 16 bytes per key), int32 key[m], int32 action[m]
//                                   OUT: uint64 w[m], float p[m]
//   offpolicy_host ratio IN OUT     IN:  int64 m, uint64 w_target[m], uint64 w_behaviour[m]
//                                   OUT: float ratio[m]
//   offpolicy_host vtrace IN OUT    IN:  int32 T, int32 n, float gamma, lambda, rho_bar, c_bar, float reward[T*n], uint8 done[T*n],
//                                        float value[(T+1)*n] (row T: the value behind the last row), float ratio[T*n]
//                                   OUT: float vs[T*n], float pg[T*n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gym-lmaze_amd/csrc/lmaze_offpolicy.h"

template <typename V>
static bool get(FILE* f, V* dst, size_t count) { return count == 0 || fread(dst, sizeof(V), count, f) == count; }
template <typename V>
static bool put(FILE* f, const V* src, size_t count) { return count == 0 || fwrite(src, sizeof(V), count, f) == count; }

static int run_weights(FILE* in, FILE* out) {
    int64_t m, keys;
    int32_t form;
    uint32_t eps;
    if (!get(in, &m, 1) || !get(in, &keys, 1) || !get(in, &form, 1) || !get(in, &eps, 1) || m < 0 || keys < 1 || keys > (1 << 24) ||
        form < 0 || form > 2)
        return 2;
    const size_t M = (size_t)m, K = (size_t)keys;
    std::vector<uint8_t> bytes(form == LMAZE_LAW_POLICY ? K : 0);
    std::vector<uint32_t> rows(form == LMAZE_LAW_POLICY ? 0 : 4 * K);
    std::vector<int32_t> key(M), action(M);
    if (!get(in, bytes.data(), bytes.size()) || !get(in, rows.data(), rows.size()) || !get(in, key.data(), M) || !get(in, action.data(), M))
        return 2;
    std::vector<uint64_t> w(M);
    std::vector<float> p(M);
    for (size_t j = 0; j < M; ++j) {
        const size_t at = lmaze_law_row(key[j], (uint32_t)keys);
        uint32_t r[4] = {0, 0, 0, 0};
        if (form == LMAZE_LAW_POLICY) r[0] = bytes[at];
        else memcpy(r, &rows[4 * at], 16);
        w[j] = lmaze_keyed_weight(key[j], (uint32_t)keys, lmaze_action_weight(form, r[0], r[1], r[2], r[3], eps, action[j]));
        p[j] = lmaze_weight_prob(w[j]);
    }
    return put(out, w.data(), M) && put(out, p.data(), M) ? 0 : 3;
}

static int run_ratio(FILE* in, FILE* out) {
    int64_t m;
    if (!get(in, &m, 1) || m < 0) return 2;
    const size_t M = (size_t)m;
    std::vector<uint64_t> wt(M), wb(M);
    if (!get(in, wt.data(), M) || !get(in, wb.data(), M)) return 2;
    std::vector<float> ratio(M);
    for (size_t j = 0; j < M; ++j) ratio[j] = lmaze_weight_ratio(wt[j], wb[j]);
    return put(out, ratio.data(), M) ? 0 : 3;
}

static int run_vtrace(FILE* in, FILE* out) {
    int32_t T, n;
    float s[4];                       // gamma, lambda, rho_bar, c_bar
    if (!get(in, &T, 1) || !get(in, &n, 1) || !get(in, s, 4) || T < 0 || n < 0) return 2;
    const size_t N = (size_t)n, rows = (size_t)T * N;
    std::vector<float> reward(rows), value(rows + N), ratio(rows), vs(rows), pg(rows);
    std::vector<uint8_t> done(rows);
    if (!get(in, reward.data(), rows) || !get(in, done.data(), rows) || !get(in, value.data(), rows + N) || !get(in, ratio.data(), rows))
        return 2;
    for (size_t i = 0; i < N; ++i) {
        LmazeVtraceCarry carry = {value[rows + i], value[rows + i], 0.0f};
        for (int32_t t = T - 1; t >= 0; --t) {
            const size_t at = (size_t)t * N + i;
            lmaze_vtrace_step(reward[at], done[at], value[at], ratio[at], s[0], s[1], s[2], s[3], &carry, &vs[at], &pg[at]);
        }
    }
    return put(out, vs.data(), rows) && put(out, pg.data(), rows) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: offpolicy_host weights|ratio|vtrace IN OUT\n");
        return 1;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = in ? fopen(argv[3], "wb") : nullptr;
    int rc = 1;
    if (in && out) {
        const std::string mode = argv[1];
        rc = mode == "weights" ? run_weights(in, out) : (mode == "ratio" ? run_ratio(in, out) : (mode == "vtrace" ? run_vtrace(in, out) : 1));
    }
    if (out && fclose(out) != 0) rc = 3;
    if (in) fclose(in);
    return rc;
}
