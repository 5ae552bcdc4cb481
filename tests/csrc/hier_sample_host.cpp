// Host build of gym-lmaze_amd/csrc/lmaze_hier_sample.h: the text the sampling closed-loop two-level rollout of v5/v6 compiles,
// run as a stand-alone program on files the test writes (tests/test_hier_rollout_sample_cpu.py builds it with
// -fsanitize=address,undefined and compares what it writes with a numpy restatement).
//   hier_sample_host IN OUT
//     IN:  int64 m, int32 G, int32 L, int32 controller_key,
//          uint32 controller[100 or 100*L*G*G][4], uint32 planner[L*G*G][24],
//          int32 lid[m], bx[m], by[m], fgx[m], fgy[m], uint32 rx[m], rz[m]
//     OUT: int32 planner_key[m], controller_key[m], goal[m] (the planner key's row against rz),
//          action[m] (the controller key's row against rx)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../gym-lmaze_amd/csrc/lmaze_hier_sample.h"

template <typename V>
static bool get(FILE* f, V* dst, size_t count) { return count == 0 || fread(dst, sizeof(V), count, f) == count; }
template <typename V>
static bool put(FILE* f, const V* src, size_t count) { return count == 0 || fwrite(src, sizeof(V), count, f) == count; }

static int run(FILE* in, FILE* out) {
    int64_t m;
    int32_t G, L, ck;
    if (!get(in, &m, 1) || !get(in, &G, 1) || !get(in, &L, 1) || !get(in, &ck, 1)) return 2;
    if (m < 0 || G < 1 || L < 1 || (ck != 0 && ck != 1)) return 2;
    const size_t M = (size_t)m, cells = (size_t)L * G * G;
    // exactly the tables: a key outside them, or a fourth compare of a controller row's last key, is the sanitizer's to report
    std::vector<uint32_t> controller((size_t)lmaze_hier_sample_controller_keys(ck, L, G) * LMAZE_HIER_SAMPLE_CROW - 1);
    std::vector<uint32_t> planner(cells * LMAZE_HIER_SAMPLE_PROW);
    std::vector<int32_t> lid(M), bx(M), by(M), fgx(M), fgy(M), kp(M), kc(M), goal(M), action(M);
    std::vector<uint32_t> rx(M), rz(M);
    uint32_t reserved;
    if (!get(in, controller.data(), controller.size()) || !get(in, &reserved, 1) || !get(in, planner.data(), planner.size()) ||
        !get(in, lid.data(), M) || !get(in, bx.data(), M) || !get(in, by.data(), M) || !get(in, fgx.data(), M) ||
        !get(in, fgy.data(), M) || !get(in, rx.data(), M) || !get(in, rz.data(), M))
        return 2;
    for (size_t j = 0; j < M; ++j) {
        kp[j] = lmaze_hier_planner_key(lid[j], bx[j], by[j], G, L);
        kc[j] = lmaze_hier_controller_key(ck, kp[j], lmaze_hier_offset(fgx[j], fgy[j], bx[j], by[j]));
        goal[j] = lmaze_hier_sample_goal(planner.data() + (size_t)kp[j] * LMAZE_HIER_SAMPLE_PROW, rz[j]);
        action[j] = lmaze_hier_sample_action(controller.data() + (size_t)kc[j] * LMAZE_HIER_SAMPLE_CROW, rx[j]);
    }
    return put(out, kp.data(), M) && put(out, kc.data(), M) && put(out, goal.data(), M) && put(out, action.data(), M) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hier_sample_host IN OUT\n");
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
