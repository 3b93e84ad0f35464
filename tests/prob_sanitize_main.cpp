// tests/prob_sanitize_main.cpp -- a stand-alone program over kanpyo_amd/csrc/kgpu_prob_host.cpp (tests/test_prob_cpu.py builds the two with
// -fsanitize=address,undefined and runs the result): both host functions over a crafted lattice of three characters, at exact capacities, one short,
// and on lattices that contradict themselves.  It prints "prob sanitize ok" when every answer is the expected one.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kanpyo_gpu.h"

namespace kgpu { void set_error(const char *, ...) {} }   // (the host file reports through its caller's)

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    // "abc": a ab b bc c between BOS and EOS, numbered by start position; three context ids
    const struct { uint32_t s, e; int16_t l, r, c; } W[] = {{0, 0, 0, 0, 0}, {0, 1, 1, 2, 100}, {0, 2, 2, 1, 0}, {1, 2, 0, 1, 300}, {1, 3, 1, 1, 100}, {2, 3, 2, 0, 0}, {3, 3, 0, 0, 0}};
    const uint64_t N = 7;
    std::vector<kgpu_lattice_node> nodes(N);
    for (uint64_t t = 0; t < N; ++t) {
        kgpu_lattice_node &n = nodes[t];
        std::memset(&n, 0, sizeof n);
        n.id = t == 0 || t == N - 1 ? 0 : (int32_t)t; n.cls = t == 0 || t == N - 1 ? KGPU_CLASS_DUMMY : KGPU_CLASS_KNOWN;
        n.byte_pos = W[t].s; n.char_pos = W[t].s; n.end_char = W[t].e; n.byte_len = W[t].e - W[t].s;
        n.left_id = W[t].l; n.right_id = W[t].r; n.cost = W[t].c; n.dp = 1 << 30; n.pre = -1;
    }
    std::vector<uint32_t> eo = {0, 1, 2, 4, 6, 7}, en = {0, 1, 2, 3, 4, 5, 6};
    const int16_t conn[9] = {0, 100, -100, 50, 0, 100, -100, 0, 25};   // element (right, left) at left * 3 + right
    nodes[0].dp = 0;
    for (uint64_t t = 1; t < N; ++t)   // the Viterbi state a dump carries
        for (uint32_t e = eo[nodes[t].char_pos]; e < eo[nodes[t].char_pos + 1]; ++e) {
            const uint32_t j = en[e];
            const int32_t v = nodes[j].dp + conn[3 * nodes[t].left_id + nodes[j].right_id] + nodes[t].cost;
            if (nodes[j].dp < (1 << 30) && v < nodes[t].dp) { nodes[t].dp = v; nodes[t].pre = (int32_t)j; }
        }
    kgpu_lattice lat{N, 5, nodes.data(), eo.data(), en.data()};
    const double theta = 0.01;

    double lz = 0, bl = 0;
    uint64_t T = 0;
    EXPECT(kgpu_marginals_host(&lat, conn, 3, 3, theta, KGPU_MARGINAL_ALL, 0.0, nullptr, 0, nullptr, nullptr, &lz, &bl, &T) == KGPU_ERR_CAPACITY);
    EXPECT(T == 6 && std::isfinite(lz) && bl <= 0);
    {
        std::vector<kgpu_token> tok(T);   // exact fits: the sanitizer watches the ends
        std::vector<double> pr(T);
        std::vector<uint8_t> ob(T);
        EXPECT(kgpu_marginals_host(&lat, conn, 3, 3, theta, KGPU_MARGINAL_ALL, 0.0, tok.data(), T, pr.data(), ob.data(), &lz, &bl, &T) == KGPU_OK);
        EXPECT(T == 6 && pr[5] == 1.0 && ob[5] == 1);
        EXPECT(std::fabs(pr[0] + pr[1] - 1.0) < 1e-12 && std::fabs(pr[4] + pr[3] - 1.0) < 1e-12);   // the nodes over the first and over the last character
        uint64_t Tb = 0;
        EXPECT(kgpu_marginals_host(&lat, conn, 3, 3, theta, KGPU_MARGINAL_BEST, 0.0, tok.data(), 1, pr.data(), ob.data(), &lz, &bl, &Tb) == KGPU_ERR_CAPACITY);
        std::vector<kgpu_token> tb(Tb);
        EXPECT(kgpu_marginals_host(&lat, conn, 3, 3, theta, KGPU_MARGINAL_BEST, 0.0, tb.data(), Tb, pr.data(), ob.data(), &lz, &bl, &Tb) == KGPU_OK);
        EXPECT(Tb >= 2 && Tb <= 4 && tb[Tb - 1].cls == KGPU_CLASS_DUMMY);
    }
    for (uint32_t ns : {1u, 3u, 256u}) {
        uint64_t P = 0, TT = 0;
        uint64_t one = 0;
        EXPECT(kgpu_samples_host(&lat, conn, 3, 3, theta, ns, 7, 2, nullptr, 0, &one, nullptr, 0, &P, &TT) == KGPU_ERR_CAPACITY);
        EXPECT(P == ns && TT >= 3 * (uint64_t)ns);
        std::vector<kgpu_token> tok(TT);
        std::vector<uint64_t> toff(P + 1);
        std::vector<int32_t> costs(P);
        EXPECT(kgpu_samples_host(&lat, conn, 3, 3, theta, ns, 7, 2, tok.data(), TT, toff.data(), costs.data(), P, &P, &TT) == KGPU_OK);
        EXPECT(toff[P] == TT && tok[TT - 1].cls == KGPU_CLASS_DUMMY);
    }
    {   // lattices that contradict themselves are refused before anything is indexed with them
        uint64_t P = 0, TT = 0, toff[4];
        auto rc = [&]() { return kgpu_samples_host(&lat, conn, 3, 3, theta, 1, 0, 0, nullptr, 0, toff, nullptr, 0, &P, &TT); };
        en[3] = 99; EXPECT(rc() == KGPU_ERR_INVALID_ARG); en[3] = 3;
        nodes[3].left_id = 3; EXPECT(rc() == KGPU_ERR_INVALID_ARG); nodes[3].left_id = 0;
        nodes[3].char_pos = 77; EXPECT(rc() == KGPU_ERR_INVALID_ARG); nodes[3].char_pos = 1;
        nodes[2].end_char = 9; EXPECT(rc() == KGPU_ERR_INVALID_ARG); nodes[2].end_char = 2;
        nodes[5].pre = 6; EXPECT(kgpu_marginals_host(&lat, conn, 3, 3, theta, 0, 0.0, nullptr, 0, nullptr, nullptr, &lz, &bl, &T) == KGPU_ERR_INVALID_ARG); nodes[5].pre = 3;
        eo[5] = 9; EXPECT(rc() == KGPU_ERR_INVALID_ARG); eo[5] = 7;
        EXPECT(kgpu_samples_host(&lat, conn, 3, 3, 0.0, 1, 0, 0, nullptr, 0, toff, nullptr, 0, &P, &TT) == KGPU_ERR_INVALID_ARG);
        EXPECT(rc() == KGPU_ERR_CAPACITY);
    }
    if (!fails) std::printf("prob sanitize ok\n");
    return fails ? 1 : 0;
}
