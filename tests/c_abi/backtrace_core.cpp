// tests/c_abi/backtrace_core.cpp -- kanpyo_amd/csrc/kgpu_backtrace_core.h on the host (tests/test_backtrace_core_cpu.py builds this with g++ and the
// sanitizers and runs it): the two doubling passes as the pool kernel makes them -- four nodes per lane and trip, lanes past the last node clamped onto it, a
// hop from "none" reading entry N -- and the chase over quads, against the plain one-step chase (lattice.rs:144-153), on random predecessor forests: indices
// falling strictly along a chain, roots, dead nodes, N from 1 to 600, every node as a start, path lengths on both sides of the bound C + 1.
// Every array is a heap block of exactly the size the kernel's carve gives it, so a read or a store outside is the sanitizer's to report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "kgpu_backtrace_core.h"

using namespace kgpu;

namespace {

struct Node { uint32_t x, y; };
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the kernel's passes over node[0 .. N]: 64 lanes, four nodes each and trip, a trip's reads before its stores
void double_passes(std::vector<Node> &node, uint32_t N) {
    node[N] = Node{0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t t0 = 0; t0 < N; t0 += 256) {
        uint32_t tc[256], p2[256];
        for (uint32_t l = 0; l < 256; ++l) tc[l] = std::min(t0 + l, N - 1);
        for (uint32_t l = 0; l < 256; ++l) p2[l] = bt_p1(node[bt_hop(bt_p1(node[tc[l]].y), N)].y);
        for (uint32_t l = 0; l < 256; ++l) node[tc[l]].y = bt_p1(node[tc[l]].y) | (p2[l] << 16);   // (a half-word store: the lower half stays)
    }
    for (uint32_t t0 = 0; t0 < N; t0 += 256) {
        uint32_t tc[256], xx[256];
        for (uint32_t l = 0; l < 256; ++l) tc[l] = std::min(t0 + l, N - 1);
        for (uint32_t l = 0; l < 256; ++l) xx[l] = node[bt_hop(bt_p2(node[tc[l]].y), N)].y;
        for (uint32_t l = 0; l < 256; ++l) node[tc[l]].x = xx[l];
    }
}

// the kernel's chase (backtrace_quads, instruction by instruction); path: C + 2 half-words and what lies behind them in the carve, ccat[align_up(C + 2, 4)]
uint32_t chase_quads(const std::vector<Node> &node, uint32_t start, uint32_t C, std::vector<uint16_t> &path, uint32_t &rounds) {
    uint32_t k = 0, pos = start, x, y;
    for (rounds = 1;; ++rounds) {
        x = node[pos].x; y = node[pos].y;
        const uint32_t w0 = bt_quad_word0(pos, y), w1 = bt_quad_word1(x, y);
        path.at(k) = (uint16_t)w0; path.at(k + 1) = (uint16_t)(w0 >> 16); path.at(k + 2) = (uint16_t)w1; path.at(k + 3) = (uint16_t)(w1 >> 16);
        pos = bt_quad_next(x);
        if (pos == BT_NONE) break;
        k += 4;
        if (!(k <= C)) { k -= 4; break; }
    }
    return bt_path_count(k, x, y, C);
}

// lattice.rs:144-153 as the kernel had it before: one predecessor a step, bounded the same way
uint32_t chase_plain(const std::vector<uint16_t> &pre, uint32_t start, uint32_t C, std::vector<uint16_t> &path) {
    uint32_t K = 0, pos = start, pr;
    while ((pr = pre[pos]) != BT_NONE && K <= C) { path[K++] = (uint16_t)pos; pos = pr; }
    return K;
}

}  // namespace

int main() {
    std::mt19937 rng(20240611);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    uint64_t forests = 0, starts = 0, longest = 0, most_rounds = 0, at_bound = 0, past_bound = 0, k_seen[12] = {0};
    std::vector<uint32_t> sizes;
    for (uint32_t n = 1; n <= 40; ++n) sizes.push_back(n);
    for (uint32_t n : {63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, 258u, 300u, 511u, 512u, 513u, 600u}) sizes.push_back(n);
    for (int i = 0; i < 40; ++i) sizes.push_back(1 + below(600));
    for (uint32_t N : sizes)
        for (int shape = 0; shape < 6; ++shape) {
            // shape: how far back a predecessor lies (1: one long chain ... wide: bushy) and how many nodes have none (roots, dead nodes, unreachable ones)
            const uint32_t reach = shape < 2 ? 1u : shape < 4 ? 3u : 40u, none_pct = (shape & 1) ? 25u : shape ? 2u : 0u;
            std::vector<uint16_t> pre(N);
            std::vector<Node> node(N + 1);
            for (uint32_t t = 0; t < N; ++t) {
                pre[t] = (t == 0 || below(100) < none_pct) ? (uint16_t)BT_NONE : (uint16_t)(t - 1 - below(std::min(reach, t)));
                node[t] = Node{(uint32_t)rng(), pre[t] | ((uint32_t)rng() << 16)};   // what stage B leaves behind: x and the upper half of y are anything
            }
            node[N] = Node{0u, 0u};
            double_passes(node, N);
            ++forests;
            for (uint32_t t = 0; t < N; ++t) {
                // the quad of t is its four nearest ancestors, BT_NONE from the chain's end on
                uint32_t a[4], p = t;
                for (int j = 0; j < 4; ++j) { p = p == BT_NONE ? BT_NONE : pre[p]; a[j] = p; }
                CHECK(bt_p1(node[t].y) == a[0] && bt_p2(node[t].y) == a[1] && (node[t].x & 0xFFFFu) == a[2] && (node[t].x >> 16) == a[3],
                      "N %u node %u: quad %08x %08x, ancestors %x %x %x %x", N, t, node[t].y, node[t].x, a[0], a[1], a[2], a[3]);
                // the chain's length from t, then C on both sides of it
                uint32_t len = 0;
                for (uint32_t q = t; pre[q] != BT_NONE; q = pre[q]) ++len;
                longest = std::max<uint64_t>(longest, len);
                if (len < 12) ++k_seen[len];
                for (uint32_t C : {len ? len - 1 : 0u, len, len + 1 + below(7), len > 2 ? below(len - 1) : 0u}) {
                    const uint32_t cap = (C + 2) + ((C + 2 + 3) & ~3u) / 2;   // path[C + 2], then ccat[align_up(C + 2, 4)] bytes
                    CHECK(2 * (C + 2) + bt_path_overrun_bytes(C) <= 2 * cap, "C %u: overrun beyond ccat", C);
                    std::vector<uint16_t> got(C + 2 + bt_path_overrun_bytes(C) / 2, 0xABCD), want(C + 2, 0xABCD);
                    uint32_t rounds = 0;
                    const uint32_t K = chase_quads(node, t, C, got, rounds), Kw = chase_plain(pre, t, C, want);
                    CHECK(K == Kw && std::equal(want.begin(), want.begin() + Kw, got.begin()), "N %u start %u C %u: K %u, plain chase %u (or the path differs)", N, t, C, K, Kw);
                    CHECK(K <= C + 1 && rounds <= C / 4 + 1, "N %u start %u C %u: K %u after %u rounds", N, t, C, K, rounds);
                    most_rounds = std::max<uint64_t>(most_rounds, rounds);
                    at_bound += K == C + 1 && len == C + 1;
                    past_bound += len > C + 1;
                    ++starts;
                }
            }
        }
    // the generator reached what it is there for
    for (int k = 0; k < 12; ++k) CHECK(k_seen[k] > 0, "no chain of length %d", k);
    CHECK(longest >= 500 && most_rounds >= 126 && at_bound > 1000 && past_bound > 1000, "longest %llu rounds %llu at the bound %llu past it %llu",
          (unsigned long long)longest, (unsigned long long)most_rounds, (unsigned long long)at_bound, (unsigned long long)past_bound);
    if (fails) { std::printf("%d FAILED\n", fails); return 1; }
    std::printf("ok %llu forests, %llu chases, longest chain %llu, most rounds %llu, %llu at the bound, %llu past it\n", (unsigned long long)forests,
                (unsigned long long)starts, (unsigned long long)longest, (unsigned long long)most_rounds, (unsigned long long)at_bound, (unsigned long long)past_bound);
    return 0;
}
