// tests/c_abi/mode_sanitize.cpp -- kgpu_mode_host (kanpyo_amd/csrc/kgpu_mode_host.cpp) under -fsanitize=address,undefined: a stand-alone program
// with its own main, linked with that file alone.  It runs the host function over a crafted lattice; every buffer is a heap block of its exact size, so
// that a read or a write one element beyond any of them is reported.  Built and run by tests/test_mode_cpu.py.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "kanpyo_gpu.h"

namespace kgpu { void set_error(const char *, ...) {} }   // (the host file reports through its caller's)

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a heap block of exactly v.size() elements (none for an empty one)
    std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

int fails = 0;
void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++fails; }
}

kgpu_lattice_node node(int32_t id, uint32_t cls, uint32_t bpos, uint32_t cpos, uint32_t cend, uint32_t blen, int16_t l, int16_t r, int16_t cost) {
    kgpu_lattice_node n{};
    n.id = id; n.cls = cls; n.byte_pos = bpos; n.char_pos = cpos; n.end_char = cend; n.byte_len = blen; n.left_id = l; n.right_id = r; n.cost = cost;
    return n;
}

}  // namespace

int main() {
    // "関西空a": three kanji words over the first four characters (the whole, and its halves), then an unknown word of two characters ("空a" is
    // not a word: the unknown node covers 空 and a), the four-byte U+20000 is not in it -- the text ends with the last node's last byte
    const char *text = "\xE9\x96\xA2\xE8\xA5\xBF\xE7\xA9\xBA\xE6\xB8\xAF\xF0\xA0\x80\x80" "a";   // 関 西 空 港 U+20000 a
    const uint64_t len = std::strlen(text);
    std::vector<uint8_t> bytes(text, text + len);
    std::vector<kgpu_lattice_node> nodes = {
        node(0, KGPU_CLASS_DUMMY, 0, 0, 0, 0, 0, 0, 0),
        node(1, KGPU_CLASS_KNOWN, 0, 0, 4, 12, 0, 1, 1000),    // 関西空港
        node(2, KGPU_CLASS_KNOWN, 0, 0, 2, 6, 1, 0, 700),      // 関西
        node(3, KGPU_CLASS_KNOWN, 6, 2, 4, 6, 0, 0, 700),      // 空港
        node(1, KGPU_CLASS_UNKNOWN, 12, 4, 6, 5, 1, 1, 2000),  // U+20000 a
        node(0, KGPU_CLASS_DUMMY, 17, 6, 6, 0, 0, 0, 0),
    };
    // edges[e]: the nodes ending at e; 8 positions (6 characters + 2)
    std::vector<uint32_t> eoff = {0, 1, 1, 2, 2, 4, 4, 5, 6};
    std::vector<uint32_t> enodes = {0, 2, 1, 3, 4, 5};
    std::vector<int16_t> conn = {0, 5, -3, 9};
    auto p_bytes = exact(bytes);
    auto p_nodes = exact(nodes);
    auto p_eoff = exact(eoff);
    auto p_enodes = exact(enodes);
    auto p_conn = exact(conn);
    kgpu_lattice lat{nodes.size(), 8, p_nodes.get(), p_eoff.get(), p_enodes.get()};

    struct Want { uint32_t mode; uint64_t tokens; };
    const Want wants[] = {{KGPU_MODE_NORMAL, 3}, {KGPU_MODE_SEARCH, 4}, {KGPU_MODE_EXTENDED, 5}};
    for (const Want &w : wants) {
        kgpu_mode_opts opts = KGPU_MODE_OPTS_DEFAULT(w.mode);
        uint64_t n = 99;
        int32_t cost = 0;
        std::unique_ptr<kgpu_token[]> out(new kgpu_token[w.tokens]);
        int rc = kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &opts, out.get(), w.tokens, &n, &cost);
        expect(rc == KGPU_OK && n == w.tokens, "an exact fit");
        expect(out[w.tokens - 1].cls == KGPU_CLASS_DUMMY && out[w.tokens - 1].position == 17, "EOS last");
        if (w.mode == KGPU_MODE_EXTENDED) expect(out[2].byte_len == 4 && out[3].byte_len == 1 && out[3].position == 16 && out[3].start == 5, "the characters of the unknown word");
        std::unique_ptr<kgpu_token[]> small(new kgpu_token[w.tokens - 1]);
        n = 99;
        rc = kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &opts, small.get(), w.tokens - 1, &n, &cost);
        expect(rc == KGPU_ERR_CAPACITY && n == w.tokens, "one short");
        rc = kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &opts, nullptr, 0, &n, &cost);
        expect(rc == KGPU_ERR_CAPACITY && n == w.tokens, "no room at all");
    }
    // the largest penalties: the product is capped, nothing wraps
    kgpu_mode_opts big = {KGPU_MODE_SEARCH, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, {0u, 0u, 0u}};
    uint64_t n = 0;
    int32_t cost = 0;
    std::unique_ptr<kgpu_token[]> out(new kgpu_token[6]);
    expect(kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &big, out.get(), 6, &n, &cost) == KGPU_OK && n == 0 && cost == (1 << 30), "capped penalties: nothing is accepted");
    // refusals: options, a node beyond the text, text that is cut inside a character
    kgpu_mode_opts bad = KGPU_MODE_OPTS_DEFAULT(3u);
    expect(kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &bad, out.get(), 6, &n, &cost) == KGPU_ERR_INVALID_ARG, "mode 3");
    bad = kgpu_mode_opts KGPU_MODE_OPTS_DEFAULT(KGPU_MODE_SEARCH);
    bad.reserved[2] = 1;
    expect(kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &bad, out.get(), 6, &n, &cost) == KGPU_ERR_INVALID_ARG, "a reserved word");
    kgpu_mode_opts ok = KGPU_MODE_OPTS_DEFAULT(KGPU_MODE_EXTENDED);
    expect(kgpu_mode_host(&lat, p_bytes.get(), len - 1, p_conn.get(), 2, 2, &ok, out.get(), 6, &n, &cost) == KGPU_ERR_INVALID_ARG, "bytes beyond the text");
    {
        std::vector<uint8_t> cut(bytes.begin(), bytes.begin() + 14);   // ends inside U+20000
        auto p_cut = exact(cut);
        expect(kgpu_mode_host(&lat, p_cut.get(), cut.size(), p_conn.get(), 2, 2, &ok, out.get(), 6, &n, &cost) == KGPU_ERR_INVALID_ARG, "a cut character");
    }
    p_nodes[4].end_char = 7;
    expect(kgpu_mode_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, &ok, out.get(), 6, &n, &cost) == KGPU_ERR_INVALID_ARG, "a node behind the characters");
    if (fails) return 1;
    std::printf("mode sanitize ok\n");
    return 0;
}
