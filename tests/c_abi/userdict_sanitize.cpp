// tests/c_abi/userdict_sanitize.cpp -- kgpu_userdict_host (kanpyo_amd/csrc/kgpu_user_host.cpp over kgpu_user_table.cpp) under
// -fsanitize=address,undefined: a stand-alone program with its own main, linked with those two files alone.  It runs the host function over a crafted
// lattice and crafted entries; every buffer is a heap block of its exact size, so that a read or a write one element beyond any of them is reported.
// Built and run by tests/test_userdict_cpu.py.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "kanpyo_gpu.h"

namespace kgpu { void set_error(const char *, ...) {} }   // (the host files report through their caller's)

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

struct Entries {
    std::vector<uint8_t> keys; std::vector<uint64_t> off{0}; std::vector<uint16_t> left, right; std::vector<int16_t> cost;
    void add(const std::string &k, uint16_t l, uint16_t r, int16_t c) {
        keys.insert(keys.end(), k.begin(), k.end()); off.push_back(keys.size()); left.push_back(l); right.push_back(r); cost.push_back(c);
    }
};

}  // namespace

int main() {
    // "関西空港" + U+20000 + "a": two known words over the first two and the next two characters, unknown words over 空 alone and over the last two
    // characters; the text ends with the last node's last byte, and a key's last byte is the text's last
    const char *text = "\xE9\x96\xA2\xE8\xA5\xBF\xE7\xA9\xBA\xE6\xB8\xAF\xF0\xA0\x80\x80" "a";   // 関 西 空 港 U+20000 a
    const uint64_t len = std::strlen(text);
    std::vector<uint8_t> bytes(text, text + len);
    std::vector<kgpu_lattice_node> nodes = {
        node(0, KGPU_CLASS_DUMMY, 0, 0, 0, 0, 0, 0, 0),
        node(2, KGPU_CLASS_KNOWN, 0, 0, 2, 6, 1, 0, 700),      // 関西
        node(3, KGPU_CLASS_KNOWN, 6, 2, 4, 6, 0, 0, 700),      // 空港
        node(1, KGPU_CLASS_UNKNOWN, 12, 4, 6, 5, 1, 1, 2000),  // U+20000 a
        node(1, KGPU_CLASS_UNKNOWN, 12, 4, 5, 4, 1, 1, 2000),  // U+20000
        node(1, KGPU_CLASS_UNKNOWN, 16, 5, 6, 1, 1, 1, 2000),  // a
        node(0, KGPU_CLASS_DUMMY, 17, 6, 6, 0, 0, 0, 0),
    };
    std::vector<uint32_t> eoff = {0, 1, 1, 2, 2, 3, 4, 6, 7};   // edges[e]: the nodes ending at e; 8 positions (6 characters + 2)
    std::vector<uint32_t> enodes = {0, 1, 2, 4, 3, 5, 6};
    std::vector<int16_t> conn = {0, 5, -3, 9};
    std::vector<uint8_t> invoke = {0, 0, 0, 0, 0, 0};
    auto p_bytes = exact(bytes);
    auto p_nodes = exact(nodes);
    auto p_eoff = exact(eoff);
    auto p_enodes = exact(enodes);
    auto p_conn = exact(conn);
    auto p_invoke = exact(invoke);
    kgpu_lattice lat{nodes.size(), 8, p_nodes.get(), p_eoff.get(), p_enodes.get()};

    Entries en;
    en.add("\xE9\x96\xA2\xE8\xA5\xBF\xE7\xA9\xBA\xE6\xB8\xAF", 0, 1, -500);   // 関西空港: the whole front
    en.add("\xF0\xA0\x80\x80" "a", 1, 0, 10);                                 // the text's last two characters: the unknown words at 4 are withdrawn
    en.add("a", 0, 0, 10);                                                    // the text's last byte
    en.add("\xF0\xA0\x80\x80" "a", 1, 0, 10);                                 // the same key once more
    en.add("a\xE9\x96\xA2", 0, 0, 1);                                         // never matches: longer than what is left
    en.add(std::string(64, 'x'), 0, 0, 1);                                   // 64 characters: the longest key
    auto k = exact(en.keys);
    auto ko = exact(en.off);
    auto kl = exact(en.left);
    auto kr = exact(en.right);
    auto kc = exact(en.cost);
    const uint64_t E = en.left.size();

    struct Want { uint32_t mode; uint64_t tokens; };
    const Want wants[] = {{KGPU_MODE_NORMAL, 3}, {KGPU_MODE_SEARCH, 4}, {KGPU_MODE_EXTENDED, 4}};   // (the whole front is four kanji: its penalty gives way to the two known words)
    for (const Want &w : wants) {
        kgpu_mode_opts opts = KGPU_MODE_OPTS_DEFAULT(w.mode);
        uint64_t n = 99;
        int32_t cost = 0;
        std::unique_ptr<kgpu_token[]> out(new kgpu_token[w.tokens]);
        int rc = kgpu_userdict_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, p_invoke.get(), k.get(), ko.get(), kl.get(), kr.get(), kc.get(), E, &opts, out.get(), w.tokens, &n, &cost);
        expect(rc == KGPU_OK && n == w.tokens, "an exact fit");
        if (rc == KGPU_OK && n == w.tokens) {
            expect(out[n - 1].cls == KGPU_CLASS_DUMMY && out[n - 1].position == 17, "EOS last");
            expect(out[n - 2].cls == KGPU_CLASS_USER && out[n - 2].id == 2 && out[n - 2].position == 12 && out[n - 2].byte_len == 5, "the first of the two entries of one key");
        }
        std::unique_ptr<kgpu_token[]> small(new kgpu_token[w.tokens - 1]);
        n = 99;
        rc = kgpu_userdict_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, p_invoke.get(), k.get(), ko.get(), kl.get(), kr.get(), kc.get(), E, &opts, small.get(), w.tokens - 1, &n, &cost);
        expect(rc == KGPU_ERR_CAPACITY && n == w.tokens, "one short");
    }
    uint64_t n = 0;
    int32_t cost = 0;
    std::unique_ptr<kgpu_token[]> out(new kgpu_token[8]);
    // no entries, no options: the lattice's own best path
    expect(kgpu_userdict_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, out.get(), 8, &n, &cost) == KGPU_OK && n == 4, "E = 0");
    // refusals
    {
        Entries b; b.add("", 0, 0, 0);
        auto bk = exact(b.keys); auto bo = exact(b.off); auto bl = exact(b.left); auto br = exact(b.right); auto bc = exact(b.cost);
        expect(kgpu_userdict_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, p_invoke.get(), bk.get(), bo.get(), bl.get(), br.get(), bc.get(), 1, nullptr, out.get(), 8, &n, &cost) == KGPU_ERR_INVALID_ARG, "an empty key");
    }
    for (const std::string &key : {std::string(65, 'x'), std::string(256, 'x'), std::string("\xE9\x96"), std::string("\xED\xA0\x80"), std::string("\xC0\x80")}) {
        Entries b; b.add(key, 0, 0, 0);
        auto bk = exact(b.keys); auto bo = exact(b.off); auto bl = exact(b.left); auto br = exact(b.right); auto bc = exact(b.cost);
        expect(kgpu_userdict_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, p_invoke.get(), bk.get(), bo.get(), bl.get(), br.get(), bc.get(), 1, nullptr, out.get(), 8, &n, &cost) == KGPU_ERR_INVALID_ARG, "a key that is no key");
    }
    {
        Entries b; b.add("a", 2, 0, 0);
        auto bk = exact(b.keys); auto bo = exact(b.off); auto bl = exact(b.left); auto br = exact(b.right); auto bc = exact(b.cost);
        expect(kgpu_userdict_host(&lat, p_bytes.get(), len, p_conn.get(), 2, 2, p_invoke.get(), bk.get(), bo.get(), bl.get(), br.get(), bc.get(), 1, nullptr, out.get(), 8, &n, &cost) == KGPU_ERR_INVALID_ARG, "an id outside the matrix");
    }
    {
        std::vector<uint8_t> cut(bytes.begin(), bytes.begin() + 14);   // ends inside U+20000
        auto p_cut = exact(cut);
        expect(kgpu_userdict_host(&lat, p_cut.get(), cut.size(), p_conn.get(), 2, 2, p_invoke.get(), k.get(), ko.get(), kl.get(), kr.get(), kc.get(), E, nullptr, out.get(), 8, &n, &cost) == KGPU_ERR_INVALID_ARG, "a cut character");
    }
    {
        // a lattice with fewer positions than the text has characters: user nodes would look up predecessors behind edge_offsets
        std::vector<uint8_t> five = {'a', 'a', 'a', 'a', 'a'};
        std::vector<kgpu_lattice_node> two = {node(0, KGPU_CLASS_DUMMY, 0, 0, 0, 0, 0, 0, 0), node(0, KGPU_CLASS_DUMMY, 1, 1, 1, 0, 0, 0, 0)};
        std::vector<uint32_t> eo = {0, 1, 1}, enn = {0, 1};
        std::vector<uint8_t> inv5 = {0, 0, 0, 0, 0};
        auto p5 = exact(five); auto pn = exact(two); auto peo = exact(eo); auto pen = exact(enn); auto pi = exact(inv5);
        kgpu_lattice small{2, 2, pn.get(), peo.get(), pen.get()};
        Entries b; b.add("a", 0, 0, 1);
        auto bk = exact(b.keys); auto bo = exact(b.off); auto bl = exact(b.left); auto br = exact(b.right); auto bc = exact(b.cost);
        expect(kgpu_userdict_host(&small, p5.get(), 5, p_conn.get(), 2, 2, pi.get(), bk.get(), bo.get(), bl.get(), br.get(), bc.get(), 1, nullptr, out.get(), 8, &n, &cost) == KGPU_ERR_INVALID_ARG, "fewer positions than characters + 2");
        expect(kgpu_userdict_host(&small, p5.get(), 5, p_conn.get(), 2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, out.get(), 8, &n, &cost) == KGPU_ERR_INVALID_ARG, "... without entries too");
    }
    if (fails) return 1;
    std::printf("userdict sanitize ok\n");
    return 0;
}
