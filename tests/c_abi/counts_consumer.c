/* tests/c_abi/counts_consumer.c -- word counts over stdin as a C consumer of include/kanpyo_gpu.h alone: C99, links libkanpyo_gpu.so.
 *
 *   counts_consumer <dir> <field> <filter> <top> [name ...] < input
 *
 * <dir> holds the blobs as tests/c_abi/lines_consumer.c reads them.  The input goes through kgpu_count_text (split and trim on the device)
 * into one handle and, split on the host, through kgpu_count_batch into a second one; both handles are read out with the exact-sizes
 * protocol of kgpu_counts_read and must agree (exit status 4 otherwise).  The dictionary and the words handle are destroyed before the
 * read-out: the counts handles keep the tables alive.  Output: "count\tword\n" per entry.  Exit status 101 at an invalid UTF-8 line, with
 * nothing printed. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kanpyo_gpu.h"

static uint8_t *slurp_file(FILE *f, size_t *len) {
    size_t cap = 1 << 16, n = 0;
    uint8_t *buf = (uint8_t *)malloc(cap);
    size_t got;
    while (buf && (got = fread(buf + n, 1, cap - n, f)) > 0) {
        n += got;
        if (n == cap) { cap *= 2; buf = (uint8_t *)realloc(buf, cap); }
    }
    if (!buf) { fprintf(stderr, "out of memory\n"); exit(2); }
    *len = n;
    return buf;
}

static uint8_t *slurp(const char *dir, const char *name, size_t *len) {
    char path[4096];
    FILE *f;
    uint8_t *b;
    snprintf(path, sizeof path, "%s/%s", dir, name);
    f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    b = slurp_file(f, len);
    fclose(f);
    return b;
}

static int check(int rc, const char *what) {
    if (rc != KGPU_OK) { fprintf(stderr, "%s: %d %s\n", what, rc, kgpu_last_error()); exit(3); }
    return rc;
}

struct readout { uint8_t *words; uint64_t *offs, *counts, n, bytes; };

static struct readout read_out(kgpu_counts *k, uint64_t top) {
    struct readout r;
    memset(&r, 0, sizeof r);
    if (kgpu_counts_read(k, top, NULL, 0, NULL, NULL, 0, &r.n, &r.bytes) == KGPU_ERR_CAPACITY || r.n == 0) {   /* the first call sizes */
        r.words = (uint8_t *)malloc((size_t)r.bytes + 1);
        r.offs = (uint64_t *)malloc((size_t)(r.n + 1) * sizeof(uint64_t));
        r.counts = (uint64_t *)malloc((size_t)(r.n + 1) * sizeof(uint64_t));
        check(kgpu_counts_read(k, top, r.words, r.bytes, r.offs, r.counts, r.n, &r.n, &r.bytes), "kgpu_counts_read");
    } else {
        fprintf(stderr, "kgpu_counts_read: %s\n", kgpu_last_error());
        exit(3);
    }
    return r;
}

int main(int argc, char **argv) {
    kgpu_dict_blobs b;
    kgpu_dict *d = NULL;
    kgpu_words *w = NULL;
    kgpu_counts *ka = NULL, *kb = NULL;
    kgpu_words_spec spec;
    kgpu_counts_opts opts;
    kgpu_counts_info info;
    size_t mf_len, uf_len, in_len, name_bytes = 0;
    uint8_t *mf, *uf, *in, *lines, *status, *status2, *names;
    uint64_t n = 0, n2 = 0, i, sum = 0, *offs, *name_offs;
    struct readout ra, rb;
    int rc, k, n_names;
    if (argc < 5) { fprintf(stderr, "usage: counts_consumer <dir> <field> <filter> <top> [name ...] < input\n"); return 2; }
    memset(&b, 0, sizeof b);
    b.index_dict = slurp(argv[1], "index.dict", &b.index_len);
    b.connection_dict = slurp(argv[1], "connection.dict", &b.connection_len);
    b.morph_dict = slurp(argv[1], "morph.dict", &b.morph_len);
    b.unk_dict = slurp(argv[1], "unk.dict", &b.unk_len);
    b.char_category = slurp(argv[1], "char_category.bin", &b.char_category_len);
    b.invoke_list = slurp(argv[1], "invoke.bin", &b.invoke_len);
    b.group_list = slurp(argv[1], "group.bin", &b.group_len);
    mf = slurp(argv[1], "morph_feature.dict", &mf_len);
    uf = slurp(argv[1], "unk_feature.dict", &uf_len);
    check(kgpu_dict_create(&b, 0, &d), "kgpu_dict_create");
    check(kgpu_dict_set_features(d, mf, mf_len, uf, uf_len), "kgpu_dict_set_features");

    n_names = argc - 5;
    for (k = 0; k < n_names; ++k) name_bytes += strlen(argv[5 + k]);
    names = (uint8_t *)malloc(name_bytes + 1);
    name_offs = (uint64_t *)malloc((size_t)(n_names + 1) * sizeof(uint64_t));
    name_offs[0] = 0;
    for (k = 0; k < n_names; ++k) {
        const size_t len = strlen(argv[5 + k]);
        memcpy(names + name_offs[k], argv[5 + k], len);
        name_offs[k + 1] = name_offs[k] + len;
    }
    memset(&spec, 0, sizeof spec);
    spec.size = (uint32_t)sizeof spec;
    spec.field = (int32_t)atoi(argv[2]);
    spec.filter = (uint32_t)atoi(argv[3]);
    spec.names = names; spec.name_offsets = name_offs; spec.n_names = (uint64_t)n_names;
    check(kgpu_words_create(d, &spec, &w), "kgpu_words_create");
    memset(&opts, 0, sizeof opts);
    opts.size = (uint32_t)sizeof opts;
    opts.table_slots = 1024; opts.key_bytes = 1 << 16;
    check(kgpu_counts_create(w, &opts, &ka), "kgpu_counts_create");
    check(kgpu_counts_create(w, &opts, &kb), "kgpu_counts_create");

    in = slurp_file(stdin, &in_len);
    status = (uint8_t *)malloc(in_len + 1);
    rc = kgpu_count_text(ka, in, in_len, status, 0, &n);            /* no room for the status bytes: the line count, nothing counted */
    if (n != 0 && rc != KGPU_ERR_CAPACITY) { fprintf(stderr, "a status array of no entries was accepted\n"); return 3; }
    check(kgpu_count_text(ka, in, in_len, status, n, &n), "kgpu_count_text");

    lines = (uint8_t *)malloc(in_len + 1);
    offs = (uint64_t *)malloc((size_t)(n + 2) * sizeof(uint64_t));
    check(kgpu_split_lines(in, in_len, lines, offs, n + 1, &n2), "kgpu_split_lines");
    status2 = (uint8_t *)malloc((size_t)n2 + 1);
    check(kgpu_count_batch(kb, lines, offs, n2, status2), "kgpu_count_batch");
    if (n2 != n || memcmp(status, status2, (size_t)n) != 0) { fprintf(stderr, "kgpu_count_text differs from kgpu_count_batch in its status\n"); return 4; }

    kgpu_words_destroy(w);                                            /* the counts handles outlive both */
    kgpu_dict_destroy(d);
    ra = read_out(ka, (uint64_t)strtoull(argv[4], NULL, 10));
    rb = read_out(kb, (uint64_t)strtoull(argv[4], NULL, 10));
    if (ra.n != rb.n || ra.bytes != rb.bytes || memcmp(ra.words, rb.words, (size_t)ra.bytes) != 0 ||
        memcmp(ra.offs, rb.offs, (size_t)(ra.n + 1) * sizeof(uint64_t)) != 0 || memcmp(ra.counts, rb.counts, (size_t)ra.n * sizeof(uint64_t)) != 0) {
        fprintf(stderr, "the two handles differ\n");
        return 4;
    }
    memset(&info, 0, sizeof info);
    info.size = (uint32_t)sizeof info;
    check(kgpu_counts_get_info(ka, &info), "kgpu_counts_get_info");
    for (i = 0; i < ra.n; ++i) sum += ra.counts[i];
    if (info.sentences != n || info.overflow_tokens != 0 || (strtoull(argv[4], NULL, 10) == 0 && sum != info.tokens_counted)) {
        fprintf(stderr, "kgpu_counts_get_info: %llu sentences, %llu counted, %llu overflow; the entries sum to %llu over %llu lines\n",
                (unsigned long long)info.sentences, (unsigned long long)info.tokens_counted, (unsigned long long)info.overflow_tokens,
                (unsigned long long)sum, (unsigned long long)n);
        return 4;
    }
    check(kgpu_counts_reset(kb), "kgpu_counts_reset");
    rb = read_out(kb, 0);
    if (rb.n != 0) { fprintf(stderr, "a reset handle has entries\n"); return 4; }
    kgpu_counts_destroy(kb);
    kgpu_counts_destroy(ka);
    for (i = 0; i < n; ++i)
        if (status[i] == KGPU_SENT_INVALID_UTF8) {
            fprintf(stderr, "line %llu is not UTF-8\n", (unsigned long long)(i + 1));
            return 101;
        }
    for (i = 0; i < ra.n; ++i) {
        printf("%llu\t", (unsigned long long)ra.counts[i]);
        fwrite(ra.words + ra.offs[i], 1, (size_t)(ra.offs[i + 1] - ra.offs[i]), stdout);
        fputc('\n', stdout);
    }
    return 0;
}
