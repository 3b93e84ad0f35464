/* tests/c_abi/encode_consumer.c -- vocabulary ids over stdin as a C consumer of include/kanpyo_gpu.h alone: C99, links libkanpyo_gpu.so.
 *
 *   encode_consumer <dir> <field> <filter> <vocab file> <unk_id> <bos_id | -> <eos_id | -> [name ...] < input
 *
 * <dir> holds the blobs as tests/c_abi/lines_consumer.c reads them; <vocab file> has one word per line, line k (0-based) is id k.  The input
 * goes through kgpu_encode_text (split and trim on the device, sized by its exact-sizes protocol) and, split on the host, through
 * kgpu_encode_batch (sized by its KGPU_ERR_CAPACITY); both must agree (exit status 4 otherwise).  The dictionary and the words handle are
 * destroyed before the first encode: the vocabulary handle keeps the tables alive.  Output: per input line its ids in decimal, separated by
 * one space.  Exit status 101 at an invalid UTF-8 line, with nothing printed. */
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

static uint8_t *slurp_path(const char *path, size_t *len) {
    FILE *f = fopen(path, "rb");
    uint8_t *b;
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    b = slurp_file(f, len);
    fclose(f);
    return b;
}

static uint8_t *slurp(const char *dir, const char *name, size_t *len) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    return slurp_path(path, len);
}

static int check(int rc, const char *what) {
    if (rc != KGPU_OK) { fprintf(stderr, "%s: %d %s\n", what, rc, kgpu_last_error()); exit(3); }
    return rc;
}

int main(int argc, char **argv) {
    kgpu_dict_blobs b;
    kgpu_dict *d = NULL;
    kgpu_words *w = NULL;
    kgpu_vocab *v = NULL;
    kgpu_words_spec spec;
    kgpu_vocab_opts opts;
    kgpu_vocab_info info;
    size_t mf_len, uf_len, in_len, vf_len, name_bytes = 0, at, start;
    uint8_t *mf, *uf, *in, *vf, *lines, *status, *status2, *names, *vwords;
    uint64_t n = 0, n2 = 0, n_ids = 0, n_ids2 = 0, i, j, *offs, *name_offs, *voffs, n_words = 0, *ioff, *ioff2;
    int32_t *ids, *ids2;
    int rc, k, n_names;
    if (argc < 8) { fprintf(stderr, "usage: encode_consumer <dir> <field> <filter> <vocab file> <unk_id> <bos_id|-> <eos_id|-> [name ...] < input\n"); return 2; }
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

    n_names = argc - 8;
    for (k = 0; k < n_names; ++k) name_bytes += strlen(argv[8 + k]);
    names = (uint8_t *)malloc(name_bytes + 1);
    name_offs = (uint64_t *)malloc((size_t)(n_names + 1) * sizeof(uint64_t));
    name_offs[0] = 0;
    for (k = 0; k < n_names; ++k) {
        const size_t len = strlen(argv[8 + k]);
        memcpy(names + name_offs[k], argv[8 + k], len);
        name_offs[k + 1] = name_offs[k] + len;
    }
    memset(&spec, 0, sizeof spec);
    spec.size = (uint32_t)sizeof spec;
    spec.field = (int32_t)atoi(argv[2]);
    spec.filter = (uint32_t)atoi(argv[3]);
    spec.names = names; spec.name_offsets = name_offs; spec.n_names = (uint64_t)n_names;
    check(kgpu_words_create(d, &spec, &w), "kgpu_words_create");

    /* the vocabulary file: every '\n'-terminated line is a word; packed in place (the newlines squeezed out) */
    vf = slurp_path(argv[4], &vf_len);
    for (at = 0; at < vf_len; ++at) n_words += vf[at] == '\n';
    vwords = (uint8_t *)malloc(vf_len + 1);
    voffs = (uint64_t *)malloc((size_t)(n_words + 1) * sizeof(uint64_t));
    voffs[0] = 0;
    for (at = 0, start = 0, i = 0; at < vf_len; ++at)
        if (vf[at] == '\n') {
            memcpy(vwords + voffs[i], vf + start, at - start);
            voffs[i + 1] = voffs[i] + (at - start);
            ++i;
            start = at + 1;
        }
    memset(&opts, 0, sizeof opts);
    opts.size = (uint32_t)sizeof opts;
    opts.unk_id = (int32_t)atoi(argv[5]);
    if (strcmp(argv[6], "-") != 0) { opts.flags |= KGPU_VOCAB_ADD_BOS; opts.bos_id = (int32_t)atoi(argv[6]); }
    if (strcmp(argv[7], "-") != 0) { opts.flags |= KGPU_VOCAB_ADD_EOS; opts.eos_id = (int32_t)atoi(argv[7]); }
    check(kgpu_vocab_create(w, vwords, voffs, n_words, &opts, &v), "kgpu_vocab_create");
    memset(&info, 0, sizeof info);
    info.size = (uint32_t)sizeof info;
    check(kgpu_vocab_get_info(v, &info), "kgpu_vocab_get_info");
    if (info.n_words != n_words || info.table_slots < 16 || info.table_slots < 2 * n_words || (info.table_slots & (info.table_slots - 1)) != 0) {
        fprintf(stderr, "kgpu_vocab_get_info: %llu words, %llu slots\n", (unsigned long long)info.n_words, (unsigned long long)info.table_slots);
        return 4;
    }
    kgpu_words_destroy(w);                                            /* the vocabulary handle outlives both */
    kgpu_dict_destroy(d);

    in = slurp_file(stdin, &in_len);
    rc = kgpu_encode_text(v, in, in_len, NULL, 0, NULL, 0, NULL, &n, &n_ids);   /* the sizing call: both exact sizes */
    if (rc != KGPU_ERR_CAPACITY) { fprintf(stderr, "the sizing call returned %d\n", rc); return 3; }
    ids = (int32_t *)malloc((size_t)(n_ids + 1) * sizeof(int32_t));
    ioff = (uint64_t *)malloc((size_t)(n + 1) * sizeof(uint64_t));
    status = (uint8_t *)malloc((size_t)n + 1);
    check(kgpu_encode_text(v, in, in_len, ids, n_ids, ioff, n + 1, status, &n, &n_ids), "kgpu_encode_text");

    lines = (uint8_t *)malloc(in_len + 1);
    offs = (uint64_t *)malloc((size_t)(n + 2) * sizeof(uint64_t));
    check(kgpu_split_lines(in, in_len, lines, offs, n + 1, &n2), "kgpu_split_lines");
    ioff2 = (uint64_t *)malloc((size_t)(n2 + 1) * sizeof(uint64_t));
    status2 = (uint8_t *)malloc((size_t)n2 + 1);
    rc = kgpu_encode_batch(v, lines, offs, n2, NULL, 0, ioff2, status2, &n_ids2);
    if (n_ids2 != n_ids || (n_ids && rc != KGPU_ERR_CAPACITY)) { fprintf(stderr, "kgpu_encode_batch sizes %llu ids, kgpu_encode_text %llu\n", (unsigned long long)n_ids2, (unsigned long long)n_ids); return 4; }
    ids2 = (int32_t *)malloc((size_t)(n_ids2 + 1) * sizeof(int32_t));
    check(kgpu_encode_batch(v, lines, offs, n2, ids2, n_ids2, ioff2, status2, &n_ids2), "kgpu_encode_batch");
    if (n2 != n || memcmp(status, status2, (size_t)n) != 0 || memcmp(ioff, ioff2, (size_t)(n + 1) * sizeof(uint64_t)) != 0 ||
        memcmp(ids, ids2, (size_t)n_ids * sizeof(int32_t)) != 0) {
        fprintf(stderr, "kgpu_encode_text differs from kgpu_encode_batch\n");
        return 4;
    }
    kgpu_vocab_destroy(v);
    for (i = 0; i < n; ++i)
        if (status[i] == KGPU_SENT_INVALID_UTF8) {
            fprintf(stderr, "line %llu is not UTF-8\n", (unsigned long long)(i + 1));
            return 101;
        }
    for (i = 0; i < n; ++i) {
        for (j = ioff[i]; j < ioff[i + 1]; ++j) printf(j == ioff[i] ? "%d" : " %d", (int)ids[j]);
        fputc('\n', stdout);
    }
    return 0;
}
