/* tests/c_abi/words_consumer.c -- wakati-gaki over stdin as a C consumer of include/kanpyo_gpu.h alone: C99, links libkanpyo_gpu.so.
 *
 *   words_consumer <dir> <field> <filter> <separator byte value> [name ...] < input
 *
 * <dir> holds the blobs as tests/c_abi/lines_consumer.c reads them.  The input is split and trimmed on the host (kgpu_split_lines) and
 * rendered by kgpu_tokenize_batch_words, one output line per input line; the same block then goes through kgpu_tokenize_text_words (split
 * and trim on the device), which must give the same bytes (exit status 4 otherwise).  The dictionary handle is destroyed before the second
 * call: the words handle keeps the tables alive.  Exit status 101 at an invalid UTF-8 line, after the lines in front of it. */
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

int main(int argc, char **argv) {
    kgpu_dict_blobs b;
    kgpu_dict *d = NULL;
    kgpu_words *w = NULL;
    kgpu_words_spec spec;
    size_t mf_len, uf_len, in_len, name_bytes = 0;
    uint8_t *mf, *uf, *in, *lines, *text, *text2, *status, *names;
    uint64_t n = 0, n2 = 0, cap, got = 0, got2 = 0, i, *offs, *toff, *toff2, *name_offs;
    int rc, k, n_names;
    if (argc < 5) { fprintf(stderr, "usage: words_consumer <dir> <field> <filter> <separator byte value> [name ...] < input\n"); return 2; }
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
    spec.separator = (uint32_t)atoi(argv[4]);
    spec.names = names; spec.name_offsets = name_offs; spec.n_names = (uint64_t)n_names;
    if (kgpu_words_create(d, &spec, &w) != KGPU_ERR_INVALID_ARG) { fprintf(stderr, "a handle without feature tables was accepted\n"); return 3; }
    check(kgpu_dict_set_features(d, mf, mf_len, uf, uf_len), "kgpu_dict_set_features");
    check(kgpu_words_create(d, &spec, &w), "kgpu_words_create");

    in = slurp_file(stdin, &in_len);
    lines = (uint8_t *)malloc(in_len + 1);
    offs = (uint64_t *)malloc(sizeof(uint64_t));
    rc = kgpu_split_lines(in, in_len, lines, offs, 1, &n);           /* the first call counts the lines */
    if (rc == KGPU_ERR_CAPACITY) {
        free(offs);
        offs = (uint64_t *)malloc((size_t)(n + 1) * sizeof(uint64_t));
        rc = kgpu_split_lines(in, in_len, lines, offs, n + 1, &n);
    }
    check(rc, "kgpu_split_lines");

    toff = (uint64_t *)malloc((size_t)(n + 1) * sizeof(uint64_t));
    toff2 = (uint64_t *)malloc((size_t)(n + 1) * sizeof(uint64_t));
    status = (uint8_t *)malloc((size_t)n + 1);
    cap = 1;
    text = (uint8_t *)malloc((size_t)cap);
    rc = kgpu_tokenize_batch_words(w, lines, offs, n, text, cap, toff, status, &got);
    if (rc == KGPU_ERR_CAPACITY) {                                    /* *n_bytes is the exact size needed */
        free(text);
        cap = got;
        text = (uint8_t *)malloc((size_t)cap + 1);
        rc = kgpu_tokenize_batch_words(w, lines, offs, n, text, cap, toff, status, &got);
    }
    check(rc, "kgpu_tokenize_batch_words");

    kgpu_dict_destroy(d);                                             /* the words handle outlives it */
    text2 = (uint8_t *)malloc((size_t)got + 1);
    check(kgpu_tokenize_text_words(w, in, in_len, text2, got, toff2, n + 1, NULL, &n2, &got2), "kgpu_tokenize_text_words");
    if (n2 != n || got2 != got || memcmp(text, text2, (size_t)got) != 0 || memcmp(toff, toff2, (size_t)(n + 1) * sizeof(uint64_t)) != 0) {
        fprintf(stderr, "kgpu_tokenize_text_words differs from kgpu_tokenize_batch_words\n");
        return 4;
    }
    kgpu_words_destroy(w);
    for (i = 0; i < n; ++i)
        if (status[i] == KGPU_SENT_INVALID_UTF8) {
            fwrite(text, 1, (size_t)toff[i], stdout);
            fflush(stdout);
            fprintf(stderr, "line %llu is not UTF-8\n", (unsigned long long)i);
            return 101;
        }
    fwrite(text, 1, (size_t)got, stdout);
    return 0;
}
