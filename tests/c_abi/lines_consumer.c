/* tests/c_abi/lines_consumer.c -- the reference's `kanpyo tokenize` over stdin (src/bin/kanpyo.rs:106-126, 174-197) as a C consumer of
 * include/kanpyo_gpu.h alone: C99, links libkanpyo_gpu.so.
 *
 *   lines_consumer <dir> < input
 *
 * <dir> holds the blobs as the reference serialises them (DictReadWrite::write_dict): index.dict, connection.dict, morph.dict, unk.dict
 * (with its trailing feature table, which kgpu_dict_create ignores), char_category.bin, invoke.bin, group.bin, morph_feature.dict and
 * unk_feature.dict (unk.dict's feature table alone).  The input is split and trimmed as read_line + trim_end do (kgpu_split_lines), every
 * line is tokenized and rendered in one kgpu_tokenize_batch_lines call, and the text goes to stdout.  Exit status 101 (a Rust panic's) at
 * an invalid UTF-8 line, after the lines in front of it. */
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
    size_t mf_len, uf_len, in_len;
    uint8_t *mf, *uf, *in, *lines, *text, *status;
    uint64_t n = 0, cap, got = 0, i, *offs, *toff;
    int rc;
    if (argc != 2) { fprintf(stderr, "usage: lines_consumer <dir> < input\n"); return 2; }
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
    status = (uint8_t *)malloc((size_t)n + 1);
    cap = 16;
    text = (uint8_t *)malloc((size_t)cap);
    rc = kgpu_tokenize_batch_lines(d, lines, offs, n, text, cap, toff, status, &got);
    if (rc == KGPU_ERR_CAPACITY) {                                    /* *n_bytes is the exact size needed */
        free(text);
        cap = got;
        text = (uint8_t *)malloc((size_t)cap + 1);
        rc = kgpu_tokenize_batch_lines(d, lines, offs, n, text, cap, toff, status, &got);
    }
    check(rc, "kgpu_tokenize_batch_lines");
    for (i = 0; i < n; ++i)
        if (status[i] == KGPU_SENT_INVALID_UTF8) {
            fwrite(text, 1, (size_t)toff[i], stdout);
            fflush(stdout);
            fprintf(stderr, "line %llu is not UTF-8\n", (unsigned long long)i);
            return 101;
        }
    fwrite(text, 1, (size_t)got, stdout);
    kgpu_dict_destroy(d);
    return 0;
}
