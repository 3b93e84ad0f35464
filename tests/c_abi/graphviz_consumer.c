/* tests/c_abi/graphviz_consumer.c -- the reference's `kanpyo graphviz INPUT` (src/bin/kanpyo.rs:127-148 over src/graphviz.rs:30-163) as a C
 * consumer of include/kanpyo_gpu.h alone: C99, links libkanpyo_gpu.so.
 *
 *   graphviz_consumer <dir> <input> [dpi [full_state]]
 *
 * <dir> holds the blobs as tests/c_abi/lines_consumer.c reads them.  The sentence goes through kgpu_graphviz_batch twice, the two-call
 * size protocol: with no buffer at all (KGPU_ERR_CAPACITY and the exact size), then with a buffer of exactly that size; the DOT document goes
 * to stdout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kanpyo_gpu.h"

static uint8_t *slurp(const char *dir, const char *name, size_t *len) {
    char path[4096];
    size_t cap = 1 << 16, n = 0, got;
    uint8_t *buf = (uint8_t *)malloc(cap);
    FILE *f;
    snprintf(path, sizeof path, "%s/%s", dir, name);
    f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    while (buf && (got = fread(buf + n, 1, cap - n, f)) > 0) {
        n += got;
        if (n == cap) { cap *= 2; buf = (uint8_t *)realloc(buf, cap); }
    }
    if (!buf) { fprintf(stderr, "out of memory\n"); exit(2); }
    fclose(f);
    *len = n;
    return buf;
}

static int check(int rc, const char *what) {
    if (rc != KGPU_OK) { fprintf(stderr, "%s: %d %s\n", what, rc, kgpu_last_error()); exit(3); }
    return rc;
}

int main(int argc, char **argv) {
    kgpu_dict_blobs b;
    kgpu_dict *d = NULL;
    size_t mf_len, uf_len;
    uint8_t *mf, *uf, *text, status = 0;
    uint64_t offs[2], toff[2], need = 0, got = 0, dpi = 48;
    int full_state = 0, rc;
    if (argc < 3 || argc > 5) { fprintf(stderr, "usage: graphviz_consumer <dir> <input> [dpi [full_state]]\n"); return 2; }
    if (argc > 3) dpi = strtoull(argv[3], NULL, 10);
    if (argc > 4) full_state = atoi(argv[4]);
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

    offs[0] = 0;
    offs[1] = strlen(argv[2]);
    rc = kgpu_graphviz_batch(d, (const uint8_t *)argv[2], offs, 1, dpi, full_state, NULL, 0, toff, &status, &need);   /* the first call sizes */
    if (rc != KGPU_ERR_CAPACITY) { fprintf(stderr, "sizing call: %d %s\n", rc, kgpu_last_error()); return 3; }
    text = (uint8_t *)malloc((size_t)need);
    if (!text) { fprintf(stderr, "out of memory\n"); return 2; }
    check(kgpu_graphviz_batch(d, (const uint8_t *)argv[2], offs, 1, dpi, full_state, text, need, toff, &status, &got), "kgpu_graphviz_batch");
    if (got != need || toff[0] != 0 || toff[1] != got) { fprintf(stderr, "sizes: %llu then %llu\n", (unsigned long long)need, (unsigned long long)got); return 3; }
    if (status != KGPU_SENT_OK) { fprintf(stderr, "sentence status %d\n", (int)status); return 101; }
    fwrite(text, 1, (size_t)got, stdout);
    free(text);
    kgpu_dict_destroy(d);
    return 0;
}
