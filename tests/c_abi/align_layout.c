/* tests/c_abi/align_layout.c -- the layout of the two records of the source alignment (include/kanpyo_gpu.h, "source alignment"), pinned from C:
 * tests/test_align_cpu.py compiles this with -std=c99 -pedantic -Werror and runs it. */
#include <stddef.h>
#include <stdio.h>

#include "kanpyo_gpu.h"

#define PIN(cond) do { if (!(cond)) { printf("layout: %s\n", #cond); return 1; } } while (0)

int main(void) {
    PIN(sizeof(kgpu_norm_edit) == 24);
    PIN(offsetof(kgpu_norm_edit, out_pos) == 0 && offsetof(kgpu_norm_edit, src_pos) == 4 && offsetof(kgpu_norm_edit, out_char) == 8 && offsetof(kgpu_norm_edit, src_char) == 12);
    PIN(offsetof(kgpu_norm_edit, out_len) == 16 && offsetof(kgpu_norm_edit, src_len) == 18 && offsetof(kgpu_norm_edit, out_chars) == 20 && offsetof(kgpu_norm_edit, src_chars) == 22);
    PIN(sizeof(kgpu_span) == 16);
    PIN(offsetof(kgpu_span, position) == 0 && offsetof(kgpu_span, byte_len) == 4 && offsetof(kgpu_span, start) == 8 && offsetof(kgpu_span, end) == 12);
    PIN(sizeof(kgpu_token) == 24);
    printf("align layout ok\n");
    return 0;
}
