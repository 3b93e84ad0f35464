/* tests/c_abi/wordpiece_layout.c -- sizeof / offsetof of kgpu_wordpiece_opts and kgpu_wordpiece_info in the format of tests/c_abi/layout.c
 * ("struct field offset size"; field "-" = the whole struct).  C99, includes only the public header; tests/test_wordpiece_cpu.py compares the
 * output with the ctypes mirrors (kanpyo_amd/_lib.py). */
#include <stddef.h>
#include <stdio.h>

#include "kanpyo_gpu.h"

#define S(T) printf("%s - 0 %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))

int main(void) {
    S(kgpu_wordpiece_opts);
    F(kgpu_wordpiece_opts, size); F(kgpu_wordpiece_opts, max_word_chars); F(kgpu_wordpiece_opts, prefix_len); F(kgpu_wordpiece_opts, prefix);
    S(kgpu_wordpiece_info);
    F(kgpu_wordpiece_info, size); F(kgpu_wordpiece_info, reserved); F(kgpu_wordpiece_info, cont_words); F(kgpu_wordpiece_info, cont_table_slots);
    F(kgpu_wordpiece_info, cont_key_bytes); F(kgpu_wordpiece_info, rows_whole); F(kgpu_wordpiece_info, rows_split); F(kgpu_wordpiece_info, rows_unk);
    F(kgpu_wordpiece_info, row_piece_ids); F(kgpu_wordpiece_info, max_initial_bytes); F(kgpu_wordpiece_info, max_cont_bytes);
    return 0;
}
