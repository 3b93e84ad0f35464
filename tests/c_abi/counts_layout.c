/* tests/c_abi/counts_layout.c -- sizeof / offsetof of kgpu_counts_opts and kgpu_counts_info and the values of the KGPU_COUNTS_* constants, in
 * the format of tests/c_abi/layout.c ("struct field offset size"; field "-" = the whole struct; constants as "const NAME value 0").  C99,
 * includes only the public header; tests/test_count_cpu.py compares the output with the ctypes mirrors (kanpyo_amd/_lib.py). */
#include <stddef.h>
#include <stdio.h>

#include "kanpyo_gpu.h"

#define S(T) printf("%s - 0 %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))
#define K(c) printf("const %s %llu 0\n", #c, (unsigned long long)(c))

int main(void) {
    S(kgpu_counts_opts);
    F(kgpu_counts_opts, size); F(kgpu_counts_opts, reserved); F(kgpu_counts_opts, table_slots); F(kgpu_counts_opts, key_bytes);
    S(kgpu_counts_info);
    F(kgpu_counts_info, size); F(kgpu_counts_info, reserved); F(kgpu_counts_info, tokens_counted); F(kgpu_counts_info, overflow_tokens);
    F(kgpu_counts_info, sentences); F(kgpu_counts_info, table_slots); F(kgpu_counts_info, table_slots_used); F(kgpu_counts_info, key_bytes);
    F(kgpu_counts_info, key_bytes_used);
    K(KGPU_COUNTS_DEFAULT_SLOTS); K(KGPU_COUNTS_DEFAULT_KEY_BYTES);
    return 0;
}
