/* tests/c_abi/encode_layout.c -- sizeof / offsetof of kgpu_vocab_opts and kgpu_vocab_info and the values of the KGPU_VOCAB_* constants, in the
 * format of tests/c_abi/layout.c ("struct field offset size"; field "-" = the whole struct; constants as "const NAME value 0").  C99,
 * includes only the public header; tests/test_encode_cpu.py compares the output with the ctypes mirrors (kanpyo_amd/_lib.py). */
#include <stddef.h>
#include <stdio.h>

#include "kanpyo_gpu.h"

#define S(T) printf("%s - 0 %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))
#define K(c) printf("const %s %llu 0\n", #c, (unsigned long long)(c))

int main(void) {
    S(kgpu_vocab_opts);
    F(kgpu_vocab_opts, size); F(kgpu_vocab_opts, flags); F(kgpu_vocab_opts, unk_id); F(kgpu_vocab_opts, bos_id); F(kgpu_vocab_opts, eos_id);
    S(kgpu_vocab_info);
    F(kgpu_vocab_info, size); F(kgpu_vocab_info, reserved); F(kgpu_vocab_info, n_words); F(kgpu_vocab_info, table_slots);
    F(kgpu_vocab_info, key_bytes); F(kgpu_vocab_info, rows_resolved);
    K(KGPU_VOCAB_ADD_BOS); K(KGPU_VOCAB_ADD_EOS);
    return 0;
}
