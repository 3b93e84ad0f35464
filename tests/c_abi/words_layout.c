/* tests/c_abi/words_layout.c -- sizeof / offsetof of kgpu_words_spec and the values of the KGPU_WORDS_* constants, in the format of
 * tests/c_abi/layout.c ("struct field offset size"; field "-" = the whole struct; constants as "const NAME value 0").  C99, includes only
 * the public header; tests/test_words_cpu.py compares the output with the ctypes mirror (kanpyo_amd/_lib.py: WordsSpec). */
#include <stddef.h>
#include <stdio.h>

#include "kanpyo_gpu.h"

#define S(T) printf("%s - 0 %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))
#define K(c) printf("const %s %d 0\n", #c, (int)(c))

int main(void) {
    S(kgpu_words_spec);
    F(kgpu_words_spec, size); F(kgpu_words_spec, field); F(kgpu_words_spec, filter); F(kgpu_words_spec, separator);
    F(kgpu_words_spec, names); F(kgpu_words_spec, name_offsets); F(kgpu_words_spec, n_names);
    K(KGPU_WORDS_SURFACE); K(KGPU_WORDS_ALL); K(KGPU_WORDS_DROP); K(KGPU_WORDS_KEEP);
    return 0;
}
