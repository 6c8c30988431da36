// knob_parse.hip -- asks parse_poison_byte (csrc/poison_knob.h) about the texts on its command line, on the CPU: no HIP
// call, no GPU.  tests/test_poison_cpu.py compiles it for the host and holds the answers to INTEGRATION.md's rule for
// NMRFIT_POISON_ALLOC.  The word UNSET stands for a variable that is not set (a null pointer).
//   knob_parse <text> ...      prints one number per text: the byte to fill with, or -1: no fill
#include "poison_knob.h"

#include <cstdio>
#include <cstring>

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) printf("%d\n", nmrfit::parse_poison_byte(strcmp(argv[i], "UNSET") == 0 ? nullptr : argv[i]));
    return 0;
}
