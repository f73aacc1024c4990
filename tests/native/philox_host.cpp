// philox_host -- the host build of csrc/rtx_common.h's counter RNG, for tests/test_philox_draws.py (no GPU is touched).
// stdin : one draw per line, "seed offset index p" (unsigned 64-bit decimals, p a float)
// stdout: "x y z w keep normal" per line -- the four Philox words and the bits of rtx_normal's float in hex, keep as 0 / 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../rectorch_amd/csrc/rtx_common.h"

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char* q = line;
        const uint64_t seed = strtoull(q, &q, 10), offset = strtoull(q, &q, 10), index = strtoull(q, &q, 10);
        const float p = strtof(q, &q);
        const Philox4 r = philox4x32_10(seed, offset, index);
        const float n = rtx_normal(seed, offset, index);
        uint32_t nb;
        memcpy(&nb, &n, sizeof nb);
        printf("%08x %08x %08x %08x %d %08x\n", r.x, r.y, r.z, r.w, rtx_dropout_keep(seed, offset, index, p) ? 1 : 0, nb);
    }
    return 0;
}
