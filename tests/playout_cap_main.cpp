// playout_cap_main.cpp -- playout_is_full (csrc/playout_cap.h) on the host: reads "seed game_idx ply full_prob" lines
// (seed in hex, full_prob as a C99 hexadecimal float), writes "is_full word0 thresh" per line.
// Built by tests/test_playout_cap_rule.py for the host only, under AddressSanitizer and UBSan.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "playout_cap.h"

int main()
{
    char seed_s[64], prob_s[64];
    long long game;
    unsigned ply;
    while (scanf("%63s %lld %u %63s", seed_s, &game, &ply, prob_s) == 4) {
        const uint64_t seed = strtoull(seed_s, nullptr, 16);
        const double p = strtod(prob_s, nullptr);
        const PlayoutCap pc = playout_cap_make(p, 1);
        const uint64_t g = (uint64_t)game;
        const uint32_t x = playout_philox_x((uint32_t)g, (uint32_t)(g >> 32), ply, PLAYOUT_PURPOSE, (uint32_t)seed, (uint32_t)(seed >> 32));
        printf("%d %" PRIu32 " %" PRIu64 "\n", playout_is_full(pc, seed, (int64_t)game, ply) ? 1 : 0, x, pc.thresh);
    }
    // the check value of include/dbaz.h: counter (1, 2, 3, 0x33333333), key (7, 0)
    return playout_philox_x(1u, 2u, 3u, PLAYOUT_PURPOSE, 7u, 0u) == 1157962352u ? 0 : 3;
}
