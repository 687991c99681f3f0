// Stand-alone host driver of slot_request_rule (csrc/endgame.h) for tests/test_slot_request_rule.py: the host half of the
// __host__ __device__ rule that k_endgame_table and k_slot_requests call.  No device code runs.
// stdin, one case per line, words in hex without prefix:
//   "hdr_valid hdr_game hdr_free[0..3] game free[0..3] max_free"
// stdout per case: "F keep solve"
#include <inttypes.h>
#include <stdio.h>

#include "endgame.h"

int main()
{
    int valid, max_free;
    int64_t hdr_game, game;
    uint64_t hdr_free[4], fe[4];
    while (scanf("%d %" SCNd64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNd64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %d", &valid,
                 &hdr_game, &hdr_free[0], &hdr_free[1], &hdr_free[2], &hdr_free[3], &game, &fe[0], &fe[1], &fe[2], &fe[3], &max_free) == 12) {
        const SlotDecision d = slot_request_rule(fe, valid, hdr_game, hdr_free, game, max_free);
        printf("%d %d %d\n", d.F, d.keep ? 1 : 0, d.solve ? 1 : 0);
    }
    return 0;
}
