// Stand-alone driver of csrc/slot_tables_plan.h for tests/test_slot_tables_plan.py (g++, no HIP).
// stdin: nothing.  stdout, for every max_free M = -1 .. 32:
//   "M rc S max_low lds_bytes" and the S values of widest
//   then for every F = 0 .. M (rc == 0 only) two lines:
//     "slot F L plain top" and per launch s < S "k width" (k < 0 once the root is finished)
//     "deep F L plain n_launches" and per launch of deep_batch_plan for ONE root of F, low_bits = 0, "k grid_x grid_y"
#include <stdio.h>

#include "deep_batch.h"
#include "slot_tables_plan.h"

int main()
{
    for (int M = -1; M <= 32; M++) {
        SlotTablesPlan p;
        const int rc = slot_tables_plan(M, p);
        printf("%d %d %d %d %u", M, rc, (int)p.n_launches, (int)p.max_low, p.lds_bytes);
        for (int s = 0; s < p.n_launches; s++) printf(" %u", p.widest[s]);
        printf("\n");
        if (rc != 0) continue;
        for (int F = 0; F <= M; F++) {
            const SlotTablesDepth &d = p.depth[F];
            printf("slot %d %d %d %d", F, (int)d.L, d.plain ? 1 : 0, (int)d.top);
            for (int s = 0; s < p.n_launches; s++) printf(" %d %u", slot_tables_layer(d, s), slot_tables_width(d, s));
            printf("\n");
            const int32_t one = F;
            DeepBatchPlan b;
            if (deep_batch_plan(&one, 1, M, 1, 0, b) != 0 || b.groups.size() != 1) return 3;
            printf("deep %d %d %d %zu", F, (int)b.groups[0].L, b.groups[0].plain ? 1 : 0, b.launches.size());
            for (const DeepBatchLaunch &l : b.launches) printf(" %d %u %u", (int)l.k, l.grid_x, l.grid_y);
            printf("\n");
        }
    }
    return 0;
}
