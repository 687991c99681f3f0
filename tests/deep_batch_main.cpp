// Stand-alone driver of csrc/deep_batch.h for tests/test_deep_batch_plan.py (g++, no HIP).
// stdin: the number of cases, then per case "n max_free n_tables low_bits" and the n free-edge counts.
// stdout: first one line with default_low_bits(0 .. 31); then per case two lines:
//   rc bad_root n_groups n_launches, n x order, n x slot byte offset, per group "F L plain first count", per launch "group k grid_x grid_y"
//   the refusal's message (empty for rc == 0)
#include <stdio.h>

#include <vector>

#include "deep_batch.h"

int main()
{
    for (int E = 0; E <= 31; E++) printf("%d%c", default_low_bits(E), E == 31 ? '\n' : ' ');
    int n_cases = 0;
    if (scanf("%d", &n_cases) != 1) return 2;
    for (int i = 0; i < n_cases; i++) {
        int n = 0, max_free = 0, n_tables = 0, low_bits = 0;
        if (scanf("%d %d %d %d", &n, &max_free, &n_tables, &low_bits) != 4) return 2;
        std::vector<int32_t> F((size_t)(n > 0 ? n : 0)); // exactly the counts: the sanitizer sees any read past them
        for (size_t k = 0; k < F.size(); k++) {
            int v = 0;
            if (scanf("%d", &v) != 1) return 2;
            F[k] = v;
        }
        DeepBatchPlan p;
        const int rc = deep_batch_plan(F.data(), n, max_free, n_tables, low_bits, p);
        printf("%d %d %zu %zu", rc, (int)p.bad_root, p.groups.size(), p.launches.size());
        for (int32_t r : p.order) printf(" %d", (int)r);
        for (size_t k = 0; k < p.order.size(); k++) printf(" %lld", (long long)deep_batch_slot_offset((int32_t)k, max_free));
        for (const DeepBatchGroup &g : p.groups) printf(" %d %d %d %d %d", (int)g.F, (int)g.L, g.plain ? 1 : 0, (int)g.first, (int)g.count);
        for (const DeepBatchLaunch &l : p.launches) printf(" %d %d %u %u", (int)l.group, (int)l.k, l.grid_x, l.grid_y);
        printf("\n%s\n", p.error.c_str());
    }
    return 0;
}
