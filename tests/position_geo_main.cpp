// Stand-alone driver of csrc/position_geo.h for tests/test_position_geo.py (g++, no HIP).
// stdin: the number of cases, then per case "rows cols" and the 3*H*W values of one feature row.
// stdout per case one line: rc F free_edges[0..3] then, for rc == 0, F x "act other0 other1".
#include <stdio.h>

#include <vector>

#include "position_geo.h"

int main()
{
    int n_cases = 0;
    if (scanf("%d", &n_cases) != 1) return 2;
    for (int i = 0; i < n_cases; i++) {
        int rows = 0, cols = 0;
        if (scanf("%d %d", &rows, &cols) != 2) return 2;
        const long long len = rows >= 0 && cols >= 0 ? 3ll * (rows + 1) * (cols + 1) : 0;
        std::vector<int16_t> x((size_t)len); // exactly the row: the sanitizer sees any read past it
        for (long long k = 0; k < len; k++) {
            int v = 0;
            if (scanf("%d", &v) != 1) return 2;
            x[(size_t)k] = (int16_t)v;
        }
        PositionGeo p;
        const int rc = position_geometry(rows, cols, x.data(), p);
        printf("%d %d %llu %llu %llu %llu", rc, p.F, (unsigned long long)p.free_edges[0], (unsigned long long)p.free_edges[1],
               (unsigned long long)p.free_edges[2], (unsigned long long)p.free_edges[3]);
        for (int j = 0; rc == 0 && j < p.F; j++) printf(" %d %u %u", (int)p.act[j], p.other[j][0], p.other[j][1]);
        printf("\n");
    }
    return 0;
}
