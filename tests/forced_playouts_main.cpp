// forced_playouts_main.cpp -- the pruning rule (csrc/forced_playouts.h) on the host: reads roots
//   "A k pbc sq root_N" then A times "P W n_and_sign valid"   (doubles and the float as C99 hexadecimal floats)
// and writes per root one line: the A pruned visit counts, then per child "forced f" of the descent's test and of forced_count.
// Built by tests/test_forced_playouts_ref_cpu.py with g++ for the host only, under AddressSanitizer and UBSan.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "forced_playouts.h"

int main()
{
    int A;
    char ks[64], ps[64], ss[64];
    long long N;
    while (scanf("%d %63s %63s %63s %lld", &A, ks, ps, ss, &N) == 5) {
        if (A < 1 || A > 256) return 2;
        const double k = strtod(ks, nullptr), pbc = strtod(ps, nullptr), sq = strtod(ss, nullptr);
        std::vector<double> P(A);
        std::vector<float> W(A);
        std::vector<uint32_t> ns(A);
        std::vector<uint8_t> valid(A);
        std::vector<int32_t> out(A);
        for (int i = 0; i < A; i++) {
            char a[64], b[64];
            unsigned n, v;
            if (scanf("%63s %63s %u %u", a, b, &n, &v) != 4) return 2;
            P[i] = strtod(a, nullptr);
            W[i] = strtof(b, nullptr);
            ns[i] = n;
            valid[i] = (uint8_t)v;
        }
        forced_prune_row(A, k, pbc, sq, N, P.data(), W.data(), ns.data(), valid.data(), out.data());
        for (int i = 0; i < A; i++) printf("%d ", out[i]);
        for (int i = 0; i < A; i++)
            printf("%d %lld ", forced_child(k, P[i], (int)(ns[i] & FORCED_VISITS_MASK), N) ? 1 : 0, forced_count(k, P[i], N));
        printf("\n");
    }
    return 0;
}
