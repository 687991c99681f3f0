// gumbel_main.cpp -- the Gumbel root rule (csrc/gumbel.h) on the host: reads records
//   "C m_eff R"                 -> one line: considered(m_eff, R, t) for t = 0 .. R - 1
//   "T A c_visit c_scale" then A times "P W n_and_sign valid"   (doubles and the float as C99 hexadecimal floats)
//                               -> one line: the A visits of the row
// Built by tests/test_gumbel_ref_cpu.py with g++ for the host only, also under AddressSanitizer and UBSan.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gumbel.h"

int main()
{
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (kind[0] == 'C') {
            int m, R;
            if (scanf("%d %d", &m, &R) != 2 || R < 0 || R > 100000) return 2;
            for (int t = 0; t < R; t++) printf("%d ", gumbel_considered(m, R, t));
            printf("\n");
            continue;
        }
        int A;
        char cv[64], cs[64];
        if (kind[0] != 'T' || scanf("%d %63s %63s", &A, cv, cs) != 3 || A < 1 || A > GUMBEL_M_MAX) return 2;
        const double c_visit = strtod(cv, nullptr), c_scale = strtod(cs, nullptr);
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
        gumbel_target_row(A, c_visit, c_scale, P.data(), W.data(), ns.data(), valid.data(), out.data());
        for (int i = 0; i < A; i++) printf("%d ", out[i]);
        printf("\n");
    }
    return 0;
}
