// Exhaustive check of the tower's (hi, lo) split (csrc/h3_split.h): every one of the 2^32 bit patterns of an f32 goes through
// the shipped h3_split and through the reference spelling h3_split_ref, in the position that the v_fma_mixlo_f16 handles and in
// the one that the v_fma_mixhi_f16 handles.  An input counts as a mismatch when a hi or a lo half differs; two NaNs are equal
// whatever their payloads.  The class counts (taken from the reference's halves) show that the sweep visited values with a
// non-zero lo, with a subnormal lo and with an infinite hi.
// Stand-alone: built and started by tests/test_hip_h3_split.py; prints one line of "name value" pairs.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "h3_split.h"

#define BLOCKS 16384
#define THREADS 256
#define PER_THREAD (1u << 10) // BLOCKS * THREADS * PER_THREAD = 2^32

__device__ __forceinline__ bool h_nan(unsigned h) { return (h & 0x7c00u) == 0x7c00u && (h & 0x03ffu) != 0; }
__device__ __forceinline__ bool h_same(unsigned a, unsigned b) { return a == b || (h_nan(a) && h_nan(b)); }

// counts: 0 mismatches, 1 inputs with lo != 0, 2 with a subnormal lo, 3 with an infinite hi, 4 inputs visited
__global__ void __launch_bounds__(THREADS) k_sweep(unsigned long long *counts)
{
    const unsigned first = (blockIdx.x * THREADS + threadIdx.x) * PER_THREAD;
    unsigned bad = 0, nz = 0, sub = 0, inf = 0, seen = 0;
    for (unsigned i = 0; i < PER_THREAD; i++) {
        const unsigned bits = first + i;
        const float x = __uint_as_float(bits);
        const float y = __uint_as_float(bits ^ 0x80000000u); // over the sweep y visits every pattern as well
        // x in the mixlo position of pair 0 and in the mixhi position of pair 1, y in the other two
        const f32x4 v = {x, y, y, x};
        u32x2 hs, ls, hr, lr;
        h3_split(v, hs, ls);
        h3_split_ref(v, hr, lr);
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            ok = ok && h_same(hs[q] & 0xffffu, hr[q] & 0xffffu) && h_same(hs[q] >> 16, hr[q] >> 16);
            ok = ok && h_same(ls[q] & 0xffffu, lr[q] & 0xffffu) && h_same(ls[q] >> 16, lr[q] >> 16);
        }
        bad += ok ? 0 : 1;
        const unsigned h0 = hr[0] & 0xffffu, l0 = lr[0] & 0xffffu; // the reference's halves of x
        nz += !h_nan(l0) && (l0 & 0x7fffu) != 0;
        sub += (l0 & 0x7c00u) == 0 && (l0 & 0x03ffu) != 0;
        inf += (h0 & 0x7fffu) == 0x7c00u;
        seen++;
    }
    atomicAdd(&counts[0], (unsigned long long)bad);
    atomicAdd(&counts[1], (unsigned long long)nz);
    atomicAdd(&counts[2], (unsigned long long)sub);
    atomicAdd(&counts[3], (unsigned long long)inf);
    atomicAdd(&counts[4], (unsigned long long)seen);
}

#define CHECK(e)                                                                          \
    do {                                                                                  \
        hipError_t err_ = (e);                                                            \
        if (err_ != hipSuccess) {                                                         \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));                     \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)

int main()
{
    static_assert((unsigned long long)BLOCKS * THREADS * PER_THREAD == 1ull << 32, "the sweep is every pattern once");
    unsigned long long *d = nullptr, h[5] = {0, 0, 0, 0, 0};
    CHECK(hipMalloc(&d, sizeof(h)));
    CHECK(hipMemset(d, 0, sizeof(h)));
    hipLaunchKernelGGL(k_sweep, dim3(BLOCKS), dim3(THREADS), 0, 0, d);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    CHECK(hipFree(d));
    printf("mismatch %llu nonzero_lo %llu subnormal_lo %llu inf_hi %llu patterns %llu\n", h[0], h[1], h[2], h[3], h[4]);
    return 0;
}
