// The (hi, lo) split of the f16x3 tower: an activation x (f32, activation-scaled) is kept as two halves,
//   hi = rn_f16(x), lo = rn_f16(x - hi),
// which every f16x3 body writes through h3_store (nn.hip): the two-cout-tile body with h3_split, the others with h3_split_ref.
// Device code only; included by nn.hip and by the exhaustive sweep tests/h3_split_sweep.hip, which compares the two spellings
// on every f32 bit pattern -- a sample's bits do not depend on the body that evaluated it.
#pragma once

#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// The spelling the tower shipped with, and the reference of the sweep: the hi pair is widened again, subtracted in f32 and
// rounded a second time (v_cvt_pk_f16_f32, 2 v_cvt_f32_f16, v_pk_add_f32, v_cvt_pk_f16_f32 per pair).
__device__ __forceinline__ void h3_split_ref(f32x4 v, u32x2 &hi, u32x2 &lo)
{
    union { f16x2 h[2]; u32x2 u; } oh, ol;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const f32x2 x = {v[2 * q], v[2 * q + 1]};
        const f16x2 h = __builtin_convertvector(x, f16x2);
        oh.h[q] = h;
        ol.h[q] = __builtin_convertvector(x - __builtin_convertvector(h, f32x2), f16x2);
    }
    hi = oh.u;
    lo = ol.u;
}

// The shipped split.  hi as above; lo by one v_fma_mixlo_f16 / v_fma_mixhi_f16 per value: x * 1.0 + (-hi) with hi taken straight
// from its f16 half (op_sel_hi of source 2), evaluated in f32 and rounded once to f16.  x - hi is exact in f32 (it is a
// multiple of x's f32 ulp below half an f16 ulp of x), so this is the same number as the reference's; NaNs may differ in payload.
// hipcc does not form the mix instructions from the C++ spelling.  The packed result feeds ds_write only: no VALU reads the
// half-written register behind the mixhi.
__device__ __forceinline__ void h3_split(f32x4 v, u32x2 &hi, u32x2 &lo)
{
    union { f16x2 h[2]; u32x2 u; } oh;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const f32x2 x = {v[2 * q], v[2 * q + 1]};
        oh.h[q] = __builtin_convertvector(x, f16x2);
        unsigned int l;
        asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(l) : "v"(x[0]), "v"(oh.u[q]));
        asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x[1]), "v"(oh.u[q]));
        lo[q] = l;
    }
    hi = oh.u;
}
