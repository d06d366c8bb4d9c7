// The exact three-term bf16 split of an fp32 value (x = hi + mid + lo), shared by the split-bf16 main loops
// (gemm_x6.hip, attention_x6.hip).
#pragma once
#include "common.h"

namespace mi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// (x0, x1) -> packed bf16 pairs of the three terms; x == hi + mid + lo exactly (each residual is representable).  Each term
// is rounded once, as a pair (v_cvt_pk_bf16_f32), and read back out of the packed word (a bf16 is the top half of its fp32).
__device__ __forceinline__ void split3(float x0, float x1, unsigned &h, unsigned &m, unsigned &l) {
    h = __builtin_bit_cast(unsigned, bf16x2{(__bf16)x0, (__bf16)x1});
    asm("" : "+v"(h));       // opaque: otherwise hipcc rounds x0 a second time, alone, to rebuild h << 16
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = __builtin_bit_cast(unsigned, bf16x2{(__bf16)r0, (__bf16)r1});
    asm("" : "+v"(m));
    const float q0 = r0 - __builtin_bit_cast(float, m << 16), q1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
    l = __builtin_bit_cast(unsigned, bf16x2{(__bf16)q0, (__bf16)q1});
}

}  // namespace mi
