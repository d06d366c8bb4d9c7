// Multi-head attention core  O = softmax(Q^T K / 8) V  of the float32 engine on the bf16 matrix pipe, with every fp32
// operand carried as three exact bf16 terms and six bf16 MFMA products per multiply-accumulate (the contract of the
// split linears, gemm_x6.hip: dropped terms <= 2^-24 |a b|, fp32 accumulation).
//
// Stands in for the attention inside nn.MultiheadAttention as called by the reference
// (demucs/transformer.py:418-419,506; 8 heads x 64, no mask, eval mode), like attention_kernel (attention.hip), whose
// structure it keeps: workgroup = 4 waves x 32 queries; per 32-key sub-tile a wave computes the TRANSPOSED score tile
// S^T[key][query] = K^T Q (keys on MFMA rows, queries on lanes), runs the online softmax on the accumulator registers, and
// feeds them as the B operand of O^T[d][query] += V[d][key] P^T[key][query] with no LDS round trip.
//
// v_mfma_f32_32x32x16_bf16 operand fragments: lane (li, lh) holds row / column li and k = 8 lh .. 8 lh + 7.
//   S^T: k = d.  A = K^T from the LDS image Kx[part][g][key][8] (d = 8 g + j, g = 2 t + lh for k step t);
//        B = Q / 8 (exact: power of two), split once per wave into qx[t][part].
//   O^T: k = key.  Registers 8 m .. 8 m + 7 of a lane are the keys (j & 3) + 8 (j >> 2) + 4 lh of the 16-key step m (the
//        accumulator row map), so V's LDS image Vx[part][2 ms + lh][d][8] holds exactly those keys in that order.
// Both images are [part 3][8][64][16 bytes]: one conflict-free ds_read_b128 per fragment term.  K and V are split once per
// tile by the threads that stage them (global -> registers during the previous tile -> three bf16 planes in LDS).
//
// ONLINE SOFTMAX WITH A THRESHOLDED RESCALE.  Each query keeps a reference max mref and p = exp(s - mref); mref follows the
// query's sub-tile max only when that passes it by more than TAU, so p <= e^TAU and the rescale of the 32 O^T accumulator
// registers (an AGPR read, a multiply and an AGPR write each) leaves the hot path: a wave enters the block when any of its
// queries moves, and there each query multiplies by its own factor, exactly 1 if it does not move, so a query's bits do not
// depend on the other 31.
//
// ACCUMULATORS IN AGPRs (see gemm_x6.hip): built with -amdgpu-mfma-vgpr-form=0 and the inline-asm anchor below.
// REGISTERS.  hipcc splits the file 128 / 128 at two waves per SIMD.  The empty asm anchors in the key loop pin O^T to AGPRs
// outside the rescale block and the split Q fragments to VGPRs at the head of every sub-tile; without them hipcc carries O^T
// through the loop in VGPRs and copies Q out of AGPRs before every score product.  The staged K tile then lands in AGPRs
// straight from the loads.  Built with -fno-slp-vectorize (Makefile): packed fp32 adds beside MFMAs cost more than the two
// scalar ones they replace, and the scalar form frees the register pairs that kept part of Q parked.  DESIGN.md section 8
// has the instruction counts.
#include "common.h"
#include "kernels.h"
#include "split_bf16.h"

namespace mi {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) char gchar;      // global-memory pointers that stay global through an asm anchor
typedef __attribute__((address_space(1))) float gfloat;
constexpr int HD = 64;       // head dim
constexpr int KT = 64;       // keys per LDS tile
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float TAU = 8.0f;   // the reference max of the online softmax follows a query's max only past this distance

__device__ __forceinline__ f32x16 mfma6(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x16 acc) {
    // the six products, smallest terms first (gemm_x6.hip's PA / PB order)
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[PA[q]]), __builtin_bit_cast(bf16x8, b[PB[q]]), acc, 0,
                                                      0, 0);
    return acc;
}

// 8 fp32 values -> the three bf16x8 terms
__device__ __forceinline__ void split8(const float (&x)[8], u32x4 (&out)[3]) {
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split3(x[2 * j], x[2 * j + 1], h[j], m[j], l[j]);
    out[0] = u32x4{h[0], h[1], h[2], h[3]};
    out[1] = u32x4{m[0], m[1], m[2], m[3]};
    out[2] = u32x4{l[0], l[1], l[2], l[3]};
}

}  // namespace

// Two workgroups per CU (128 VGPRs + 70 AGPRs, no scratch); at three (168 registers) hipcc spills to scratch.
__global__ __launch_bounds__(256, 2) void attention_x6_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                              const float *__restrict__ v, float *__restrict__ o, int Tq, int Tk,
                                                              int64_t q_bs, int64_t kv_bs, int64_t o_bs, int planes, int heads) {
    __shared__ u32x4 Kx[3 * 8 * KT];     // [part][g][key]: K[d = 8 g + j][key], j = 0..7
    __shared__ u32x4 Vx[3 * 8 * HD];     // [part][2 ms + h][d]: V[d][16 ms + 4 h + (j & 3) + 8 (j >> 2)], j = 0..7
    {   // keeps the MFMA accumulators in AGPRs (gemm_x6.hip note)
        float agpr_anchor = 0.f;
        asm volatile("; accumulators in AGPRs %0" : "+a"(agpr_anchor));
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    // XCD-aware plane order, as attention_kernel
    const int nqb = (Tq + 127) / 128;
    const int xj = blockIdx.x >> 3;
    const int pl = (xj / nqb) * 8 + (blockIdx.x & 7);
    if (pl >= planes) return;                  // grid padding (whole workgroup, before any barrier)
    const int head = pl % heads, b = pl / heads;
    const int q0 = (xj % nqb) * 128 + wave * 32;
    const float *qp = q + (size_t)b * q_bs + (size_t)head * HD * Tq;
    const float *kp = k + (size_t)b * kv_bs + (size_t)head * HD * Tk;
    const float *vp = v + (size_t)b * kv_bs + (size_t)head * HD * Tk;

    // Q fragments (B operand of S^T = K^T Q): lane (query li, half lh) holds Q[d = 16 t + 8 lh + j][q0 + li] / 8
    const int qi = q0 + li;
    const bool qok = qi < Tq;
    const int qic = qok ? qi : Tq - 1;        // loads stay in bounds and unconditional (no branch per load); the value is dropped
    u32x4 qx[4][3];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float qv = qp[(size_t)(16 * t + 8 * lh + j) * Tq + qic];
            x[j] = qok ? qv * 0.125f : 0.f;
        }
        split8(x, qx[t]);
    }

    f32x16 oacc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc[0][r] = 0.f; oacc[1][r] = 0.f; }
    // reference max (both halves agree), -mref log2(e) as the exponent's addend, and this half's partial sum
    float mref = -INFINITY, nml2 = INFINITY, lrun = 0.f;

    // global -> register staging of the next K / V tile.  K: key k0 + lane, rows 8 g .. 8 g + 7 for g = wave, wave + 4 (coalesced
    // dwords; the image writes are consecutive 16-byte words).  V: rows d = (lane & 7) + 8 wave + 32 i, keys 16 ms + 4 h + {0..3, 8..11}
    // for (ms, h) = lane >> 3 (each 8-lane group writes 128 consecutive bytes of the image).
    const int ve = lane >> 3, vd = (lane & 7) + 8 * wave, vc = 16 * (ve >> 1) + 4 * (ve & 1);
    float kst[2][8];
    float4 vst[2][2];
    // Keys past Tk (ragged last tile) load from a clamped in-bounds address and are replaced by 0: no branch per load.
    // Every load is a wave-uniform row base plus one 32-bit byte offset per lane (launch_attention_x6 keeps 4 HD Tk under 2^32).
    // The K row bases are opaque scalars: hipcc otherwise folds them into sixteen 64-bit vector addresses per tile.
    const gchar *krow[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            krow[i][j] = (const gchar *)(kp + (size_t)(8 * (wave + 4 * i) + j) * Tk);
            asm("" : "+s"(krow[i][j]));
        }
    auto stage_load = [&](int k0) {
        const bool kok = k0 + lane < Tk;
        const unsigned kc = 4u * (unsigned)(kok ? k0 + lane : Tk - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) kst[i][j] = *(const gfloat *)(krow[i][j] + kc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int key = k0 + vc + 8 * c;          // Tk % 4 == 0: the 4 keys are all in range or all out
                const unsigned vo = 4u * ((unsigned)((lane & 7) * Tk) + (unsigned)(key < Tk ? key : Tk - 4));
                vst[i][c] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(vp + (size_t)(8 * wave + 32 * i) * Tk) + vo);
            }
    };
    // the zeroing of out-of-range keys happens here, after the loads have landed
    auto stage_mask = [&](int k0) {
        if (k0 + KT <= Tk) return;                   // (uniform) full tile
        if (k0 + lane >= Tk) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) kst[i][j] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (k0 + vc + 8 * c >= Tk)
#pragma unroll
                for (int i = 0; i < 2; ++i) vst[i][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x4 t[3];
            split8(kst[i], t);
#pragma unroll
            for (int p = 0; p < 3; ++p) Kx[(p * 8 + wave + 4 * i) * KT + lane] = t[p];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float x[8] = {vst[i][0].x, vst[i][0].y, vst[i][0].z, vst[i][0].w, vst[i][1].x, vst[i][1].y, vst[i][1].z, vst[i][1].w};
            u32x4 t[3];
            split8(x, t);
#pragma unroll
            for (int p = 0; p < 3; ++p) Vx[(p * 8 + ve) * HD + vd + 32 * i] = t[p];
        }
    };

    stage_load(0);
    for (int k0 = 0; k0 < Tk; k0 += KT) {
        asm volatile("" : "+a"(oacc[0]), "+a"(oacc[1]));
        __syncthreads();                     // previous tile fully consumed
        stage_mask(k0);
        stage_store();
        __syncthreads();
        if (k0 + KT < Tk) stage_load(k0 + KT);   // in flight under this tile's MFMAs
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int kb = sub * 32;
            if (k0 + kb >= Tk) break;            // (wave-uniform) a ragged last tile with no key in this sub-tile
            asm volatile("" : "+a"(oacc[0]), "+a"(oacc[1]));     // register anchors: see the header
#pragma unroll
            for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(qx[t][0]), "+v"(qx[t][1]), "+v"(qx[t][2]));
            // S^T[key][query]: 4 k steps of 16 d
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                u32x4 kf[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) kf[p] = Kx[(p * 8 + 2 * t + lh) * KT + kb + li];
                sacc = mfma6(kf, qx[t], sacc);
            }
            // register r of lane (li, lh) is key kb + (r&3) + 8(r>>2) + 4 lh, query li
            float s[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = sacc[r];
            float mloc = -INFINITY;
            if (k0 + kb + 32 > Tk) {             // ragged last tile only (wave-uniform): mask keys past Tk
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (k0 + kb + (r & 3) + 8 * (r >> 2) + 4 * lh >= Tk) s[r] = -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[r]);
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
            // Thresholded rescale: p = exp(s - mref) against a reference max that moves only when a query's sub-tile max passes it
            // by more than TAU (p <= e^TAU, lrun <= Tk e^TAU).  Each query decides for itself; the others multiply by exactly 1.
            if (k0 + kb == 0) {                  // first sub-tile: the accumulators are still zero, nothing to rescale
                mref = mloc;
                nml2 = -(mloc * LOG2E);
            }
            if (__any(mloc > mref + TAU)) {
                const bool up = mloc > mref + TAU;
                const float nnew = -(mloc * LOG2E);
                const float alpha = up ? __builtin_amdgcn_exp2f(nnew - nml2) : 1.0f;       // exp(mref - mloc), in the addends' rounding
                mref = up ? mloc : mref;
                nml2 = up ? nnew : nml2;
                lrun *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) { oacc[0][r] *= alpha; oacc[1][r] *= alpha; }
            }
            asm volatile("" : "+a"(oacc[0]), "+a"(oacc[1]));     // O^T stays in AGPRs outside the rescale block
            // exp(s - mref) as v_exp_f32 of one fused multiply-add (the rounding of nml2 is common to a query's keys and cancels in
            // the normalisation); masked keys give exp(-inf) = 0
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], LOG2E, nml2));
                s[r] = p;
                psum += p;
            }
            lrun += psum;
            // O^T[d][query] += V[d][key] P^T[key][query]: 2 k steps of 16 keys (registers 8 m .. 8 m + 7) x 2 d tiles
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = s[8 * m + j];
                u32x4 px[3];
                split8(x, px);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    u32x4 vf[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) vf[p] = Vx[(p * 8 + 2 * (2 * sub + m) + lh) * HD + dt * 32 + li];
                    oacc[dt] = mfma6(vf, px, oacc[dt]);
                }
            }
        }
    }
    const float ltot = lrun + __shfl_xor(lrun, 32);
    const float inv = 1.0f / ltot;
    if (qok) {
        float *op = o + (size_t)b * o_bs + (size_t)head * HD * Tq + qi;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dd = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                op[(size_t)dd * Tq] = oacc[dt][r] * inv;
            }
    }
}

int launch_attention_x6(const float *q, const float *k, const float *v, float *o, int B, int heads, int Tq, int Tk, int64_t q_bs,
                        int64_t kv_bs, int64_t o_bs, hipStream_t st) {
    MI_REQUIRE(Tk % 4 == 0, "attention x6: Tk %% 4 != 0 (%d)", Tk);
    MI_REQUIRE(Tk < (1 << 24), "attention x6: Tk %d too long for 32-bit staging offsets", Tk);
    MI_REQUIRE(((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && kv_bs % 4 == 0, "attention x6: k/v must be 16-byte aligned");
    const int planes = B * heads;
    hipLaunchKernelGGL(attention_x6_kernel, dim3((unsigned)(ceil_div(Tq, 128) * ((planes + 7) / 8) * 8)), dim3(256), 0, st, q, k, v, o,
                       Tq, Tk, q_bs, kv_bs, o_bs, planes, heads);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
