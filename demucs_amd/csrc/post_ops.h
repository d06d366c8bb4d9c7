// Per-sample arithmetic of the stem post-processing, shared by post.hip (mi_prevent_clip, mi_two_stems: one output per call),
// deliver.hip (mi_deliver_peaks / mi_deliver_pcm: every output of a call in one launch), deliver_mix.hip (the same for
// gain-weighted remixes) and deliver_mix_auto.hip (remixes whose gains change along the track), so all routes run the same float32
// sequence.  Every step is a separately rounded operation (the
// library builds with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

namespace mi {

// "add" of `--two-stems` (demucs/separate.py:207-210): zeros_like, then += every stem but `sel` in index order, for W samples
// side by side.  stem(k, s) fills s[0 .. W-1] with stem k's samples
template <int W, class Stem>
__device__ __forceinline__ void two_stems_add(int S, int sel, Stem stem, float (&a)[W]) {
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] = 0.f;
    for (int k = 0; k < S; ++k) {
        if (k == sel) continue;
        float s[W];
        stem(k, s);
#pragma unroll
        for (int e = 0; e < W; ++e) a[e] = __fadd_rn(a[e], s[e]);
    }
}

// "minus" (separate.py:197): origin - stem
__device__ __forceinline__ float two_stems_minus(float origin, float stem) { return __fsub_rn(origin, stem); }

// A gain-weighted remix of the mix and the stems, what a user of the reference writes as `sum(g * x for ...)` after
// `separate_tensor`: acc = 0; if g_mix != 0: acc = acc + g_mix * o; for k ascending, if g_k != 0: acc = acc + g_k * s_k -- every
// product and every sum a separately rounded float32 operation.  A term whose gain is 0 is NOT READ, so a NaN or Inf in a muted
// stem never reaches the output.  gain(0) is the mix's, gain(1 + k) stem k's; origin(s) / stem(k, s) fill s[0 .. W-1]
template <int W, class Gain, class Origin, class Stem>
__device__ __forceinline__ void mix_values(int S, Gain gain, Origin origin, Stem stem, float (&a)[W]) {
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] = 0.f;
    const float g_mix = gain(0);
    if (g_mix != 0.f) {
        float s[W];
        origin(s);
#pragma unroll
        for (int e = 0; e < W; ++e) a[e] = __fadd_rn(a[e], __fmul_rn(g_mix, s[e]));
    }
    for (int k = 0; k < S; ++k) {
        const float g = gain(1 + k);
        if (g == 0.f) continue;
        float s[W];
        stem(k, s);
#pragma unroll
        for (int e = 0; e < W; ++e) a[e] = __fadd_rn(a[e], __fmul_rn(g, s[e]));
    }
}

// mix_values with a gain per ELEMENT (deliver_mix_auto.hip: gains that change along the track).  gain(i, g) fills the W gains of
// term i (0: the mix, 1 + k: stem k).  Element e of a term is added only where g[e] != 0, so a NaN in a stem stays out of exactly
// the samples at which the stem is muted; a term whose W gains are all 0 is not loaded at all.  With W equal gains per term this is
// mix_values' sequence, operation for operation
template <int W, class Gain, class Origin, class Stem>
__device__ __forceinline__ void mix_values_each(int S, Gain gain, Origin origin, Stem stem, float (&a)[W]) {
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] = 0.f;
    for (int i = 0; i <= S; ++i) {
        float g[W];
        gain(i, g);
        bool any = false;
#pragma unroll
        for (int e = 0; e < W; ++e) any = any || g[e] != 0.f;
        if (!any) continue;
        float s[W];
        if (i == 0) origin(s);
        else stem(i - 1, s);
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (g[e] != 0.f) a[e] = __fadd_rn(a[e], __fmul_rn(g[e], s[e]));
    }
}

// the Separator's inverse affine on a normalised sample (track_affine_kernel mode 1, api._restore_on_device): w * s, then + mean
__device__ __forceinline__ float restore_sample(float w, float mean, float s) { return __fadd_rn(__fmul_rn(w, s), mean); }

// the divisor of "rescale" from the peak's bit pattern: 1.01 * wav.abs().max() (demucs/audio.py:226)
__device__ __forceinline__ float clip_divisor(unsigned peak_bits) { return __fmul_rn(__uint_as_float(peak_bits), 1.01f); }

// mode 1 "rescale": v / max(d, 1); 2 "clamp": clamp(v, -0.99, 0.99); 3 "tanh"; anything else: v   (audio.py:225-231)
__device__ __forceinline__ float clip_sample(float v, int mode, float d) {
    if (mode == 1) return (d > 1.0f || d != d) ? __fdiv_rn(v, d) : v;   // a NaN peak divides everything (python's max(nan_tensor, 1) keeps the NaN)
    if (mode == 2) return v != v ? v : fminf(fmaxf(v, -0.99f), 0.99f);   // torch's clamp keeps a NaN; fmaxf / fminf alone would drop it
    if (mode == 3) return tanhf(v);
    return v;
}

// the unsigned bit pattern of |v|: unsigned order == float order for non-negative floats, and |NaN| orders above +inf, so a max
// over these reaches the peak as torch's abs().max() propagates a NaN
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(fabsf(v)); }

// `i16_pcm` (audio.py:178): (wav.clamp_(-1, 1) * (2**15 - 1)).short(); the conversion truncates toward zero.  A NaN passes the
// clamp and the product; C leaves its conversion undefined, torch on x86 gives 0: that is the rule here
__device__ __forceinline__ short pcm_i16(float v) {
    if (v != v) return 0;
    return (short)(int)__fmul_rn(fminf(fmaxf(v, -1.0f), 1.0f), 32767.0f);
}

}  // namespace mi
