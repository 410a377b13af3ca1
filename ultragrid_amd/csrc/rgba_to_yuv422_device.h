// rgba_to_yuv422_device.h -- dxt_compress/rgba_to_yuv422.glsl (the RGBA -> 4:2:2 pass of the reference's GL DXT decoder, and the
// fragment shader of src/video_compress/uyvy.cpp, whose text is the same) on pairs of 8-bit RGB texels, shared by the DXT decoder's UYVY
// outputs (dxt_decode.hip) and the RGB / RGBA -> UG_PF_UYVY_GL converter (uyvy_gl.hip).  Two forms of the same bytes:
//   rgb_pair_to_uyvy         the shader's own fp32 operations, in its order (-ffp-contract=off), texel fetch from the caller's table
//                            (DXT decoder: v / 255.0f; uyvy_gl.hip: v * (1.0f / 255.0f), llvmpipe's unorm8 -> float);
//   uyvy_pair_fixed[_packed] 32-bit fixed point, exact wherever no value lies within kGuardUyvy of a rounding boundary -- the caller runs
//                            rgb_pair_to_uyvy_call on the (rare) pairs it flags.
// Pinned to the shader as Mesa llvmpipe executes it (tests/golden/dxt_glsl_ref.npz, tests/golden/uyvy_glsl_ref.npz).
#ifndef UG_RGBA_TO_YUV422_DEVICE_H
#define UG_RGBA_TO_YUV422_DEVICE_H

#include "ug_common.h"

namespace {

// float -> unorm8 framebuffer write of the receiver's shaders.  GL rounds to nearest and leaves exact .5 ties to the implementation:
// AWAY = false (UG_DXT_TIES_EVEN, default): ties to even, what Mesa llvmpipe does when it executes the reference's rgba_to_yuv422.glsl
// (pinned byte for byte, tests/test_oracle_dxt.py); AWAY = true (UG_DXT_TIES_AWAY): floor(x * 255 + 0.5).
template <bool AWAY>
__device__ __forceinline__ uint8_t unorm8_out(float x)
{
        x = __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); // the clamp of the write (the values here are finite; -0 and +0 end as the same byte): one operation, not two compares and two selects
        return AWAY ? (uint8_t) (int) (x * 255.0f + 0.5f) : (uint8_t) (int) rintf(x * 255.0f);
}

// dxt_compress/rgba_to_yuv422.glsl:27-46 on two 8-bit RGB texels -> one UYVY word.  `unorm` = the 256 values v / 255.0f (the
// texel fetch), computed once per workgroup with the IEEE division and kept in LDS: a table read instead of six divisions per pair.
template <bool AWAY>
__device__ __forceinline__ uint32_t rgb_pair_to_uyvy(uint32_t p1, uint32_t p2, const float *unorm)
{
        float yuv[2][3];
#pragma unroll
        for (int i = 0; i < 2; i++) {
                const uint32_t p = i ? p2 : p1;
                const float r = unorm[p & 0xff], g = unorm[(p >> 8) & 0xff], b = unorm[(p >> 16) & 0xff];
                yuv[i][0] = (float) (1.0 / 16.0) + ((r * 0.2126f + g * 0.7152f) + b * 0.0722f) * 0.8588f;
                yuv[i][1] = 0.5f + ((-r * 0.1145f - g * 0.3854f) + b * 0.5f) * 0.8784f;
                yuv[i][2] = 0.5f + ((r * 0.5f - g * 0.4541f) - b * 0.0458f) * 0.8784f;
        }
        const float U = yuv[0][1] * 0.5f + yuv[1][1] * 0.5f, V = yuv[0][2] * 0.5f + yuv[1][2] * 0.5f;
        return (uint32_t) unorm8_out<AWAY>(U) | (uint32_t) unorm8_out<AWAY>(yuv[0][0]) << 8 | (uint32_t) unorm8_out<AWAY>(V) << 16 |
               (uint32_t) unorm8_out<AWAY>(yuv[1][0]) << 24;
}

// one copy of the shader arithmetic for the rare pairs the fixed-point form hands back (a call inside a divergent branch)
template <bool AWAY>
__device__ __noinline__ uint32_t rgb_pair_to_uyvy_call(uint32_t p1, uint32_t p2, const float *unorm) { return rgb_pair_to_uyvy<AWAY>(p1, p2, unorm); }

// rgba_to_yuv422.glsl:27-46 on two 8-bit RGB texels in 32-bit fixed point (2^-24 of a code value) (the DXT5-YCoCg decoder, the RGB / RGBA -> UYVY_GL converter).
// In exact arithmetic the shader's values are linear in the bytes (the v / 255 of the texel fetch cancels against the * 255 of the write):
//      Y'  = 15.9375 + cm (c1 R + c2 G + c3 B)                               cm = 0.8588f, c1..c3 = 0.2126f, 0.7152f, 0.0722f
//      Cb  = 127.5 + 0.5 cu (0.5 SB - c4 SR - c5 SG),  SR = R0 + R1 ...      cu = 0.8784f, c4, c5 = 0.1145f, 0.3854f
//      Cr  = 127.5 + 0.5 cu (0.5 SR - c6 SG - c7 SB)                         c6, c7 = 0.4541f, 0.0458f
// The shader's fp32 evaluation (rgb_pair_to_uyvy above) stays within 1.1e-4 of these (Y': six roundings of 2^-24 on partial sums
// <= 1, times 0.8588, one on the sum, times 255, one on the product; Cb / Cr: 1.04e-4 incl. the + 0.5f of the AWAY rule); the 24-bit
// coefficients below add <= 0.5 * 255 * 3 (Y') or 0.5 * 510 * 3 (Cb, Cr) units = 2.3e-5 / 4.6e-5.  Guard: kGuardUyvy = 3072 units = 1.83e-4
// on each side of a rounding boundary (x.5): outside it the rounded fixed-point value is the shader's byte whatever the tie rule; a pair
// with a value inside it is converted again by the shader's own operations.  All sums stay in [15.5, 240] * 2^24 < 2^32, unsigned.
// The budget assumes the correctly rounded texel fetch v / 255.0f (the DXT decoder's table).  uyvy_gl.hip's fallback table holds
// v * (1.0f / 255.0f), llvmpipe's form, which can be one ulp off the quotient: that moves a shader value by at most ~1.5e-5 code values,
// still inside the guard (1.1e-4 + 4.6e-5 + 1.5e-5 < 1.83e-4), so a pair outside the guard is the same byte under either table.
constexpr int kGuardUyvy = 3072;
constexpr double kCm = (double) 0.8588f, kCu = (double) 0.8784f, kTwo24 = 16777216.0;
constexpr uint32_t kYr = (uint32_t) (kCm * (double) 0.2126f * kTwo24 + 0.5), kYg = (uint32_t) (kCm * (double) 0.7152f * kTwo24 + 0.5),
                   kYb = (uint32_t) (kCm * (double) 0.0722f * kTwo24 + 0.5), kY0 = (uint32_t) (15.9375 * kTwo24) + (1u << 23) + kGuardUyvy;
constexpr uint32_t kUb = (uint32_t) (0.5 * kCu * 0.5 * kTwo24 + 0.5), kUr = (uint32_t) (0.5 * kCu * (double) 0.1145f * kTwo24 + 0.5),
                   kUg = (uint32_t) (0.5 * kCu * (double) 0.3854f * kTwo24 + 0.5);
constexpr uint32_t kVr = (uint32_t) (0.5 * kCu * 0.5 * kTwo24 + 0.5), kVg = (uint32_t) (0.5 * kCu * (double) 0.4541f * kTwo24 + 0.5),
                   kVb = (uint32_t) (0.5 * kCu * (double) 0.0458f * kTwo24 + 0.5);
constexpr uint32_t kC0 = (uint32_t) (127.5 * kTwo24) + (1u << 23) + kGuardUyvy;

// k * x (+ acc) on 24-bit operands as ONE instruction each, the constant from a scalar register.  Written out: left to itself the compiler turns
// "c - k * x" into a full 32-bit multiply by -k behind an AND that re-establishes the 24 bits (v_and + v_mul_lo_u32 + v_add for what
// v_mad_u32_u24 does) -- 12 instructions for the chroma of a pixel pair instead of 8.
#define UG_MUL24(dst, k, x) asm("v_mul_u32_u24 %0, %1, %2" : "=v"(dst) : "s"(k), "v"(x))
#define UG_MAD24(dst, k, x, acc) asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(dst) : "s"(k), "v"(x), "v"(acc))
// Cb / Cr of a pixel pair from the channel sums (0 .. 510): (kA * sa + kC0) - (kB * sb + kC * sc), all modulo 2^32
__device__ __forceinline__ uint32_t chroma_fixed(uint32_t ka, uint32_t sa, uint32_t kb, uint32_t sb, uint32_t kc, uint32_t sc)
{
        uint32_t neg, pos;
        UG_MUL24(neg, kb, sb);
        UG_MAD24(neg, kc, sc, neg);
        UG_MAD24(pos, ka, sa, kC0);
        return pos - neg;
}

// returns the UYVY word as the fixed-point values round; `near` = the smallest distance (in 2^-24 units, biased by the guard) of the four
// values from a rounding boundary: < 2 * kGuardUyvy means the word must not be trusted
__device__ __forceinline__ uint32_t uyvy_pair_fixed(uint32_t r0, uint32_t g0, uint32_t b0, uint32_t r1, uint32_t g1, uint32_t b1, uint32_t &near)
{
        const uint32_t y0 = __umul24(kYr, r0) + (__umul24(kYg, g0) + (__umul24(kYb, b0) + kY0));
        const uint32_t y1 = __umul24(kYr, r1) + (__umul24(kYg, g1) + (__umul24(kYb, b1) + kY0));
        const uint32_t sr = r0 + r1, sg = g0 + g1, sb = b0 + b1;
        const uint32_t u = chroma_fixed(kUb, sb, kUr, sr, kUg, sg);
        const uint32_t v = chroma_fixed(kVr, sr, kVg, sg, kVb, sb);
        const uint32_t m = 0xFFFFFFu;
        near = min(min(y0 & m, y1 & m), min(u & m, v & m));
        // the integer parts are the top bytes: U | Y0 << 8 | V << 16 | Y1 << 24
        return __builtin_amdgcn_perm(y0, u, 0x0c0c0703u) | __builtin_amdgcn_perm(y1, v, 0x07030c0cu);
}

// The same on PACKED bytes (what V_ASHR_PK_U8_I32 leaves): d0 = R0 | G0 << 8 | B0 << 16 | R1 << 24, d1 = G1 | B1 << 8 | (anything) << 16.
// SDWA operand selects read the bytes in place: a 24-bit multiply or an add takes its 8-bit operand straight out of the packed word.
#define UG_MUL24_BYTE(dst, k, packed, n) asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #n : "=v"(dst) : "v"(k), "v"(packed))
#define UG_ADD_BYTES(dst, a, i, b, j) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_" #i " src1_sel:BYTE_" #j : "=v"(dst) : "v"(a), "v"(b))
__device__ __forceinline__ uint32_t uyvy_pair_fixed_packed(uint32_t d0, uint32_t d1, uint32_t &near)
{
        const uint32_t cyr = kYr, cyg = kYg, cyb = kYb; // in registers: SDWA takes no literal
        uint32_t a0, a1, a2, b0, b1, b2, sr, sg, sb;
        UG_MUL24_BYTE(a0, cyr, d0, 0); UG_MUL24_BYTE(a1, cyg, d0, 1); UG_MUL24_BYTE(a2, cyb, d0, 2);
        UG_MUL24_BYTE(b0, cyr, d0, 3); UG_MUL24_BYTE(b1, cyg, d1, 0); UG_MUL24_BYTE(b2, cyb, d1, 1);
        UG_ADD_BYTES(sr, d0, 0, d0, 3); UG_ADD_BYTES(sg, d0, 1, d1, 0); UG_ADD_BYTES(sb, d0, 2, d1, 1);
        const uint32_t y0 = (a0 + a1) + (a2 + kY0), y1 = (b0 + b1) + (b2 + kY0);
        const uint32_t u = chroma_fixed(kUb, sb, kUr, sr, kUg, sg);
        const uint32_t v = chroma_fixed(kVr, sr, kVg, sg, kVb, sb);
        const uint32_t m = 0xFFFFFFu;
        near = min(min(y0 & m, y1 & m), min(u & m, v & m));
        return __builtin_amdgcn_perm(y0, u, 0x0c0c0703u) | __builtin_amdgcn_perm(y1, v, 0x07030c0cu);
}

} // namespace

#endif
