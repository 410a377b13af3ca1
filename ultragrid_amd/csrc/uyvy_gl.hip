// uyvy_gl.hip -- RGB / RGBA -> UG_PF_UYVY_GL: the conversion of `-c uyvy` (src/video_compress/uyvy.cpp), on gfx950.
//
// The reference draws a w/2 x h quad with dxt_compress/rgba_to_yuv422.glsl's text (fp_display_rgba_to_yuv422_legacy, uyvy.cpp:51-95)
// over the frame uploaded as a GL_NEAREST / CLAMP_TO_EDGE texture (uyvy.cpp:184-198) and reads the framebuffer back (uyvy.cpp:211-262).
// Fragment i of line y samples TEXCOORD -+ 1 / (2 imageWidth): the centres of pixels 2i and 2i + 1 of line y (row 0 stays row 0, quad and
// glReadPixels alike), and writes vec4(U, Y(2i), V, Y(2i + 1)) through float -> unorm8.  The arithmetic is rgba_to_yuv422_device.h's,
// shared with the DXT decoder's UYVY outputs and pinned to the shader as llvmpipe executes it (tests/golden/uyvy_glsl_ref.npz).
// Not reproduced (deviations): RGB lines read at GL's default 4-byte unpack alignment, and the w/2 x h texture of odd
// widths -- lines are read at the caller's pitch, and the last pair of an odd width repeats the last pixel (what CLAMP_TO_EDGE gives).
//
// Streaming kernel: 3 or 4 bytes in and 2 out per pixel.  A lane's unit is a quad of 4 pixels = 2 output pairs: 12 B (RGB, three dwords)
// or 16 B (RGBA, one dwordx4) in, 8 B out; the lanes of a wave take consecutive quads, so every load and store instruction of a wave
// covers one contiguous run of memory (768 / 1024 B in, 512 B out).  Each lane holds Q quads, Q * 256 quads apart, all loads issued
// before the arithmetic.  Per pair the fixed-point form costs ~30 VALU operations (about 2.5 per byte moved); the shader's fp32 form runs
// for the ~0.15 % of pairs with a value within the guard of a rounding boundary.  Lines that are not aligned for the wide accesses, and the
// last partial quad of a line, go through the pair-at-a-time path (byte loads, clamped second pixel).
#include "ug_common.h"
#include "rgba_to_yuv422_device.h"

namespace {

constexpr int kBlock = 256;

// the texel-fetch table of the fp32 fallback: v * (1.0f / 255.0f), llvmpipe's unorm8 -> float (it differs from v / 255.0f by one ulp for
// some v; executed on fp32 ties of Y', only the product form gives the shader's bytes -- tests/golden/uyvy_glsl_ref.npz "ties")
__device__ __forceinline__ void fill_unorm_table(float *unorm)
{
        unorm[threadIdx.x] = (float) threadIdx.x * (1.0f / 255.0f);
        __syncthreads();
}

// d0 = R0 | G0 << 8 | B0 << 16 | R1 << 24, d1 = G1 | B1 << 8 | (anything): the pair's UYVY word
__device__ __forceinline__ uint32_t pair_word(uint32_t d0, uint32_t d1, const float *unorm)
{
        uint32_t near;
        const uint32_t w = uyvy_pair_fixed_packed(d0, d1, near);
        if (near < 2u * kGuardUyvy) return rgb_pair_to_uyvy_call<false>(d0 & 0xFFFFFFu, d0 >> 24 | (d1 & 0xFFFFu) << 8, unorm);
        return w;
}

// pixel x of a line as R | G << 8 | B << 16, byte loads
template <int BPP>
__device__ __forceinline__ uint32_t load_px(const uint8_t *s, int x)
{
        const uint8_t *p = s + (long) BPP * x;
        return (uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16;
}

// pairs 2q and 2q + 1 of a line, one at a time: any alignment, any width (the second pixel of the last pair of an odd width is the last pixel)
template <int BPP, bool DST_ALIGNED>
__device__ __forceinline__ void quad_slow(const uint8_t *s, uint8_t *d, int q, int width, const float *unorm)
{
        const int pairs = (width + 1) / 2;
#pragma unroll
        for (int t = 0; t < 2; t++) {
                const int j = 2 * q + t;
                if (j >= pairs) break;
                const uint32_t p1 = load_px<BPP>(s, 2 * j), p2 = load_px<BPP>(s, min(2 * j + 1, width - 1));
                const uint32_t w = pair_word(p1 | p2 << 24, p2 >> 8, unorm);
                if (DST_ALIGNED) {
                        ug::st_stream((uint32_t *) (d + 4L * j), w);
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) d[4L * j + b] = (uint8_t) (w >> (8 * b));
                }
        }
}

// FAST: src line start 16-B (RGBA) / 4-B (RGB) aligned, dst line start 8-B aligned
template <int BPP, int Q, bool FAST>
__global__ __launch_bounds__(kBlock) void rgb_to_uyvy_gl_kernel(const uint8_t *__restrict__ src, long spitch, uint8_t *__restrict__ dst,
                                                                long dpitch, int width, int height)
{
        __shared__ float unorm[256];
        fill_unorm_table(unorm);
        const int quads = (width + 3) / 4, full_quads = width / 4;
        const int q0 = blockIdx.x * (kBlock * Q) + threadIdx.x;
        for (int line = blockIdx.y; line < height; line += gridDim.y) {
                const uint8_t *s = src + (long) line * spitch;
                uint8_t *d = dst + (long) line * dpitch;
                if constexpr (FAST) {
                        uint32_t w[Q][BPP];
#pragma unroll
                        for (int k = 0; k < Q; k++) {
                                const int q = q0 + k * kBlock;
                                if (q < full_quads) {
                                        // plain loads: one unit of consecutive memory per lane (ug_common.h, ld_stream)
                                        if constexpr (BPP == 4) {
                                                const uint4 v = ((const uint4 *) s)[q];
                                                w[k][0] = v.x; w[k][1] = v.y; w[k][2] = v.z; w[k][3] = v.w;
                                        } else {
                                                const uint32_t *p = (const uint32_t *) s + 3 * q;
                                                w[k][0] = p[0]; w[k][1] = p[1]; w[k][2] = p[2];
                                        }
                                }
                        }
#pragma unroll
                        for (int k = 0; k < Q; k++) {
                                const int q = q0 + k * kBlock;
                                if (q < full_quads) {
                                        uint32_t a, b;
                                        if constexpr (BPP == 4) { // pixels w0..w3 = R | G << 8 | B << 16 | A << 24
                                                a = pair_word(__builtin_amdgcn_perm(w[k][1], w[k][0], 0x04020100u), w[k][1] >> 8, unorm);
                                                b = pair_word(__builtin_amdgcn_perm(w[k][3], w[k][2], 0x04020100u), w[k][3] >> 8, unorm);
                                        } else { // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
                                                a = pair_word(w[k][0], w[k][1], unorm);
                                                b = pair_word(__builtin_amdgcn_alignbit(w[k][2], w[k][1], 16), w[k][2] >> 16, unorm);
                                        }
                                        ug::st_stream((uint2 *) d + q, make_uint2(a, b));
                                } else if (q < quads) {
                                        quad_slow<BPP, true>(s, d, q, width, unorm);
                                }
                        }
                } else {
#pragma unroll
                        for (int k = 0; k < Q; k++) {
                                const int q = q0 + k * kBlock;
                                if (q < quads) quad_slow<BPP, false>(s, d, q, width, unorm);
                        }
                }
        }
}

template <int BPP, bool FAST>
int launch(const uint8_t *src, uint8_t *dst, int width, int height, long sp, long dp, hipStream_t st)
{
        const int quads = (width + 3) / 4;
        // Q: quads per lane -- 4 where a line fills a workgroup that way (4K: 960 quads, 8K: 1920), fewer for short lines
        const int q = FAST ? (quads >= 3 * kBlock ? 4 : (quads >= kBlock + kBlock / 2 ? 2 : 1)) : 1;
        const dim3 grid((unsigned) ((quads + kBlock * q - 1) / (kBlock * q)), (unsigned) (height < 65535 ? height : 65535));
        if (q == 4) hipLaunchKernelGGL((rgb_to_uyvy_gl_kernel<BPP, 4, FAST>), grid, dim3(kBlock), 0, st, src, sp, dst, dp, width, height);
        else if (q == 2) hipLaunchKernelGGL((rgb_to_uyvy_gl_kernel<BPP, 2, FAST>), grid, dim3(kBlock), 0, st, src, sp, dst, dp, width, height);
        else hipLaunchKernelGGL((rgb_to_uyvy_gl_kernel<BPP, 1, FAST>), grid, dim3(kBlock), 0, st, src, sp, dst, dp, width, height);
        UG_HIP_LAUNCH_CHECK();
        return UG_HIP_SUCCESS;
}

} // namespace

namespace ug {

// behind ug_hip_pixfmt_convert[_batch] (pixfmt.hip), which has checked the arguments; pitches > 0
int uyvy_gl_convert(ug_pixfmt_t in, const void *src, void *dst, int width, int height, int src_pitch, int dst_pitch, hipStream_t st)
{
        const uint8_t *s = (const uint8_t *) src;
        uint8_t *d = (uint8_t *) dst;
        const bool dst_ok = !(7 & (uintptr_t) d) && !(dst_pitch & 7);
        if (in == UG_PF_RGBA) {
                if (dst_ok && !(15 & (uintptr_t) s) && !(src_pitch & 15)) return launch<4, true>(s, d, width, height, src_pitch, dst_pitch, st);
                return launch<4, false>(s, d, width, height, src_pitch, dst_pitch, st);
        }
        if (in == UG_PF_RGB) {
                if (dst_ok && !(3 & (uintptr_t) s) && !(src_pitch & 3)) return launch<3, true>(s, d, width, height, src_pitch, dst_pitch, st);
                return launch<3, false>(s, d, width, height, src_pitch, dst_pitch, st);
        }
        set_last_error_msg("ug_hip_pixfmt_convert: UG_PF_UYVY_GL is an output of UG_PF_RGB / UG_PF_RGBA only");
        return UG_HIP_EUNSUPP;
}

} // namespace ug
