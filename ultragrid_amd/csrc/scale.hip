// scale.hip -- ug_hip_scale: the `scale` video postprocessor (src/vo_postprocess/scale.c) on gfx950.
//
// The reference draws one full-viewport quad over the frame uploaded as a GL_RGBA texture with GL_LINEAR / GL_CLAMP_TO_EDGE filtering and
// reads the framebuffer back (scale.c:255-305).  What GL leaves to the implementation -- subtexel precision and the rounding of the weights --
// is pinned to Mesa llvmpipe executing the module (tests/golden/scale_gl_ref.npz): per axis the sample position in 1/256 texel,
// p = round_half_up((2x + 1) * n_in * 128 / n_out) - 128, and per byte lerp(a, b, w) = (a * (256 - w) + b * w + 128) >> 8, columns first
// (tests/scale_gl_restatement.py; include/ug_mi355x.h states the rule and the deviations).
//
// Layout.  A wave covers 64 x 4 consecutive output texels of one output line (16 B per lane: one dwordx4 store where the line allows it)
// and walks kRows texel rows; the four waves of a workgroup take four consecutive row groups, grid.z = frame.  A lane computes its four columns'
// positions once (exact: 64-bit numerators, an fp64 quotient corrected by one step) and reuses them on every row; the row position is
// wave-uniform.  An INTERLACED_MERGED picture is walked by output line: line L is texel row L / 2, texel columns (L & 1) * line texels + x --
// the blocks of one grid.y half take the even lines, the other half the odd lines, so the column positions stay fixed per lane.
// Per texel: four 4-byte gathers (2 x 2 texels) and three byte-wise lerps on two 16-bit-per-channel halves (a * (256 - w) + b * w + 128 fits
// 16 bits: 255 * 256 + 128 < 65536).
#include "ug_common.h"

namespace {

constexpr int kWaveX = 64;  // lanes along a line, 4 texels each
constexpr int kWavesY = 4;  // waves of a workgroup, stacked along the rows
constexpr int kRows = 4;    // texel rows walked by one wave
constexpr int kTexelsPerLane = 4;

// round_half_up((2x + 1) * n_in * 128 / n_out) - 128, exactly: q = floor(num / den), num = (2x + 1) * n_in * 256 + n_out, den = 2 * n_out
// (num < 2^44: exact in fp64; the correctly rounded quotient is at most one away from the floor)
__device__ __forceinline__ int position(int x, int n_in, int n_out)
{
        const long long num = (2LL * x + 1) * n_in * 256 + n_out, den = 2LL * n_out;
        long long q = (long long) ((double) num / (double) den);
        if (q * den > num) q--;
        else if ((q + 1) * den <= num) q++;
        return (int) q - 128;
}

// byte-wise (a * (256 - w) + b * w + 128) >> 8 of two texels
__device__ __forceinline__ uint32_t lerp4(uint32_t a, uint32_t b, uint32_t w)
{
        const uint32_t v = 256u - w;
        const uint32_t lo = (a & 0x00FF00FFu) * v + (b & 0x00FF00FFu) * w + 0x00800080u;
        const uint32_t hi = ((a >> 8) & 0x00FF00FFu) * v + ((b >> 8) & 0x00FF00FFu) * w + 0x00800080u;
        return ((lo >> 8) & 0x00FF00FFu) | (hi & 0xFF00FF00u);
}

struct Geometry {
        int tpl_in, tpl_out;        // texels per LINE (in / out)
        int tw_in, th_in, tw_out, th_out; // texture sizes (merged: 2 x tpl, lines / 2)
        long spitch, dpitch;
        size_t sstride, dstride;
        int merged;
};

__global__ __launch_bounds__(kWaveX * kWavesY) void scale_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, Geometry g, bool wide)
{
        const int lane = threadIdx.x % kWaveX, wave = threadIdx.x / kWaveX;
        const int parity = g.merged ? (int) (blockIdx.y & 1) : 0;
        const int group = g.merged ? (int) (blockIdx.y >> 1) : (int) blockIdx.y;
        const int x0 = (blockIdx.x * kWaveX + lane) * kTexelsPerLane; // texel of the output LINE
        if (x0 >= g.tpl_out) return;
        const uint8_t *s = src + (size_t) blockIdx.z * g.sstride;
        uint8_t *d = dst + (size_t) blockIdx.z * g.dstride;
        // the four columns: byte offsets of texels i0 / i1 inside a texel row (merged: the second half lies on the next line), weights
        uint32_t c0[kTexelsPerLane], c1[kTexelsPerLane], wx[kTexelsPerLane];
#pragma unroll
        for (int k = 0; k < kTexelsPerLane; k++) {
                const int c = parity * g.tpl_out + min(x0 + k, g.tpl_out - 1);
                const int p = position(c, g.tw_in, g.tw_out);
                const int i0 = min(max(p >> 8, 0), g.tw_in - 1), i1 = min(max((p >> 8) + 1, 0), g.tw_in - 1);
                wx[k] = (uint32_t) (p & 255);
                c0[k] = i0 < g.tpl_in ? 4u * i0 : (uint32_t) g.spitch + 4u * (i0 - g.tpl_in);
                c1[k] = i1 < g.tpl_in ? 4u * i1 : (uint32_t) g.spitch + 4u * (i1 - g.tpl_in);
        }
        const int r_begin = (group * kWavesY + wave) * kRows;
        const int r_end = min(r_begin + kRows, g.th_out);
        const int row_lines = g.merged ? 2 : 1;
        for (int r = r_begin; r < r_end; r++) {
                const int p = position(r, g.th_in, g.th_out);
                const int j0 = min(max(p >> 8, 0), g.th_in - 1), j1 = min(max((p >> 8) + 1, 0), g.th_in - 1);
                const uint32_t wy = (uint32_t) (p & 255);
                const uint8_t *row0 = s + (long) j0 * row_lines * g.spitch, *row1 = s + (long) j1 * row_lines * g.spitch;
                uint32_t out[kTexelsPerLane];
#pragma unroll
                for (int k = 0; k < kTexelsPerLane; k++) {
                        const uint32_t t00 = *(const uint32_t *) (row0 + c0[k]), t01 = *(const uint32_t *) (row0 + c1[k]);
                        const uint32_t t10 = *(const uint32_t *) (row1 + c0[k]), t11 = *(const uint32_t *) (row1 + c1[k]);
                        out[k] = lerp4(lerp4(t00, t01, wx[k]), lerp4(t10, t11, wx[k]), wy);
                }
                uint8_t *line = d + (long) (r * row_lines + parity) * g.dpitch;
                if (wide && x0 + kTexelsPerLane <= g.tpl_out) {
                        ug::st_stream((uint4 *) (line + 4L * x0), make_uint4(out[0], out[1], out[2], out[3]));
                } else {
#pragma unroll
                        for (int k = 0; k < kTexelsPerLane; k++) {
                                if (x0 + k < g.tpl_out) ug::st_stream((uint32_t *) (line + 4L * (x0 + k)), out[k]);
                        }
                }
        }
}

} // namespace

extern "C" int ug_hip_scale(const struct ug_scale_desc *d, ug_hip_stream_t stream)
{
        if (d == nullptr || d->src == nullptr || d->dst == nullptr) {
                ug::set_last_error_msg("ug_hip_scale: NULL descriptor or pointer");
                return UG_HIP_EINVAL;
        }
        if (d->format != UG_PF_RGBA && d->format != UG_PF_UYVY) {
                ug::set_last_error_msg("ug_hip_scale: format must be UG_PF_RGBA or UG_PF_UYVY (scale.c:68)");
                return UG_HIP_EUNSUPP;
        }
        if (!ug::dims_ok(d->src_width, d->src_height) || !ug::dims_ok(d->dst_width, d->dst_height)) return ug::refuse_size("ug_hip_scale");
        const int merged = d->interlaced_merged != 0;
        if (merged && (d->src_height < 2 || d->dst_height % 2 != 0)) {
                ug::set_last_error_msg("ug_hip_scale: interlaced_merged needs src_height >= 2 and an even dst_height");
                return UG_HIP_EINVAL;
        }
        const long long sls = ug::linesize(d->format, d->src_width), dls = ug::linesize(d->format, d->dst_width);
        const long long sp = d->src_pitch ? (long long) d->src_pitch : sls, dp = d->dst_pitch ? (long long) d->dst_pitch : dls;
        if (d->src_pitch > (size_t) ug::kMaxFrameBytes || d->dst_pitch > (size_t) ug::kMaxFrameBytes || sp < sls || dp < dls || sp % 4 || dp % 4 ||
            !ug::span_ok(sp, d->src_height) || !ug::span_ok(dp, d->dst_height)) {
                return ug::refuse_size("ug_hip_scale");
        }
        if (d->frames < 1 || d->frames > 65535 ||
            (d->frames > 1 && (d->src_frame_stride < (size_t) (sp * d->src_height) || d->dst_frame_stride < (size_t) (dp * d->dst_height) ||
                               d->src_frame_stride % 4 || d->dst_frame_stride % 4 ||
                               d->src_frame_stride > SIZE_MAX / (size_t) d->frames || d->dst_frame_stride > SIZE_MAX / (size_t) d->frames))) {
                ug::set_last_error_msg("ug_hip_scale: frames 1..65535, strides multiples of 4 that cover a frame");
                return UG_HIP_EINVAL;
        }
        if ((3 & (uintptr_t) d->src) || (3 & (uintptr_t) d->dst)) {
                ug::set_last_error_msg("ug_hip_scale: src and dst must be 4-byte aligned");
                return UG_HIP_EINVAL;
        }
        Geometry g;
        g.tpl_in = (int) (sls / 4);
        g.tpl_out = (int) (dls / 4);
        g.merged = merged;
        g.tw_in = merged ? 2 * g.tpl_in : g.tpl_in;
        g.tw_out = merged ? 2 * g.tpl_out : g.tpl_out;
        g.th_in = merged ? d->src_height / 2 : d->src_height;
        g.th_out = merged ? d->dst_height / 2 : d->dst_height;
        g.spitch = (long) sp;
        g.dpitch = (long) dp;
        g.sstride = d->src_frame_stride;
        g.dstride = d->dst_frame_stride;
        // dwordx4 stores: every line start 16-B aligned
        const bool wide = !(15 & (uintptr_t) d->dst) && !(dp & 15) && (d->frames == 1 || !(d->dst_frame_stride & 15));
        const int groups = (g.th_out + kWavesY * kRows - 1) / (kWavesY * kRows);
        const dim3 grid((unsigned) ((g.tpl_out + kWaveX * kTexelsPerLane - 1) / (kWaveX * kTexelsPerLane)), (unsigned) (groups * (merged ? 2 : 1)),
                        (unsigned) d->frames);
        hipLaunchKernelGGL(scale_kernel, grid, dim3(kWaveX * kWavesY), 0, (hipStream_t) stream, (const uint8_t *) d->src, (uint8_t *) d->dst, g, wide);
        UG_HIP_LAUNCH_CHECK();
        return UG_HIP_SUCCESS;
}
