// pixel_filter.hip -- ug_hip_pixel_filter: the reference's per-pixel colour filters and its two mirror filters on gfx950.
//
//   UG_PXF_MATRIX   src/capture_filter/matrix.c:127-309 (`-F/-p matrix:a:..:i[:no-bound-check]`): a 3x3 double matrix on unpacked pixels; UYVY comes
//                   out as RGB (both pixels of a pair with the pair's U and V, offsets -16 / -128, :158-181), RGB -> RGB, RG48 -> RG48
//   UG_PXF_MATRIX2  src/capture_filter/matrix2.c:167-243 (`matrix2`): the matrix on offset Y / Cb / Cr; UYVY directly (chroma from the mean luma of
//                   the pair, :174-196), Y416 (:219-237), v210 through vc_copylineV210toY416 -> the Y416 loop -> vc_copylineY416toV210 in one pass
//   UG_PXF_LUT      src/capture_filter/gamma.cpp:119-145 (`gamma`): out[i] = lut[in[i]], 8 -> 8, 16 -> 16, 8 -> 16, 16 -> 8 bits
//   UG_PXF_GRAY     src/capture_filter/grayscale.c:95-102: U = V = 127
//   UG_PXF_MIRROR   src/capture_filter/mirror.c:76-93: a UYVY line reversed pair by pair, the two lumas of a pair swapped
//   UG_PXF_FLIP     src/capture_filter/flip.c:96-99: line y -> line lines - 1 - y
//
// Arithmetic (tests/pixel_filter_restatement.py states the same in numpy): integer -> double is exact; the products and sums are IEEE fp64 in the
// reference's left-to-right order, never fused (the library builds with -ffp-contract=off); double -> integer is truncation toward zero to int32
// and then the low 8 or 16 bits -- what the x86-64 build's cvttsd2si and a byte / word store do where the reference's conversion to
// unsigned char / uint16_t is undefined.  The entry point refuses matrices whose results could leave int32 (matrix_ok() below).
//
// Layout.  A lane owns one unit of a line: 16, 32 or 48 input bytes (a whole number of pixels, pairs or v210 groups) and the 16, 32 or 48 output
// bytes they become.  A workgroup is 64 units x 4 lines, grid.y the rest of the lines, grid.z the frame.  A whole unit whose address is a multiple
// of 16 moves as dwordx4, anything else word by word (multiples of 4) or byte by byte -- also the last, partial unit of a line -- so any
// pointer, pitch and stride is taken and the aligned picture pays nothing for it.  The 8-bit-input LUTs (256 or 512 bytes) are copied to LDS by
// every workgroup; the 65 536-entry tables are gathered from global memory, i.e. from L2, which holds their 64 / 128 KiB many times over.
#include "ug_common.h"
#include "v210_y416_device.h"

#include <math.h>
#include <string.h>

namespace {

enum { LUT_8_8 = 0, LUT_16_16 = 1, LUT_8_16 = 2, LUT_16_8 = 3 }; // FMT of the LUT instantiations
constexpr int kUnitsX = 64, kLinesY = 4;

struct Params {
        const uint8_t *src;
        uint8_t *dst;
        const void *lut;
        long spitch, dpitch;
        size_t sstride, dstride;
        int in_line, out_line, lines; // bytes of a source / destination line
        double m[9];
};

// input / output bytes of a lane's unit
template <int OP, int FMT> struct Unit { static constexpr int IN = 16, OUT = 16; };
template <> struct Unit<UG_PXF_MATRIX, UG_PF_UYVY> { static constexpr int IN = 32, OUT = 48; }; // 8 pairs -> 16 RGB pixels
template <> struct Unit<UG_PXF_MATRIX, UG_PF_RGB> { static constexpr int IN = 48, OUT = 48; };  // 16 pixels
template <> struct Unit<UG_PXF_MATRIX, UG_PF_RG48> { static constexpr int IN = 48, OUT = 48; }; // 8 pixels
template <> struct Unit<UG_PXF_LUT, LUT_8_16> { static constexpr int IN = 16, OUT = 32; };
template <> struct Unit<UG_PXF_LUT, LUT_16_8> { static constexpr int IN = 32, OUT = 16; };

// n bytes (<= 4 * NW) from p; the rest of the unit is zero
template <int NW> __device__ __forceinline__ void ld(const uint8_t *p, int n, uint32_t (&w)[NW])
{
        const uintptr_t a = (uintptr_t) p;
        if (n == 4 * NW && a % 16 == 0) {
#pragma unroll
                for (int i = 0; i < NW / 4; i++) {
                        const uint4 v = ((const uint4 *) p)[i];
                        w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
                }
                return;
        }
#pragma unroll
        for (int i = 0; i < NW; i++) {
                uint32_t v = 0;
                if (a % 4 == 0 && 4 * i + 4 <= n) {
                        v = *(const uint32_t *) (p + 4 * i);
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) if (4 * i + b < n) v |= (uint32_t) p[4 * i + b] << (8 * b);
                }
                w[i] = v;
        }
}

// bytes [lo, hi) of the unit to p + lo ...
template <int NW> __device__ __forceinline__ void st(uint8_t *p, const uint32_t (&w)[NW], int lo, int hi)
{
        const uintptr_t a = (uintptr_t) p;
        if (lo == 0 && hi == 4 * NW && a % 16 == 0) {
#pragma unroll
                for (int i = 0; i < NW / 4; i++) ug::st_stream((uint4 *) p + i, make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]));
                return;
        }
#pragma unroll
        for (int i = 0; i < NW; i++) {
                if (a % 4 == 0 && 4 * i >= lo && 4 * i + 4 <= hi) {
                        *(uint32_t *) (p + 4 * i) = w[i];
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) if (4 * i + b >= lo && 4 * i + b < hi) p[4 * i + b] = (uint8_t) (w[i] >> (8 * b));
                }
        }
}

// byte / 16-bit element i of a unit held in words (i is a constant wherever these are used: the loops around them are unrolled)
template <int NW> __device__ __forceinline__ uint32_t getb(const uint32_t (&w)[NW], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }
template <int NW> __device__ __forceinline__ uint32_t geth(const uint32_t (&w)[NW], int i) { return (w[i >> 1] >> (16 * (i & 1))) & 0xffffu; }
template <int NW> __device__ __forceinline__ void putb(uint32_t (&w)[NW], int i, uint32_t v) { w[i >> 2] |= (v & 0xffu) << (8 * (i & 3)); }
template <int NW> __device__ __forceinline__ void puth(uint32_t (&w)[NW], int i, uint32_t v) { w[i >> 1] |= (v & 0xffffu) << (16 * (i & 1)); }

// the conversion rule: toward zero to int32 (the entry point keeps the value inside it), then -- by the callers' masks -- the low bits
__device__ __forceinline__ uint32_t cvt(double v) { return (uint32_t) (int) v; }
// matrix.c's `int val = ...; CLAMP(val, 0, 255)` or its direct conversion
template <bool CLAMP> __device__ __forceinline__ uint32_t cvt_matrix(double v)
{
        const int i = (int) v;
        return CLAMP ? (uint32_t) (i < 0 ? 0 : (i > 255 ? 255 : i)) : (uint32_t) i;
}
// one row of matrix.c: m[0] * a + m[1] * b + m[2] * c, left to right
__device__ __forceinline__ double row(const double *m, double a, double b, double c) { return m[0] * a + m[1] * b + m[2] * c; }
// one row of matrix2.c: off + m[0] * a + m[1] * b + m[2] * c, left to right
__device__ __forceinline__ double row2(double off, const double *m, double a, double b, double c) { return off + m[0] * a + m[1] * b + m[2] * c; }

// matrix2.c:219-237 on one Y416 pixel
__device__ __forceinline__ void matrix2_y416(const double *m, uint32_t u_in, uint32_t y_in, uint32_t v_in, uint32_t &u_out, uint32_t &y_out, uint32_t &v_out)
{
        const double u = (int) u_in - (1 << 15), y = (int) y_in - (1 << 12), v = (int) v_in - (1 << 15);
        u_out = cvt(row2(1 << 15, m + 3, y, u, v)) & 0xffffu;
        y_out = cvt(row2(1 << 12, m, y, u, v)) & 0xffffu;
        v_out = cvt(row2(1 << 15, m + 6, y, u, v)) & 0xffffu;
}

template <int OP, int FMT, bool CLAMP>
__global__ __launch_bounds__(kUnitsX *kLinesY) void pixel_filter_kernel(Params p)
{
        constexpr int IN = Unit<OP, FMT>::IN, OUT = Unit<OP, FMT>::OUT, NI = IN / 4, NO = OUT / 4;
        constexpr bool kLdsLut = OP == UG_PXF_LUT && (FMT == LUT_8_8 || FMT == LUT_8_16);
        __shared__ uint16_t s_lut[kLdsLut ? 256 : 1];
        if constexpr (kLdsLut) { // before any lane leaves: every lane of the workgroup reaches the barrier
                const int t = threadIdx.y * kUnitsX + threadIdx.x;
                s_lut[t] = FMT == LUT_8_8 ? ((const uint8_t *) p.lut)[t] : ((const uint16_t *) p.lut)[t];
                __syncthreads();
        }
        const int y = blockIdx.y * kLinesY + threadIdx.y;
        const long x0 = ((long) blockIdx.x * kUnitsX + threadIdx.x) * IN;
        if (y >= p.lines || x0 >= p.in_line) return;
        const int n_in = (int) min((long) IN, p.in_line - x0);
        const int n_out = (int) ((long) n_in * OUT / IN); // (a line is a whole number of pixels, pairs or groups: exact)
        const uint8_t *const s = p.src + (size_t) blockIdx.z * p.sstride + (long) y * p.spitch + x0;
        const int yd = OP == UG_PXF_FLIP ? p.lines - 1 - y : y;
        uint8_t *const dline = p.dst + (size_t) blockIdx.z * p.dstride + (long) yd * p.dpitch;
        uint32_t in[NI], out[NO];
        ld<NI>(s, n_in, in);
#pragma unroll
        for (int i = 0; i < NO; i++) out[i] = 0;
        const double *const m = p.m;

        if constexpr (OP == UG_PXF_MATRIX && FMT == UG_PF_UYVY) {
#pragma unroll
                for (int k = 0; k < IN / 4; k++) { // a pair: U Y0 V Y1 -> R G B R G B
                        const double u = (double) getb(in, 4 * k) - 128, v = (double) getb(in, 4 * k + 2) - 128;
#pragma unroll
                        for (int j = 0; j < 2; j++) {
                                const double l = (double) getb(in, 4 * k + 1 + 2 * j) - 16;
#pragma unroll
                                for (int c = 0; c < 3; c++) putb(out, 6 * k + 3 * j + c, cvt_matrix<CLAMP>(row(m + 3 * c, l, u, v)));
                        }
                }
        } else if constexpr (OP == UG_PXF_MATRIX && FMT == UG_PF_RGB) {
#pragma unroll
                for (int k = 0; k < IN / 3; k++) {
                        const double a = getb(in, 3 * k), b = getb(in, 3 * k + 1), c3 = getb(in, 3 * k + 2);
#pragma unroll
                        for (int c = 0; c < 3; c++) putb(out, 3 * k + c, cvt_matrix<CLAMP>(row(m + 3 * c, a, b, c3)));
                }
        } else if constexpr (OP == UG_PXF_MATRIX && FMT == UG_PF_RG48) {
#pragma unroll
                for (int k = 0; k < IN / 6; k++) { // (bounds-checked: 0..255 here too, matrix.c:217)
                        const double a = geth(in, 3 * k), b = geth(in, 3 * k + 1), c3 = geth(in, 3 * k + 2);
#pragma unroll
                        for (int c = 0; c < 3; c++) puth(out, 3 * k + c, cvt_matrix<CLAMP>(row(m + 3 * c, a, b, c3)));
                }
        } else if constexpr (OP == UG_PXF_MATRIX2 && FMT == UG_PF_UYVY) {
#pragma unroll
                for (int k = 0; k < IN / 4; k++) {
                        const double u = (int) getb(in, 4 * k) - 128, y1 = (int) getb(in, 4 * k + 1) - 16;
                        const double v = (int) getb(in, 4 * k + 2) - 128, y2 = (int) getb(in, 4 * k + 3) - 16;
                        const double ym = (y1 + y2) / 2;
                        putb(out, 4 * k, cvt(row2(128, m + 3, ym, u, v)));
                        putb(out, 4 * k + 1, cvt(row2(16, m, y1, u, v)));
                        putb(out, 4 * k + 2, cvt(row2(128, m + 6, ym, u, v)));
                        putb(out, 4 * k + 3, cvt(row2(16, m, y2, u, v)));
                }
        } else if constexpr (OP == UG_PXF_MATRIX2 && FMT == UG_PF_Y416) {
#pragma unroll
                for (int k = 0; k < IN / 8; k++) {
                        uint32_t u, l, v;
                        matrix2_y416(m, geth(in, 4 * k), geth(in, 4 * k + 1), geth(in, 4 * k + 2), u, l, v);
                        puth(out, 4 * k, u), puth(out, 4 * k + 1, l), puth(out, 4 * k + 2, v), puth(out, 4 * k + 3, 0xFFFFu);
                }
        } else if constexpr (OP == UG_PXF_MATRIX2 && FMT == UG_PF_V210) {
                uint32_t Y[6], U[3], V[3];
                ug::v210_unpack(in[0], in[1], in[2], in[3], Y, U, V);
                uint16_t t[24];
#pragma unroll
                for (int i = 0; i < 6; i++) { // vc_copylineV210toY416: sample << 6, the pair's chroma for both pixels
                        uint32_t u, l, v;
                        matrix2_y416(m, U[i / 2] << 6, Y[i] << 6, V[i / 2] << 6, u, l, v);
                        t[4 * i] = (uint16_t) u, t[4 * i + 1] = (uint16_t) l, t[4 * i + 2] = (uint16_t) v, t[4 * i + 3] = 0xFFFF;
                }
                ug::y416_pack_v210(t, out);
        } else if constexpr (OP == UG_PXF_LUT) {
                if constexpr (FMT == LUT_8_8) {
#pragma unroll
                        for (int i = 0; i < IN; i++) putb(out, i, s_lut[getb(in, i)]);
                } else if constexpr (FMT == LUT_8_16) {
#pragma unroll
                        for (int i = 0; i < IN; i++) puth(out, i, s_lut[getb(in, i)]);
                } else if constexpr (FMT == LUT_16_16) {
#pragma unroll
                        for (int i = 0; i < IN / 2; i++) puth(out, i, ((const uint16_t *) p.lut)[geth(in, i)]);
                } else {
#pragma unroll
                        for (int i = 0; i < IN / 2; i++) putb(out, i, ((const uint8_t *) p.lut)[geth(in, i)]);
                }
        } else if constexpr (OP == UG_PXF_GRAY) {
#pragma unroll
                for (int i = 0; i < NI; i++) out[i] = (in[i] & 0xff00ff00u) | 0x007f007fu;
        } else if constexpr (OP == UG_PXF_MIRROR) {
                // pair j of the reversed unit = pair 3 - j with its lumas swapped; of a partial unit of k pairs the last k of these are its output
#pragma unroll
                for (int i = 0; i < NI; i++) {
                        const uint32_t w = in[NI - 1 - i];
                        out[i] = (w & 0x00ff00ffu) | (w >> 16 & 0xff00u) | (w << 16 & 0xff000000u);
                }
                st<NO>(dline + (p.out_line - x0 - OUT), out, OUT - n_out, OUT);
                return;
        } else { // FLIP
#pragma unroll
                for (int i = 0; i < NI; i++) out[i] = in[i];
        }
        st<NO>(dline + x0 / IN * OUT, out, 0, n_out);
}

// A/B build (`make lutlds`, -DUG_PXF_LUT16_LDS=1; not the product): the 65 536-entry tables in LDS -- 64 or 128 KiB of the CU's 160 --, one
// workgroup of 1024 lanes per CU walking the units of all frames with a grid stride.  Measured against the L2 gather: DESIGN.md 4.12.
#ifndef UG_PXF_LUT16_LDS
#define UG_PXF_LUT16_LDS 0
#endif
#if UG_PXF_LUT16_LDS
template <int FMT> __global__ __launch_bounds__(1024) void lut16_lds_kernel(Params p, int units_x, long total)
{
        extern __shared__ uint4 s_tab[];
        constexpr int IN = Unit<UG_PXF_LUT, FMT>::IN, OUT = Unit<UG_PXF_LUT, FMT>::OUT, NI = IN / 4, NO = OUT / 4;
        constexpr int kWords = (FMT == LUT_16_16 ? 131072 : 65536) / 16;
        for (int i = threadIdx.x; i < kWords; i += 1024) s_tab[i] = ((const uint4 *) p.lut)[i];
        __syncthreads();
        for (long u = blockIdx.x * 1024L + threadIdx.x; u < total; u += gridDim.x * 1024L) {
                const long x0 = (u % units_x) * IN, line = u / units_x;
                const int y = (int) (line % p.lines);
                const size_t f = (size_t) (line / p.lines);
                const int n_in = (int) min((long) IN, p.in_line - x0);
                uint32_t in[NI], out[NO];
                ld<NI>(p.src + f * p.sstride + (long) y * p.spitch + x0, n_in, in);
#pragma unroll
                for (int i = 0; i < NO; i++) out[i] = 0;
#pragma unroll
                for (int i = 0; i < IN / 2; i++) {
                        if constexpr (FMT == LUT_16_16) puth(out, i, ((const uint16_t *) s_tab)[geth(in, i)]);
                        else putb(out, i, ((const uint8_t *) s_tab)[geth(in, i)]);
                }
                st<NO>(p.dst + f * p.dstride + (long) y * p.dpitch + x0 / IN * OUT, out, 0, n_in * OUT / IN);
        }
}

template <int FMT> bool launch_lut16_lds(const Params &p, int frames, hipStream_t st)
{
        constexpr int IN = Unit<UG_PXF_LUT, FMT>::IN;
        constexpr int kBytes = FMT == LUT_16_16 ? 131072 : 65536;
        int dev = 0, cus = 0;
        if ((uintptr_t) p.lut % 16 || hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1 ||
            hipFuncSetAttribute((const void *) lut16_lds_kernel<FMT>, hipFuncAttributeMaxDynamicSharedMemorySize, kBytes) != hipSuccess) {
                return false;
        }
        const int units_x = (p.in_line + IN - 1) / IN;
        const long total = (long) units_x * p.lines * frames;
        hipLaunchKernelGGL((lut16_lds_kernel<FMT>), dim3((unsigned) cus), dim3(1024), kBytes, st, p, units_x, total);
        return true;
}
#endif

// (format, natural output format) per op; FLIP takes every packed format of ug_pixfmt_t that has a line size
int natural_out(int op, ug_pixfmt_t f)
{
        switch (op) {
        case UG_PXF_MATRIX: return f == UG_PF_UYVY ? UG_PF_RGB : (f == UG_PF_RGB || f == UG_PF_RG48 ? (int) f : -1);
        case UG_PXF_MATRIX2: return f == UG_PF_UYVY || f == UG_PF_Y416 || f == UG_PF_V210 ? (int) f : -1;
        case UG_PXF_LUT: return f == UG_PF_RGB || f == UG_PF_RG48 ? (int) f : -1;
        case UG_PXF_GRAY:
        case UG_PXF_MIRROR: return f == UG_PF_UYVY ? (int) f : -1;
        case UG_PXF_FLIP: return f != UG_PF_I420 && f != UG_PF_UYVY_GL && ug::linesize(f, 2) > 0 ? (int) f : -1;
        default: return -1;
        }
}

int elem_size(ug_pixfmt_t f)
{
        switch (f) {
        case UG_PF_RG48: case UG_PF_Y416: case UG_PF_Y216: return 2;
        case UG_PF_V210: case UG_PF_R10K: case UG_PF_R12L: case UG_PF_DVS10: return 4;
        default: return 1;
        }
}

// The int32 step of the conversion rule stays defined: every coefficient finite, and per row sum |m| * (65535 + 32768) < 2^31 (the largest input
// magnitude of any format plus the largest offset added to a row)
bool matrix_ok(const double *m)
{
        for (int r = 0; r < 3; r++) {
                double sum = 0;
                for (int c = 0; c < 3; c++) {
                        if (!isfinite(m[3 * r + c])) return false;
                        sum += fabs(m[3 * r + c]);
                }
                if (!(sum * (65535.0 + 32768.0) < 2147483648.0)) return false;
        }
        return true;
}

bool overlap(const void *a, size_t an, const void *b, size_t bn)
{
        const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
        return x < y + bn && y < x + an;
}

template <int OP, int FMT, bool CLAMP = false> void launch(const Params &p, int frames, hipStream_t st)
{
        constexpr int IN = Unit<OP, FMT>::IN;
        const long units = ((long) p.in_line + IN - 1) / IN;
        const dim3 grid((unsigned) ((units + kUnitsX - 1) / kUnitsX), (unsigned) ((p.lines + kLinesY - 1) / kLinesY), (unsigned) frames);
        hipLaunchKernelGGL((pixel_filter_kernel<OP, FMT, CLAMP>), grid, dim3(kUnitsX, kLinesY), 0, st, p);
}

} // namespace

extern "C" int ug_hip_pixel_filter_supported(int op, ug_pixfmt_t format)
{
        return natural_out(op, format) >= 0 ? 1 : 0;
}

extern "C" int ug_hip_matrix2_preset(const char *name, double m[9])
{
        // y601_y709_matrix, matrix2.c:69-73
        static const double y601_to_y709[9] = { 1, -0.11555, -0.207938, 0, 1.01864, 0.114618, 0, 0.075049, 1.025327 };
        if (name == nullptr || m == nullptr || strcmp(name, "y601_to_y709") != 0) {
                ug::set_last_error_msg("ug_hip_matrix2_preset: the one preset is y601_to_y709");
                return UG_HIP_EINVAL;
        }
        memcpy(m, y601_to_y709, sizeof y601_to_y709);
        return UG_HIP_SUCCESS;
}

extern "C" int ug_hip_gamma_lut(double gamma, int in_bits, int out_bits, void *table_host)
{
        if (!(gamma > 0) || !isfinite(gamma) || (in_bits != 8 && in_bits != 16) || (out_bits != 8 && out_bits != 16) || table_host == nullptr) {
                ug::set_last_error_msg("ug_hip_gamma_lut: gamma finite and > 0, in_bits and out_bits 8 or 16, a table to fill");
                return UG_HIP_EINVAL;
        }
        // gamma.cpp:74-93: pow(i / max_in, gamma) * max_out, converted to the table's element
        const int max_in = (1 << in_bits) - 1, max_out = (1 << out_bits) - 1;
        for (int i = 0; i <= max_in; ++i) {
                const double v = pow(static_cast<double>(i) / max_in, gamma) * max_out;
                if (out_bits == 8) ((uint8_t *) table_host)[i] = (uint8_t) v;
                else ((uint16_t *) table_host)[i] = (uint16_t) v;
        }
        return UG_HIP_SUCCESS;
}

extern "C" int ug_hip_pixel_filter(const struct ug_pixel_filter_desc *d, ug_hip_stream_t stream)
{
        auto bad = [](const char *msg) { ug::set_last_error_msg(msg); return UG_HIP_EINVAL; };
        if (d == nullptr) return bad("ug_hip_pixel_filter: NULL descriptor");
        const int op = d->op;
        if (op < UG_PXF_MATRIX || op > UG_PXF_FLIP) return bad("ug_hip_pixel_filter: op must be one of UG_PXF_*");
        const int nat = natural_out(op, d->format);
        if (nat < 0) {
                ug::set_last_error_msg("ug_hip_pixel_filter: unsupported format for this op (matrix: UYVY, RGB, RG48; matrix2: UYVY, v210, Y416; LUT: RGB, RG48; "
                                       "gray, mirror: UYVY; flip: packed formats)");
                return UG_HIP_EUNSUPP;
        }
        ug_pixfmt_t out_format = d->out_format == UG_PF_NONE ? (ug_pixfmt_t) nat : d->out_format;
        if (op == UG_PXF_LUT ? (out_format != UG_PF_RGB && out_format != UG_PF_RG48) : out_format != (ug_pixfmt_t) nat) {
                ug::set_last_error_msg("ug_hip_pixel_filter: out_format must be UG_PF_NONE or the op's output (matrix on UYVY: RGB; LUT: RGB or RG48; else the input's)");
                return UG_HIP_EUNSUPP;
        }
        if (d->src == nullptr || d->dst == nullptr) return bad("ug_hip_pixel_filter: NULL pointer");
        if ((op == UG_PXF_MATRIX || op == UG_PXF_MATRIX2) && !matrix_ok(d->matrix)) {
                return bad("ug_hip_pixel_filter: matrix coefficients must be finite with sum |m| * 98303 < 2^31 per row (the conversion to int32 is undefined beyond)");
        }
        if (op == UG_PXF_LUT && d->lut_dev == nullptr) return bad("ug_hip_pixel_filter: LUT needs lut_dev");
        if (d->lines < 1 || d->lines > ug::kMaxDim || d->width < 1 || d->width > ug::kMaxDim) return ug::refuse_size("ug_hip_pixel_filter");
        const long long L = ug::linesize(d->format, d->width), LO = ug::linesize(out_format, d->width);
        if (L <= 0 || LO <= 0) return ug::refuse_size("ug_hip_pixel_filter");
        if (op == UG_PXF_MATRIX && d->format == UG_PF_UYVY && d->width % 2) {
                return bad("ug_hip_pixel_filter: matrix on UYVY needs an even width (the pair of an odd last pixel has no room in the RGB line; the reference writes past its frame)");
        }
        if (d->src_pitch > (size_t) ug::kMaxFrameBytes || d->dst_pitch > (size_t) ug::kMaxFrameBytes) return ug::refuse_size("ug_hip_pixel_filter");
        const long long sp = d->src_pitch ? (long long) d->src_pitch : L, dp = d->dst_pitch ? (long long) d->dst_pitch : LO;
        if (sp < L || dp < LO || !ug::span_ok(sp, d->lines) || !ug::span_ok(dp, d->lines)) return ug::refuse_size("ug_hip_pixel_filter");
        const size_t ei = op == UG_PXF_FLIP ? 1 : elem_size(d->format), eo = op == UG_PXF_FLIP ? 1 : elem_size(out_format);
        if (sp % ei || dp % eo) return bad("ug_hip_pixel_filter: pitches must be multiples of the format's element (2 bytes: RG48, Y416; 4: v210)");
        const size_t sspan = (size_t) (sp * d->lines), dspan = (size_t) (dp * d->lines);
        if (d->frames < 1 || d->frames > 65535 ||
            (d->frames > 1 && (d->src_frame_stride < sspan || d->dst_frame_stride < dspan || d->src_frame_stride % ei || d->dst_frame_stride % eo ||
                               d->src_frame_stride > SIZE_MAX / (size_t) d->frames || d->dst_frame_stride > SIZE_MAX / (size_t) d->frames))) {
                return bad("ug_hip_pixel_filter: frames 1..65535, strides multiples of the element that cover a frame");
        }
        if ((uintptr_t) d->src % ei || (uintptr_t) d->dst % eo || (op == UG_PXF_LUT && out_format == UG_PF_RG48 && (uintptr_t) d->lut_dev % 2)) {
                return bad("ug_hip_pixel_filter: pointers must be aligned to the format's element");
        }
        const size_t sstride = d->frames > 1 ? d->src_frame_stride : 0, dstride = d->frames > 1 ? d->dst_frame_stride : 0;
        const size_t sall = sstride * (size_t) (d->frames - 1) + sspan, dall = dstride * (size_t) (d->frames - 1) + dspan;
        if (overlap(d->src, sall, d->dst, dall)) return bad("ug_hip_pixel_filter: source and destination must not overlap");
        Params p;
        p.src = (const uint8_t *) d->src;
        p.dst = (uint8_t *) d->dst;
        p.lut = d->lut_dev;
        p.spitch = (long) sp;
        p.dpitch = (long) dp;
        p.sstride = sstride;
        p.dstride = dstride;
        p.in_line = (int) L;
        p.out_line = (int) LO;
        p.lines = d->lines;
        for (int i = 0; i < 9; i++) p.m[i] = d->matrix[i];
        hipStream_t st = (hipStream_t) stream;
        const int f = d->frames;
        const bool clamp = d->clamp != 0;
        switch (op) {
        case UG_PXF_MATRIX:
                if (d->format == UG_PF_UYVY) clamp ? launch<UG_PXF_MATRIX, UG_PF_UYVY, true>(p, f, st) : launch<UG_PXF_MATRIX, UG_PF_UYVY>(p, f, st);
                else if (d->format == UG_PF_RGB) clamp ? launch<UG_PXF_MATRIX, UG_PF_RGB, true>(p, f, st) : launch<UG_PXF_MATRIX, UG_PF_RGB>(p, f, st);
                else clamp ? launch<UG_PXF_MATRIX, UG_PF_RG48, true>(p, f, st) : launch<UG_PXF_MATRIX, UG_PF_RG48>(p, f, st);
                break;
        case UG_PXF_MATRIX2:
                if (d->format == UG_PF_UYVY) launch<UG_PXF_MATRIX2, UG_PF_UYVY>(p, f, st);
                else if (d->format == UG_PF_Y416) launch<UG_PXF_MATRIX2, UG_PF_Y416>(p, f, st);
                else launch<UG_PXF_MATRIX2, UG_PF_V210>(p, f, st);
                break;
        case UG_PXF_LUT:
                if (d->format == UG_PF_RGB) out_format == UG_PF_RGB ? launch<UG_PXF_LUT, LUT_8_8>(p, f, st) : launch<UG_PXF_LUT, LUT_8_16>(p, f, st);
#if UG_PXF_LUT16_LDS
                else if (out_format == UG_PF_RG48 ? launch_lut16_lds<LUT_16_16>(p, f, st) : launch_lut16_lds<LUT_16_8>(p, f, st)) break;
#endif
                else out_format == UG_PF_RG48 ? launch<UG_PXF_LUT, LUT_16_16>(p, f, st) : launch<UG_PXF_LUT, LUT_16_8>(p, f, st);
                break;
        case UG_PXF_GRAY: launch<UG_PXF_GRAY, UG_PF_UYVY>(p, f, st); break;
        case UG_PXF_MIRROR: launch<UG_PXF_MIRROR, UG_PF_UYVY>(p, f, st); break;
        default: launch<UG_PXF_FLIP, UG_PF_NONE>(p, f, st); break;
        }
        UG_HIP_LAUNCH_CHECK();
        return UG_HIP_SUCCESS;
}
