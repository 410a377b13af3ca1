// compose.hip -- ug_hip_compose: the reference's geometric and compositing per-frame filters on gfx950.
//
//   UG_CMP_CROP           src/vo_postprocess/crop.c:159-182 (`-p crop`, capture filter `crop`): line y = line_bytes bytes of source line yoff + y from
//                         byte xoff_bytes; ug_hip_crop_geometry is :141-148 and :170-173 (double get_bpp arithmetic, whole pixel blocks)
//   UG_CMP_BORDER         src/vo_postprocess/border.c:158-208 (`-p border`): the frame with border_h lines at the top and bottom and border_w pixels at
//                         either side filled with a 4-byte pattern (RGB: its first 3 bytes; UYVY: one U Y V Y word, rows filled over the whole line
//                         size, sides ceil(border_w / 2) pairs from each end, :177-186); ug_hip_border_pattern is :161-166
//   UG_CMP_LOGO           src/capture_filter/logo.c:182-230 (`--capture-filter logo`): an R,G,B,A overlay blended into the frame in place, per pixel
//                         decoder to 8-bit RGB (shifts 0, 8, 16) -> c = (c * (255 - a) + l * a) / 255 -> coder back; ug_hip_logo_geometry is :182-196
//   UG_CMP_INTERLACE      src/vo_postprocess/interlace.c:172-181 (`-p interlace`): line i of src for even i, of src2 for odd i
//   UG_CMP_INTERLACED_3D  src/vo_postprocess/3d-interlaced.c:152-169 (`-p interlaced_3d`): line x = pavgb of lines (x / 2) * 2 and (x / 2) * 2 + 1 of eye
//                         x % 2 (src = tile 0, src2 = tile 1), on BYTES whatever the format (wrong for v210's 10-bit fields there, and reproduced)
//   UG_CMP_SPLIT          src/utils/vf_split.cpp:79-108 (`-p split:X:Y`): tile (tx, ty) = tile_width * get_bpp bytes per line from byte tx * that
//
// Where the reference leaves its buffers: slips that stay inside the frame are reproduced, the others are deviations or refusals.
//   logo.c:198-222      the RGB segment holds dec_width = (lw + 1) / bb * bb pixels per line, lw are blended: for dec_width < lw (lw % 4 in {1, 2}
//                       on UYVY / RGBA, lw % 3 == 1 on RGB, lw % 6 not in {0, 5} on RG48) the blend runs into the next line's segment and past the
//                       malloc.  DEVIATION: every logo pixel is blended over its own decoded frame pixel (what the other widths compute).
//   logo.c:185-196      rect_x = W - lw is rounded with C's division toward zero, so a logo up to bb - 1 pixels WIDER than the frame ends at
//                       rect_x = 0 and is drawn across the line ends (and a logo higher than the frame is caught, one wider is not).  The geometry
//                       helper states the arithmetic; ug_hip_compose REFUSES a rectangle that leaves the frame.
//   3d-interlaced.c:157-168  the output advances 16 bytes per step across lines: a line size that is no multiple of 16 shears and overruns it; an odd
//                       height reads line H of a tile.  DEVIATION: lines at dst_pitch, linesize bytes each; odd `lines` REFUSED.
//   border.c:158,181-184,203-206  2 * border_h > H: memcpy of a negative length; border_w > W: writes in front of the line.  REFUSED.
//   crop.c:176-178      copies req_pitch bytes per line, not the output's line size (the same wherever the caller passes the line size, as the
//                       capture filter does, :227).  Here: line_bytes bytes, and xoff_bytes + line_bytes beyond the source line (v210: a line size
//                       padded to 48 pixels read from an offset) is REFUSED.
//
// Layout, as pixel_filter.hip: a lane owns one 16-byte unit of a destination line; a workgroup is 64 units x 4 lines, grid.y the rest of the lines,
// grid.z the frame.  A whole unit at a multiple of 16 moves as dwordx4, anything else word by word (multiples of 4) or byte by byte, so every
// pointer, pitch and stride is taken; bytes of a destination line past the written size keep their content.  These ops work in bytes: no element
// alignment is asked (LOGO on RG48: 2).  LOGO is one fused kernel over the logo's rectangle, a lane owning one pair (UYVY) or pixel: no RGB
// intermediate in memory.
#include "ug_common.h"
#include "rgb_yuv_device.h"

#include <string.h>

namespace {

constexpr int kUnitsX = 64, kLinesY = 4;
constexpr ug::Cfs kCfs8Host = UG_CFS8_INIT;

struct Params {
        const uint8_t *src, *src2, *logo;
        uint8_t *dst;
        long spitch, dpitch; // dpitch: SPLIT's tile pitch
        size_t sstride, dstride;
        int line_bytes;      // bytes written per destination line (SPLIT: per tile line)
        int lines;           // destination lines (SPLIT: source lines)
        int xoff, yoff;      // CROP
        int side, band, pat_len; // BORDER: bytes at either end of a line, lines at the top and bottom, bytes of the pattern (3 or 4)
        uint32_t pattern;
        int grid_x, tile_h;  // SPLIT
        size_t tile_stride;
        int logo_w, logo_h, rect_x, rect_y; // LOGO
};

// n bytes (<= 16) from p; the rest of the unit is zero
__device__ __forceinline__ void ld(const uint8_t *p, int n, uint32_t (&w)[4])
{
        const uintptr_t a = (uintptr_t) p;
        if (n == 16 && a % 16 == 0) {
                const uint4 v = *(const uint4 *) p;
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                return;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
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

// bytes [0, n) of the unit to p
__device__ __forceinline__ void st(uint8_t *p, const uint32_t (&w)[4], int n)
{
        const uintptr_t a = (uintptr_t) p;
        if (n == 16 && a % 16 == 0) {
                ug::st_stream((uint4 *) p, make_uint4(w[0], w[1], w[2], w[3]));
                return;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
                if (a % 4 == 0 && 4 * i + 4 <= n) {
                        *(uint32_t *) (p + 4 * i) = w[i];
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) if (4 * i + b < n) p[4 * i + b] = (uint8_t) (w[i] >> (8 * b));
                }
        }
}

template <int OP>
__global__ __launch_bounds__(kUnitsX *kLinesY) void compose_kernel(Params p)
{
        const int y = blockIdx.y * kLinesY + threadIdx.y;
        long u = (long) blockIdx.x * kUnitsX + threadIdx.x;
        if (y >= p.lines) return;
        int tx = 0;
        if constexpr (OP == UG_CMP_SPLIT) {
                const int per_tile = (p.line_bytes + 15) / 16;
                tx = (int) (u / per_tile);
                u %= per_tile;
                if (tx >= p.grid_x) return;
        }
        const long x0 = u * 16;
        if (x0 >= p.line_bytes) return;
        const int n = (int) min(16L, p.line_bytes - x0);
        const size_t sf = (size_t) blockIdx.z * p.sstride;
        uint8_t *d = p.dst + (size_t) blockIdx.z * p.dstride;
        uint32_t w[4];

        if constexpr (OP == UG_CMP_CROP) {
                ld(p.src + sf + (long) (p.yoff + y) * p.spitch + p.xoff + x0, n, w);
                d += (long) y * p.dpitch + x0;
        } else if constexpr (OP == UG_CMP_INTERLACE) {
                ld((y & 1 ? p.src2 : p.src) + sf + (long) y * p.spitch + x0, n, w);
                d += (long) y * p.dpitch + x0;
        } else if constexpr (OP == UG_CMP_INTERLACED_3D) { // (lines is even: y | 1 is a line of the eye)
                const uint8_t *const eye = (y & 1 ? p.src2 : p.src) + sf + x0;
                uint32_t b[4];
                ld(eye + (long) (y & ~1) * p.spitch, n, w);
                ld(eye + (long) (y | 1) * p.spitch, n, b);
#pragma unroll
                for (int i = 0; i < 4; i++) w[i] = __builtin_amdgcn_lerp(w[i], b[i], 0x01010101u); // pavgb: (a + b + 1) >> 1 per byte
                d += (long) y * p.dpitch + x0;
        } else if constexpr (OP == UG_CMP_SPLIT) {
                ld(p.src + sf + (long) y * p.spitch + (long) tx * p.line_bytes + x0, n, w);
                d += (size_t) ((y / p.tile_h) * p.grid_x + tx) * p.tile_stride + (long) (y % p.tile_h) * p.dpitch + x0;
        } else { // BORDER
                const bool row = y < p.band || y >= p.lines - p.band;
                if (row) {
#pragma unroll
                        for (int i = 0; i < 4; i++) w[i] = 0;
                } else {
                        ld(p.src + sf + (long) y * p.spitch + x0, n, w);
                }
                // (per byte, with the pattern's phase carried along: right for 3- and 4-byte patterns alike.  For UYVY and RGBA the pattern is one word, so a
                // unit inside a row band could store that word four times; not done -- border on UYVY measures 1.2-1.28 of its copy twin at 4K)
                if (row || x0 < p.side || x0 + 16 > p.line_bytes - p.side) {
                        int m = (int) (x0 % p.pat_len);
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                                const long b = x0 + i;
                                if (row || b < p.side || b >= p.line_bytes - p.side) {
                                        const uint32_t v = (p.pattern >> (8 * m)) & 0xffu;
                                        w[i >> 2] = (w[i >> 2] & ~(0xffu << (8 * (i & 3)))) | v << (8 * (i & 3));
                                }
                                m = m + 1 == p.pat_len ? 0 : m + 1;
                        }
                }
                d += (long) y * p.dpitch + x0;
        }
        st(d, w, n);
}

// logo.c:217 on one component
__device__ __forceinline__ int blend(int c, int l, int a) { return (c * (255 - a) + l * a) / 255; }
__device__ __forceinline__ void blend3(uint8_t *c, const uint8_t *l)
{
        const int a = l[3];
#pragma unroll
        for (int i = 0; i < 3; i++) c[i] = (uint8_t) blend(c[i], l[i], a);
}

template <int FMT>
__global__ __launch_bounds__(kUnitsX *kLinesY) void logo_kernel(Params p)
{
        const int y = blockIdx.y * kLinesY + threadIdx.y;
        const int ux = blockIdx.x * kUnitsX + threadIdx.x;
        const int units = FMT == UG_PF_UYVY ? (p.logo_w + 1) / 2 : p.logo_w;
        if (y >= p.logo_h || ux >= units) return;
        uint8_t *const line = p.dst + (size_t) blockIdx.z * p.dstride + (long) (p.rect_y + y) * p.dpitch;
        const uint8_t *const lg = p.logo + ((long) y * p.logo_w) * 4;
        if constexpr (FMT == UG_PF_UYVY) { // vc_copylineUYVYtoRGB -> blend -> vc_copylineRGBtoUYVY on one pair (rect_x is even)
                uint8_t *const q = line + ((long) (p.rect_x / 2) + ux) * 4;
                const bool word = (uintptr_t) q % 4 == 0;
                const uint32_t in = word ? *(const uint32_t *) q : ((uint32_t) q[0] | (uint32_t) q[1] << 8 | (uint32_t) q[2] << 16 | (uint32_t) q[3] << 24);
                const int cu = (int) (in & 0xff) - 128, cv = (int) (in >> 16 & 0xff) - 128;
                uint8_t c[6];
                ug::yuv_to_rgb8(ug::kCfs8.y_scale * ((int) (in >> 8 & 0xff) - 16), cu, cv, c);
                ug::yuv_to_rgb8(ug::kCfs8.y_scale * ((int) (in >> 24) - 16), cu, cv, c + 3);
                blend3(c, lg + 8 * ux);
                if (2 * ux + 1 < p.logo_w) blend3(c + 3, lg + 8 * ux + 4); // an odd width: the last pair's second pixel is decoded and encoded, unblended
                const uint32_t out = ug::rgb_pair_to_uyvy(ug::kCfs8, c[0], c[1], c[2], c[3], c[4], c[5]);
                if (word) {
                        *(uint32_t *) q = out;
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) q[b] = (uint8_t) (out >> (8 * b));
                }
        } else if constexpr (FMT == UG_PF_RGB) { // vc_copylineRGB both ways
                uint8_t *const q = line + ((long) p.rect_x + ux) * 3;
                uint8_t c[3] = { q[0], q[1], q[2] };
                blend3(c, lg + 4 * ux);
                q[0] = c[0], q[1] = c[1], q[2] = c[2];
        } else if constexpr (FMT == UG_PF_RGBA) { // vc_copylineRGBAtoRGB, vc_copylineRGBtoRGBA: alpha comes back as 0xFF
                uint8_t *const q = line + ((long) p.rect_x + ux) * 4;
                uint8_t c[3] = { q[0], q[1], q[2] };
                blend3(c, lg + 4 * ux);
                q[0] = c[0], q[1] = c[1], q[2] = c[2], q[3] = 0xff;
        } else { // RG48: vc_copylineRG48toRGB takes the high bytes, vc_copylineRGBtoRG48 writes them over zero low bytes
                uint8_t *const q = line + ((long) p.rect_x + ux) * 6;
                uint8_t c[3] = { q[1], q[3], q[5] };
                blend3(c, lg + 4 * ux);
                uint16_t *const q16 = (uint16_t *) q;
                q16[0] = (uint16_t) (c[0] << 8), q16[1] = (uint16_t) (c[1] << 8), q16[2] = (uint16_t) (c[2] << 8);
        }
}

// block bytes / pixels of a packed format (video_codec.c:120-206): get_bpp is (double) bb / bp, get_pf_block_bytes is bb
bool block_of(ug_pixfmt_t f, int &bb, int &bp)
{
        switch (f) {
        case UG_PF_RGBA: case UG_PF_VUYA: case UG_PF_R10K: bb = 4; bp = 1; return true;
        case UG_PF_UYVY: case UG_PF_UYVY_RAW: case UG_PF_YUYV: bb = 4; bp = 2; return true;
        case UG_PF_RGB: case UG_PF_BGR: case UG_PF_YUV444: bb = 3; bp = 1; return true;
        case UG_PF_DVS10: case UG_PF_V210: bb = 16; bp = 6; return true;
        case UG_PF_R12L: bb = 36; bp = 8; return true;
        case UG_PF_Y216: bb = 8; bp = 2; return true;
        case UG_PF_Y416: bb = 8; bp = 1; return true;
        case UG_PF_RG48: bb = 6; bp = 1; return true;
        default: return false;
        }
}

bool supported(int op, ug_pixfmt_t f)
{
        int bb, bp;
        switch (op) {
        case UG_CMP_CROP: case UG_CMP_INTERLACE: case UG_CMP_INTERLACED_3D: case UG_CMP_SPLIT: return block_of(f, bb, bp);
        case UG_CMP_BORDER: return f == UG_PF_UYVY || f == UG_PF_RGB || f == UG_PF_RGBA;
        case UG_CMP_LOGO: return f == UG_PF_UYVY || f == UG_PF_RGB || f == UG_PF_RGBA || f == UG_PF_RG48;
        default: return false;
        }
}

bool overlap(const void *a, size_t an, const void *b, size_t bn)
{
        const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
        return x < y + bn && y < x + an;
}

template <int OP> void launch(const Params &p, long units, int frames, hipStream_t st)
{
        const dim3 grid((unsigned) ((units + kUnitsX - 1) / kUnitsX), (unsigned) ((p.lines + kLinesY - 1) / kLinesY), (unsigned) frames);
        hipLaunchKernelGGL((compose_kernel<OP>), grid, dim3(kUnitsX, kLinesY), 0, st, p);
}
template <int FMT> void launch_logo(const Params &p, int frames, hipStream_t st)
{
        const int units = FMT == UG_PF_UYVY ? (p.logo_w + 1) / 2 : p.logo_w;
        const dim3 grid((unsigned) ((units + kUnitsX - 1) / kUnitsX), (unsigned) ((p.logo_h + kLinesY - 1) / kLinesY), (unsigned) frames);
        hipLaunchKernelGGL((logo_kernel<FMT>), grid, dim3(kUnitsX, kLinesY), 0, st, p);
}

int bad(const char *msg)
{
        ug::set_last_error_msg(msg);
        return UG_HIP_EINVAL;
}

} // namespace

extern "C" int ug_hip_compose_supported(int op, ug_pixfmt_t format)
{
        return supported(op, format) ? 1 : 0;
}

extern "C" int ug_hip_crop_geometry(ug_pixfmt_t format, int in_w, int in_h, int want_w, int want_h, int xoff, int yoff, int *out_w, int *out_h,
                                    int *xoff_bytes, int *yoff_out)
{
        int bb, bp;
        if (!block_of(format, bb, bp)) {
                ug::set_last_error_msg("ug_hip_crop_geometry: not a packed format");
                return UG_HIP_EUNSUPP;
        }
        if (!ug::dims_ok(in_w, in_h) || want_w < 0 || want_h < 0 || want_w > ug::kMaxDim || want_h > ug::kMaxDim || xoff < 0 || yoff < 0 || xoff > ug::kMaxDim ||
            yoff > ug::kMaxDim || out_w == nullptr || out_h == nullptr || xoff_bytes == nullptr || yoff_out == nullptr) {
                return bad("ug_hip_crop_geometry: frame 1..65536 each way, size and offsets 0..65536, four places for the results");
        }
        const double bpp = (double) bb / bp; // get_bpp, video_codec.c:309-320
        int w = want_w ? (want_w < in_w ? want_w : in_w) : in_w;
        const int h = want_h ? (want_h < in_h ? want_h : in_h) : in_h;
        const int linesize = (int) (w * bpp) / bb * bb; // crop.c:146-148
        w = (int) (linesize / bpp);
        const int xo = xoff + w > in_w ? in_w - w : xoff; // :170-173
        *xoff_bytes = (int) (xo * bpp) / bb * bb;
        *yoff_out = yoff + h > in_h ? in_h - h : yoff;
        *out_w = w;
        *out_h = h;
        return UG_HIP_SUCCESS;
}

extern "C" int ug_hip_logo_geometry(ug_pixfmt_t format, int frame_w, int frame_h, int logo_w, int logo_h, int x, int y, int *rect_x, int *rect_y)
{
        int bb, bp;
        if (!block_of(format, bb, bp)) {
                ug::set_last_error_msg("ug_hip_logo_geometry: not a packed format");
                return UG_HIP_EUNSUPP;
        }
        if (!ug::dims_ok(frame_w, frame_h) || !ug::dims_ok(logo_w, logo_h) || x < -ug::kMaxDim || x > ug::kMaxDim || y < -ug::kMaxDim || y > ug::kMaxDim ||
            rect_x == nullptr || rect_y == nullptr) {
                return bad("ug_hip_logo_geometry: frame and logo 1..65536 each way, position within +-65536, two places for the results");
        }
        int rx = x, ry = y; // logo.c:182-193
        if (rx < 0 || rx + logo_w > frame_w) rx = frame_w - logo_w;
        rx = rx / bb * bb; // a pixel position rounded by the block's BYTE count, toward zero
        if (ry < 0 || ry + logo_h > frame_h) ry = frame_h - logo_h;
        *rect_x = rx;
        *rect_y = ry;
        return UG_HIP_SUCCESS;
}

extern "C" int ug_hip_border_pattern(ug_pixfmt_t format, const unsigned char rgba[4], unsigned char out[4])
{
        if (rgba == nullptr || out == nullptr) return bad("ug_hip_border_pattern: NULL pointer");
        if (format == UG_PF_RGB || format == UG_PF_RGBA) {
                memcpy(out, rgba, 4);
                return UG_HIP_SUCCESS;
        }
        if (format != UG_PF_UYVY) {
                ug::set_last_error_msg("ug_hip_border_pattern: UYVY, RGB or RGBA");
                return UG_HIP_EUNSUPP;
        }
        // border.c:161-166: vc_copylineRGBAtoUYVY over two copies of the colour, 4 bytes out
        const uint32_t w = ug::rgb_pair_to_uyvy(kCfs8Host, rgba[0], rgba[1], rgba[2], rgba[0], rgba[1], rgba[2]);
        for (int b = 0; b < 4; b++) out[b] = (unsigned char) (w >> (8 * b));
        return UG_HIP_SUCCESS;
}

extern "C" int ug_hip_compose(const struct ug_compose_desc *d, ug_hip_stream_t stream)
{
        static const char *const who = "ug_hip_compose";
        if (d == nullptr) return bad("ug_hip_compose: NULL descriptor");
        const int op = d->op;
        if (op < UG_CMP_CROP || op > UG_CMP_SPLIT) return bad("ug_hip_compose: op must be one of UG_CMP_*");
        if (!supported(op, d->format)) {
                ug::set_last_error_msg("ug_hip_compose: unsupported format for this op (crop, interlace, interlaced_3d, split: packed formats; border: UYVY, RGB, RGBA; "
                                       "logo: UYVY, RGB, RGBA, RG48)");
                return UG_HIP_EUNSUPP;
        }
        const bool logo = op == UG_CMP_LOGO, two = op == UG_CMP_INTERLACE || op == UG_CMP_INTERLACED_3D;
        if (d->dst == nullptr || (!logo && d->src == nullptr) || (two && d->src2 == nullptr)) return bad("ug_hip_compose: NULL pointer");
        if (logo && d->src != nullptr && d->src != d->dst) return bad("ug_hip_compose: LOGO works in place: src NULL or equal to dst");
        if (!ug::dims_ok(d->width, d->lines)) return ug::refuse_size(who);
        int bb = 0, bp = 0;
        block_of(d->format, bb, bp);
        const long long L = ug::linesize(d->format, d->width);
        if (L <= 0) return ug::refuse_size(who);
        if (d->src_pitch > (size_t) ug::kMaxFrameBytes || d->dst_pitch > (size_t) ug::kMaxFrameBytes || d->tile_pitch > (size_t) ug::kMaxFrameBytes ||
            d->tile_stride > (size_t) ug::kMaxFrameBytes) {
                return ug::refuse_size(who);
        }
        const long long sp = logo ? 0 : (d->src_pitch ? (long long) d->src_pitch : L);
        if (!logo && (sp < L || !ug::span_ok(sp, d->lines))) return ug::refuse_size(who);

        // per op: bytes and lines written, the destination's own pitch, the bytes one destination frame spans
        long long lb = L, ol = d->lines, dp = d->dst_pitch ? (long long) d->dst_pitch : L, dspan = 0, ts = 0;
        long long tiles = 1, tile_h = d->lines;
        Params p = {};
        switch (op) {
        case UG_CMP_CROP:
                if (d->xoff_bytes < 0 || d->yoff < 0 || d->out_line_bytes < 1 || d->out_lines < 1 || (long long) d->xoff_bytes + d->out_line_bytes > L ||
                    (long long) d->yoff + d->out_lines > d->lines) {
                        return bad("ug_hip_compose: CROP needs 0 <= xoff_bytes, xoff_bytes + out_line_bytes <= the source's line size, 0 <= yoff, yoff + out_lines <= lines");
                }
                lb = d->out_line_bytes, ol = d->out_lines;
                dp = d->dst_pitch ? (long long) d->dst_pitch : lb;
                p.xoff = d->xoff_bytes, p.yoff = d->yoff;
                break;
        case UG_CMP_BORDER: {
                if (d->border_w < 0 || d->border_h < 0 || d->border_w > d->width || 2LL * d->border_h > d->lines) {
                        return bad("ug_hip_compose: BORDER needs 0 <= border_w <= width and 0 <= 2 * border_h <= lines (the reference writes outside its frame beyond)");
                }
                p.band = d->border_h;
                p.pat_len = d->format == UG_PF_RGB ? 3 : 4;
                p.side = d->format == UG_PF_UYVY ? (d->border_w + 1) / 2 * 4 : d->border_w * p.pat_len;
                memcpy(&p.pattern, d->fill, 4);
                break;
        }
        case UG_CMP_INTERLACED_3D:
                if (d->lines % 2) return bad("ug_hip_compose: INTERLACED_3D needs an even number of lines (the reference reads line H of a tile)");
                break;
        case UG_CMP_SPLIT: {
                if (d->grid_x < 1 || d->grid_y < 1 || d->width % d->grid_x || d->lines % d->grid_y) {
                        return bad("ug_hip_compose: SPLIT needs a grid that divides width and lines (the reference asserts it)");
                }
                const int tile_w = d->width / d->grid_x;
                if (bb % bp ? tile_w % bp != 0 : false) {
                        ug::set_last_error_msg("ug_hip_compose: SPLIT of v210 / R12L needs tiles of whole pixel blocks (tile_width * get_bpp is no whole number of bytes otherwise)");
                        return UG_HIP_EUNSUPP;
                }
                tile_h = d->lines / d->grid_y;
                tiles = (long long) d->grid_x * d->grid_y;
                lb = (long long) tile_w * bb / bp;
                dp = d->tile_pitch ? (long long) d->tile_pitch : ug::linesize(d->format, tile_w);
                if (dp < lb || !ug::span_ok(dp, tile_h)) return ug::refuse_size(who);
                ts = d->tile_stride ? (long long) d->tile_stride : dp * tile_h;
                if (ts < dp * tile_h || ts > ug::kMaxFrameBytes / tiles) return bad("ug_hip_compose: SPLIT needs tile_stride 0 or at least a tile, all tiles within INT_MAX bytes");
                p.grid_x = d->grid_x, p.tile_h = (int) tile_h, p.tile_stride = (size_t) ts;
                break;
        }
        case UG_CMP_LOGO:
                if (d->logo == nullptr) return bad("ug_hip_compose: LOGO needs the overlay");
                if (!ug::dims_ok(d->logo_w, d->logo_h)) return ug::refuse_size(who);
                if (d->rect_x >= 0 && d->rect_y >= 0 && ((long long) d->rect_x + d->logo_w > d->width || (long long) d->rect_y + d->logo_h > d->lines)) {
                        return bad("ug_hip_compose: LOGO's rectangle leaves the frame (the reference's rounding lets a logo up to block bytes - 1 wider than the frame through)");
                }
                if (d->format == UG_PF_UYVY && d->rect_x > 0 && d->rect_x % 2) return bad("ug_hip_compose: LOGO on UYVY needs an even rect_x (ug_hip_logo_geometry gives multiples of 4)");
                break;
        default: break;
        }
        if (op != UG_CMP_SPLIT) {
                if (dp < lb || !ug::span_ok(dp, ol)) return ug::refuse_size(who);
                dspan = dp * ol;
        } else {
                dspan = ts * (tiles - 1) + dp * tile_h;
        }
        const size_t e = logo && d->format == UG_PF_RG48 ? 2 : 1;
        const size_t sspan = (size_t) (sp * d->lines);
        if (d->frames < 1 || d->frames > 65535 ||
            (d->frames > 1 && ((!logo && d->src_frame_stride < sspan) || d->dst_frame_stride < (size_t) dspan || d->dst_frame_stride % e ||
                               d->src_frame_stride > SIZE_MAX / (size_t) d->frames || d->dst_frame_stride > SIZE_MAX / (size_t) d->frames))) {
                return bad("ug_hip_compose: frames 1..65535, strides that cover a frame (LOGO on RG48: multiples of 2)");
        }
        if ((uintptr_t) d->dst % e || (size_t) dp % e) return bad("ug_hip_compose: LOGO on RG48 needs a pointer and a pitch that are multiples of 2");
        const size_t sstride = d->frames > 1 && !logo ? d->src_frame_stride : 0, dstride = d->frames > 1 ? d->dst_frame_stride : 0;
        const size_t sall = sstride * (size_t) (d->frames - 1) + sspan, dall = dstride * (size_t) (d->frames - 1) + (size_t) dspan;
        if (logo) {
                if (overlap(d->logo, (size_t) d->logo_w * d->logo_h * 4, d->dst, dall)) return bad("ug_hip_compose: the overlay and the frame must not overlap");
                if (d->rect_x < 0 || d->rect_y < 0) return UG_HIP_SUCCESS; // logo.c:195-196: the frame as it is
        } else if (overlap(d->src, sall, d->dst, dall) || (two && overlap(d->src2, sall, d->dst, dall))) {
                return bad("ug_hip_compose: source and destination must not overlap");
        }
        p.src = (const uint8_t *) d->src;
        p.src2 = (const uint8_t *) d->src2;
        p.logo = (const uint8_t *) d->logo;
        p.dst = (uint8_t *) d->dst;
        p.spitch = (long) sp;
        p.dpitch = (long) dp;
        p.sstride = sstride;
        p.dstride = dstride;
        p.line_bytes = (int) lb;
        p.lines = op == UG_CMP_SPLIT ? d->lines : (int) ol;
        p.logo_w = d->logo_w, p.logo_h = d->logo_h, p.rect_x = d->rect_x, p.rect_y = d->rect_y;
        hipStream_t st = (hipStream_t) stream;
        const int f = d->frames;
        const long units = (lb + 15) / 16;
        switch (op) {
        case UG_CMP_CROP: launch<UG_CMP_CROP>(p, units, f, st); break;
        case UG_CMP_BORDER: launch<UG_CMP_BORDER>(p, units, f, st); break;
        case UG_CMP_INTERLACE: launch<UG_CMP_INTERLACE>(p, units, f, st); break;
        case UG_CMP_INTERLACED_3D: launch<UG_CMP_INTERLACED_3D>(p, units, f, st); break;
        case UG_CMP_SPLIT: launch<UG_CMP_SPLIT>(p, units * d->grid_x, f, st); break;
        default:
                if (d->format == UG_PF_UYVY) launch_logo<UG_PF_UYVY>(p, f, st);
                else if (d->format == UG_PF_RGB) launch_logo<UG_PF_RGB>(p, f, st);
                else if (d->format == UG_PF_RGBA) launch_logo<UG_PF_RGBA>(p, f, st);
                else launch_logo<UG_PF_RG48>(p, f, st);
                break;
        }
        UG_HIP_LAUNCH_CHECK();
        return UG_HIP_SUCCESS;
}
