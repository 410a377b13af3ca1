// deinterlace_ex.hip -- ug_hip_deinterlace: the reference's de-interlacing postprocessors on gfx950.
//
//   UG_DEINT_BLEND   vc_deinterlace_ex (src/video_codec.c:722-854; `-p deinterlace`, `-p deinterlace_blend`): out of place (or dst == src),
//                    line y = rounded average of lines y and y + 1, the last line = the line above it
//   UG_DEINT_WEAVE   perform_df (src/vo_postprocess/temporal-deint.c:240-277; `-p double_framerate[:d]`): output 0 = even lines of this
//                    frame + odd lines of the previous one, output 1 = this frame; `:d` = vc_deinterlace_ex over each, fused here
//   UG_DEINT_BOB     perform_bob (:279-300): output 0 = every even line twice, output 1 = every odd line twice (shifted by one line)
//   UG_DEINT_LINEAR  perform_linear (:442-466): as bob, the missing lines interpolated by avg_lines (:307-440)
//
// Arithmetic, restated from the reference (tests/deinterlace_restatement.py states the same in numpy):
//   vc_deinterlace_ex  (a + b + 1) >> 1 per element: bytes (v_lerp_u8), uint16_t, v210's fields of 10 / 10 / 12 bits (the third is `v >> 20`,
//                      bits 30-31 included), R10k's big-endian fields at bits 22 / 12 / 2 (the low two bits of every output word are zero),
//                      R12L's continuous stream of 12-bit samples.  All but the bytes as (a | b) - (((a ^ b) & ~lsb) >> 1), `lsb` holding the
//                      lowest bit of every field: no carry crosses a field, so R12L's fields that straddle words need nothing but a 96-bit
//                      shift and subtraction per 3 words = 8 samples.
//   avg_lines_per_elem (8- and 16-bit formats of deinterlace_linear) is NOT that average: (c1 >> 1) + (c2 >> 1) + (c1 & 1), c1 the upper line
//                      (temporal-deint.c:318-319,334-335: `(c1 % 2 + c1 % 2) / 2`).  The reference's shipped behaviour is the pin, reproduced.
//                      v210 / R10k / R12L of avg_lines are vc_deinterlace_ex's average.
// How much of a line an averaged line writes follows the reference's loop bounds (written_bytes() below); the rest of such a destination
// line keeps its bytes (WEAVE + blend: the woven bytes, as the reference blends in place).
//
// Layout.  A lane owns a 16-byte column chunk (R12L: 48 bytes = four 3-word groups) and walks a band of 16 output lines (8 or 4 where a
// single small picture would leave the GPU short of waves), keeping the one or two lines above in registers: every source line is
// fetched once per band (bands overlap by one line, LINEAR by two; the four bands of a workgroup are neighbours, so the shared lines come from
// L2 -- measured HBM traffic 1.00 x the algorithmic bytes, profiles/r12_deinterlace_ex.txt) and every output byte stored once, both outputs of
// a two-output filter from the same registers.  A workgroup is 64 chunks x 4 bands; grid.z = frame.  Where every pointer, pitch and stride is
// a multiple of 16 a chunk moves as dwordx4 -- R12L's three per lane as one contiguous region per wave, through LDS --; otherwise word by word
// (multiples of 4) or byte by byte, which is also the path of the last, partial chunk of a line.  dst == src (BLEND) runs one band per
// column: a band's last line needs the line below it as it was.
#include "ug_common.h"

namespace {

enum Cls { C8, C16, CV210, CR10K, CR12L };
constexpr int kBand = 16, kMinBand = 4; // output lines per lane (even: WEAVE / BOB / LINEAR pair lines up)
constexpr long kWantLanes = 256L * 4 * 4 * 64; // four waves on every SIMD of 256 CUs
constexpr int kChunksX = 64, kBandsY = 4;

template <int NW> struct alignas(16) Chunk { uint32_t w[NW]; };

struct Params {
        const uint8_t *src, *prev;
        uint8_t *dst0, *dst1;
        long spitch, dpitch;
        size_t sstride, dstride;
        int linesize, lines, wbytes, band, amode, blend;
};

// n bytes (<= 4 * NW) from p; the rest of the chunk is zero
template <int NW> __device__ __forceinline__ Chunk<NW> ld(const uint8_t *p, int n, int amode)
{
        Chunk<NW> c;
        if (amode == 16 && n == 4 * NW) {
#pragma unroll
                for (int i = 0; i < NW / 4; i++) {
                        const uint4 v = ((const uint4 *) p)[i];
                        c.w[4 * i] = v.x; c.w[4 * i + 1] = v.y; c.w[4 * i + 2] = v.z; c.w[4 * i + 3] = v.w;
                }
                return c;
        }
#pragma unroll
        for (int i = 0; i < NW; i++) {
                uint32_t v = 0;
                if (amode >= 4 && 4 * i + 4 <= n) {
                        v = *(const uint32_t *) (p + 4 * i);
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) if (4 * i + b < n) v |= (uint32_t) p[4 * i + b] << (8 * b);
                }
                c.w[i] = v;
        }
        return c;
}

// bytes [lo, hi) of the chunk to p + lo ...
template <int NW> __device__ __forceinline__ void st(uint8_t *p, const Chunk<NW> &c, int lo, int hi, int amode)
{
        if (amode == 16 && lo == 0 && hi == 4 * NW) {
#pragma unroll
                for (int i = 0; i < NW / 4; i++) ug::st_stream((uint4 *) p + i, make_uint4(c.w[4 * i], c.w[4 * i + 1], c.w[4 * i + 2], c.w[4 * i + 3]));
                return;
        }
#pragma unroll
        for (int i = 0; i < NW; i++) {
                if (amode >= 4 && 4 * i >= lo && 4 * i + 4 <= hi) {
                        ug::st_stream((uint32_t *) (p + 4 * i), c.w[i]);
                } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) if (4 * i + b >= lo && 4 * i + b < hi) p[4 * i + b] = (uint8_t) (c.w[i] >> (8 * b));
                }
        }
}

// per field (a + b + 1) >> 1, `lsb` = the lowest bit of every field of the word
__device__ __forceinline__ uint32_t avg_fields(uint32_t a, uint32_t b, uint32_t lsb) { return (a | b) - (((a ^ b) & ~lsb) >> 1); }

// the average of two lines' chunks; LIN: avg_lines (a = the upper line), else vc_deinterlace_ex
template <Cls C, bool LIN, int NW> __device__ __forceinline__ Chunk<NW> avg(const Chunk<NW> &a, const Chunk<NW> &b)
{
        Chunk<NW> r;
        if (C == CR12L) {
#pragma unroll
                for (int g = 0; g < NW / 3; g++) {
                        const uint32_t a0 = a.w[3 * g], a1 = a.w[3 * g + 1], a2 = a.w[3 * g + 2], b0 = b.w[3 * g], b1 = b.w[3 * g + 1], b2 = b.w[3 * g + 2];
                        // samples start at bits 0, 12, 24 | 36, 48, 60 | 72, 84 of the 96
                        const uint32_t x0 = (a0 ^ b0) & ~0x01001001u, x1 = (a1 ^ b1) & ~0x10010010u, x2 = (a2 ^ b2) & ~0x00100100u;
                        const uint64_t f = (uint64_t) (a0 | b0) | (uint64_t) (a1 | b1) << 32;
                        const uint64_t t = (uint64_t) ((x0 >> 1) | (x1 << 31)) | (uint64_t) ((x1 >> 1) | (x2 << 31)) << 32;
                        const uint64_t lo = f - t;
                        r.w[3 * g] = (uint32_t) lo;
                        r.w[3 * g + 1] = (uint32_t) (lo >> 32);
                        r.w[3 * g + 2] = (a2 | b2) - (x2 >> 1) - (f < t ? 1u : 0u);
                }
                return r;
        }
#pragma unroll
        for (int i = 0; i < NW; i++) {
                const uint32_t x = a.w[i], y = b.w[i];
                if (C == C8) {
                        r.w[i] = LIN ? ((x >> 1) & 0x7F7F7F7Fu) + ((y >> 1) & 0x7F7F7F7Fu) + (x & 0x01010101u) : __builtin_amdgcn_lerp(x, y, 0x01010101u);
                } else if (C == C16) {
                        r.w[i] = LIN ? ((x >> 1) & 0x7FFF7FFFu) + ((y >> 1) & 0x7FFF7FFFu) + (x & 0x00010001u) : avg_fields(x, y, 0x00010001u);
                } else if (C == CV210) {
                        r.w[i] = avg_fields(x, y, 0x00100401u);
                } else { // CR10K
                        // avg_lines reads with ntohl and stores the host-order word (temporal-deint.c:388-393): LINEAR's averaged lines are byte-swapped
                        const uint32_t v = avg_fields(__builtin_bswap32(x) & ~3u, __builtin_bswap32(y) & ~3u, 0x00401004u);
                        r.w[i] = LIN ? v : __builtin_bswap32(v);
                }
        }
        return r;
}

// word by word (a select between whole chunks would go through scratch memory)
template <int NW> __device__ __forceinline__ Chunk<NW> sel(bool first, const Chunk<NW> &a, const Chunk<NW> &b)
{
        Chunk<NW> r;
#pragma unroll
        for (int i = 0; i < NW; i++) r.w[i] = first ? a.w[i] : b.w[i];
        return r;
}

template <Cls C, int MODE> __global__ __launch_bounds__(kChunksX *kBandsY) void deinterlace_ex_kernel(Params p)
{
        constexpr int NW = C == CR12L ? 12 : 4, CB = 4 * NW;
        using Ch = Chunk<NW>;
        using IO = ug::UnitIO<CB>;
        // R12L's 48-byte chunks, lane by lane, would make every load and store instruction touch 64 lines and use a third of each: where everything
        // is 16-byte aligned the wave moves its 64 chunks as one contiguous region instead, the words changing hands through LDS (ug_common.h)
        constexpr bool kCoop = IO::V > 1;
        __shared__ uint4 s_io[kCoop ? kBandsY * IO::LDS_WORDS : 1];
        const int lane = threadIdx.x;
        const long wave_x0 = (long) blockIdx.x * kChunksX * CB, x0 = wave_x0 + (long) lane * CB;
        const int H = p.lines;
        const int y0 = (int) (blockIdx.y * kBandsY + threadIdx.y) * p.band;
        const int am = p.amode;
        const bool coop = kCoop && am == 16; // (then lanes past the end of the line stay: they move words for the others)
        if (y0 >= H || wave_x0 >= p.linesize || (!coop && x0 >= p.linesize)) return;
        const int y1 = min(y0 + p.band, H);
        const int nL = (int) max(0L, min((long) CB, p.linesize - x0));   // bytes of the chunk inside the line
        const int nW = (int) max(0L, min((long) CB, p.wbytes - x0));     // ... that an averaged line writes
        uint4 *const lds = s_io + (kCoop ? threadIdx.y * IO::LDS_WORDS : 0);
        auto whole = [&](long total) { return (int) max(0L, min(64L, (total - wave_x0) / CB)); }; // the wave's chunks that lie whole in `total` bytes
        const int uL = whole(p.linesize);
        // a line's chunk (every lane of the wave calls these together)
        auto LD = [&](const uint8_t *q) {
                Ch c;
                if (coop) {
                        IO::load((const uint4 *) (q - (long) lane * CB), (uint8_t *) c.w, lds, lane, uL);
                        if (lane >= uL) c = ld<NW>(q, nL, am);
                } else {
                        c = ld<NW>(q, nL, am);
                }
                return c;
        };
        // the chunk's bytes below `total` (the line size, or what an averaged line writes)
        auto ST = [&](uint8_t *q, const Ch &c, int total) {
                const int n = (int) max(0L, min((long) CB, total - x0));
                if (coop) {
                        const int u = whole(total);
                        IO::store((uint4 *) (q - (long) lane * CB), (const uint8_t *) c.w, lds, lane, u);
                        if (lane >= u) st<NW>(q, c, 0, n, am);
                } else {
                        st<NW>(q, c, 0, n, am);
                }
        };
        const uint8_t *const s = p.src + (size_t) blockIdx.z * p.sstride + x0;
        uint8_t *const d0 = p.dst0 + (size_t) blockIdx.z * p.dstride + x0;
        auto S = [&](int y) { return LD(s + (long) y * p.spitch); };
        auto D0 = [&](int y) { return d0 + (long) y * p.dpitch; };
        if (MODE == UG_DEINT_BLEND) {
                if (H == 1) { // vc_deinterlace_ex copies a single line
                        ST(D0(0), S(0), p.linesize);
                        return;
                }
                Ch a, o;
                if (y0 == H - 1) o = avg<C, false, NW>(S(H - 2), S(H - 1));
                else a = S(y0);
                for (int y = y0; y < y1; y++) {
                        if (y < H - 1) {
                                const Ch b = S(y + 1);
                                o = avg<C, false, NW>(a, b);
                                a = b;
                                ST(D0(y), o, p.wbytes);
                        } else { // the last line: the L bytes of the destination's line above (:851)
                                ST(D0(y), o, p.wbytes);
                                if (nW < nL) st<NW>(D0(y), ld<NW>(D0(H - 2), nL, am), nW, nL, am);
                        }
                }
                return;
        }
        uint8_t *const d1 = p.dst1 + (size_t) blockIdx.z * p.dstride + x0;
        auto D1 = [&](int y) { return d1 + (long) y * p.dpitch; };
        if (MODE == UG_DEINT_WEAVE) {
                const uint8_t *const q = p.prev + (size_t) blockIdx.z * p.sstride + x0;
                auto Q = [&](int y) { return LD(q + (long) y * p.spitch); };
                if (!p.blend) {
                        for (int y = y0; y < y1; y++) {
                                const Ch c = S(y);
                                ST(D1(y), c, p.linesize);
                                ST(D0(y), (y & 1) ? Q(y) : c, p.linesize);
                        }
                        return;
                }
                // vc_deinterlace_ex in place over each woven frame: bytes past the averaged part keep the woven line (H is even: y0 < H - 1)
                auto emit = [&](uint8_t *line, const Ch &o, const Ch &bg) {
                        ST(line, o, p.wbytes);
                        if (nW < nL) st<NW>(line, bg, nW, nL, am);
                };
                Ch c = S(y0), w = (y0 & 1) ? Q(y0) : c, o0 = c, o1 = c, bw = c, bc = c;
                for (int y = y0; y < y1; y++) {
                        if (y < H - 1) {
                                const Ch cn = S(y + 1), wn = ((y + 1) & 1) ? Q(y + 1) : cn;
                                o0 = avg<C, false, NW>(w, wn);
                                o1 = avg<C, false, NW>(c, cn);
                                emit(D0(y), o0, w);
                                emit(D1(y), o1, c);
                                bw = w; bc = c;
                                w = wn; c = cn;
                        } else {
                                emit(D0(y), o0, bw);
                                emit(D1(y), o1, bc);
                        }
                }
                return;
        }
        if (MODE == UG_DEINT_BOB) {
                int ie = -1, io = -1;
                Ch ce, co;
                for (int y = y0; y < y1; y++) {
                        int i0 = y & ~1, i1 = y == 0 ? 1 : ((y - 1) & ~1) + 1;
                        if (y == H - 1) { // "memcpy(dst, dst - pitch)" (:297-299): the line above once more
                                if (H & 1) i0 = H - 3;
                                else i1 = H == 2 ? 1 : H - 3;
                        }
                        if (i0 != ie) { ce = S(i0); ie = i0; }
                        if (i1 != io) { co = S(i1); io = i1; }
                        ST(D0(y), ce, p.linesize);
                        ST(D1(y), co, p.linesize);
                }
                return;
        }
        if (MODE == UG_DEINT_LINEAR) {
                // output 0: odd lines below 2 * n0 are averages; output 1: line 0 = line 1, even lines 2 .. 2 * n1 are averages; the rest copies --
                // where two lines are left at the bottom both are the first of them (the reference's source pointer stands still, :462-465)
                const int n0 = (H - 1) / 2, n1 = (H - 2) / 2;
                Ch b = S(y0), a = y0 > 0 ? S(y0 - 1) : b;
                for (int y = y0; y < y1; y++) {
                        const Ch c = y + 1 < H ? S(y + 1) : b;
                        const bool av0 = (y & 1) && y < 2 * n0, av1 = !(y & 1) && y >= 2 && y <= 2 * n1;
                        Ch m = b;
                        if (av0 || av1) m = avg<C, true, NW>(a, c);
                        if (av0) ST(D0(y), m, p.wbytes);
                        else ST(D0(y), sel(y > 2 * n0, a, b), p.linesize);
                        if (av1) ST(D1(y), m, p.wbytes);
                        else ST(D1(y), sel(y == 0, c, sel(y > 2 * n1 + 1, a, b)), p.linesize);
                        a = b;
                        b = c;
                }
        }
}

int cls_of(ug_pixfmt_t f)
{
        switch (f) {
        case UG_PF_RGBA: case UG_PF_UYVY: case UG_PF_YUYV: case UG_PF_RGB: case UG_PF_BGR: case UG_PF_VUYA: return C8;
        case UG_PF_RG48: case UG_PF_Y216: case UG_PF_Y416: return C16;
        case UG_PF_V210: return CV210;
        case UG_PF_R10K: return CR10K;
        case UG_PF_R12L: return CR12L;
        default: return -1;
        }
}

// The bytes of a line that an averaged line writes: the reference's loop bounds.
//   vc_deinterlace_ex: v210 / R10k linesize / 16 groups of 4 words (:778,794); R12L linesize / 36 groups of EIGHT words (:814-816 -- a 36-byte
//   group is nine: the last ninth of a line is never reached), of which the last is written only if it ends on a sample boundary.
//   avg_lines: v210 linesize / 16 groups of 4 words (:370); R12L linesize / 16 groups of 4 words (:404); R10k walks four lines' worth (:385-387),
//   not reproducible in bounds: the one line here.  8- and 16-bit: the line (avg_lines_per_elem rounds up to 16 bytes, past the line: not here).
long written_bytes(int cls, bool linear, long L)
{
        switch (cls) {
        // the x86-64 build's 16-bit tail loop (:759,769) compares a BYTE offset with the number of elements and so never runs after a vector loop
        // that ran: from 16 bytes on, the linesize % 16 bytes behind the last whole vector are not written (the reference builds with -msse4.1)
        case C16: return linear || L < 16 ? L : L / 16 * 16;
        case CV210: return L / 16 * 16;
        case CR10K: return linear ? L : L / 16 * 16;
        case CR12L: {
                const long n = linear ? L / 16 * 4 : L / 36 * 8;
                return 4 * (n - (n % 3 != 0));
        }
        default: return L;
        }
}

template <Cls C> void launch(int mode, dim3 grid, hipStream_t st, const Params &p)
{
        const dim3 block(kChunksX, kBandsY);
        switch (mode) {
        case UG_DEINT_BLEND: hipLaunchKernelGGL((deinterlace_ex_kernel<C, UG_DEINT_BLEND>), grid, block, 0, st, p); break;
        case UG_DEINT_WEAVE: hipLaunchKernelGGL((deinterlace_ex_kernel<C, UG_DEINT_WEAVE>), grid, block, 0, st, p); break;
        case UG_DEINT_BOB: hipLaunchKernelGGL((deinterlace_ex_kernel<C, UG_DEINT_BOB>), grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL((deinterlace_ex_kernel<C, UG_DEINT_LINEAR>), grid, block, 0, st, p); break;
        }
}

bool overlap(const void *a, size_t an, const void *b, size_t bn)
{
        const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
        return x < y + bn && y < x + an;
}

} // namespace

extern "C" int ug_hip_deinterlace_supported(ug_pixfmt_t format, int mode)
{
        return cls_of(format) >= 0 && mode >= UG_DEINT_BLEND && mode <= UG_DEINT_LINEAR ? 1 : 0;
}

extern "C" int ug_hip_deinterlace(const struct ug_deinterlace_desc *d, ug_hip_stream_t stream)
{
        auto bad = [](const char *msg) { ug::set_last_error_msg(msg); return UG_HIP_EINVAL; };
        if (d == nullptr) return bad("ug_hip_deinterlace: NULL descriptor");
        if (d->mode < UG_DEINT_BLEND || d->mode > UG_DEINT_LINEAR) return bad("ug_hip_deinterlace: mode must be UG_DEINT_BLEND / _WEAVE / _BOB / _LINEAR");
        const int cls = cls_of(d->format);
        if (cls < 0) {
                ug::set_last_error_msg("ug_hip_deinterlace: 8- and 16-bit packed formats, v210, R10k and R12L only (vc_deinterlace_ex returns false for the rest)");
                return UG_HIP_EUNSUPP;
        }
        const int mode = d->mode;
        const bool two = mode != UG_DEINT_BLEND;
        if (d->src == nullptr || d->dst[0] == nullptr || (two && d->dst[1] == nullptr) || (mode == UG_DEINT_WEAVE && d->prev == nullptr)) {
                return bad("ug_hip_deinterlace: NULL pointer (src, dst[0]; dst[1] unless BLEND; prev for WEAVE)");
        }
        if (d->lines < 1 || d->lines > ug::kMaxDim || d->linesize < 1 || d->linesize > 8ull * ug::kMaxDim) return ug::refuse_size("ug_hip_deinterlace");
        if (two && d->lines < 2) return bad("ug_hip_deinterlace: WEAVE, BOB and LINEAR need at least 2 lines (the reference reads in front of its buffers below that)");
        if (mode == UG_DEINT_WEAVE && d->lines % 2 != 0) {
                return bad("ug_hip_deinterlace: WEAVE needs an even number of lines (perform_df copies one line past both buffers otherwise)");
        }
        const size_t unit = cls == C8 ? 1 : cls == C16 ? 2 : 4;
        const long long L = (long long) d->linesize;
        if (d->src_pitch > (size_t) ug::kMaxFrameBytes || d->dst_pitch > (size_t) ug::kMaxFrameBytes) return ug::refuse_size("ug_hip_deinterlace");
        const long long sp = d->src_pitch ? (long long) d->src_pitch : L, dp = d->dst_pitch ? (long long) d->dst_pitch : L;
        if (sp < L || dp < L || !ug::span_ok(sp, d->lines) || !ug::span_ok(dp, d->lines)) return ug::refuse_size("ug_hip_deinterlace");
        if (L % unit || sp % unit || dp % unit) return bad("ug_hip_deinterlace: line size and pitches must be multiples of the format's element (2 bytes: 16-bit formats; 4: v210, R10k, R12L)");
        const size_t sspan = (size_t) (sp * d->lines), dspan = (size_t) (dp * d->lines);
        if (d->frames < 1 || d->frames > 65535 ||
            (d->frames > 1 && (d->src_frame_stride < sspan || d->dst_frame_stride < dspan || d->src_frame_stride % unit || d->dst_frame_stride % unit ||
                               d->src_frame_stride > SIZE_MAX / (size_t) d->frames || d->dst_frame_stride > SIZE_MAX / (size_t) d->frames))) {
                return bad("ug_hip_deinterlace: frames 1..65535, strides multiples of the element that cover a frame");
        }
        const uintptr_t ptrs = (uintptr_t) d->src | (uintptr_t) d->dst[0] | (two ? (uintptr_t) d->dst[1] : 0) | (mode == UG_DEINT_WEAVE ? (uintptr_t) d->prev : 0);
        if (ptrs % unit) return bad("ug_hip_deinterlace: pointers must be aligned to the format's element");
        const size_t sstride = d->frames > 1 ? d->src_frame_stride : 0, dstride = d->frames > 1 ? d->dst_frame_stride : 0;
        const size_t sall = sstride * (size_t) (d->frames - 1) + sspan, dall = dstride * (size_t) (d->frames - 1) + dspan;
        bool in_place = false;
        if (mode == UG_DEINT_BLEND) {
                in_place = d->dst[0] == d->src;
                if (in_place ? (sp != dp || (d->frames > 1 && sstride != dstride)) : overlap(d->src, sall, d->dst[0], dall)) {
                        return bad("ug_hip_deinterlace: BLEND runs out of place or with dst == src at the same pitch; other overlaps are refused");
                }
        } else if (overlap(d->src, sall, d->dst[0], dall) || overlap(d->src, sall, d->dst[1], dall) || overlap(d->dst[0], dall, d->dst[1], dall) ||
                   (mode == UG_DEINT_WEAVE && (overlap(d->prev, sall, d->dst[0], dall) || overlap(d->prev, sall, d->dst[1], dall)))) {
                return bad("ug_hip_deinterlace: sources and destinations must not overlap");
        }
        Params p;
        p.src = (const uint8_t *) d->src;
        p.prev = (const uint8_t *) d->prev;
        p.dst0 = (uint8_t *) d->dst[0];
        p.dst1 = two ? (uint8_t *) d->dst[1] : nullptr;
        p.spitch = (long) sp;
        p.dpitch = (long) dp;
        p.sstride = sstride;
        p.dstride = dstride;
        p.linesize = (int) L;
        p.lines = d->lines;
        p.blend = d->blend_after_weave != 0;
        p.wbytes = (int) written_bytes(cls, mode == UG_DEINT_LINEAR, (long) L);
        const int cb = cls == CR12L ? 48 : 16;
        const long chunks = (L + cb - 1) / cb;
        // lines per lane: kBand where that leaves enough lanes to hide the latency of a lane's line-after-line walk; shorter bands for a single
        // small picture (neighbouring bands run side by side in a workgroup: the lines they share come from L2)
        int band = kBand;
        while (band > kMinBand && chunks * d->frames * ((d->lines + band - 1) / band) < kWantLanes) band /= 2;
        p.band = in_place ? (d->lines + 1) / 2 * 2 : band;
        const uintptr_t all = ptrs | (uintptr_t) sp | (uintptr_t) dp | (uintptr_t) sstride | (uintptr_t) dstride;
        p.amode = all % 16 == 0 ? 16 : all % 4 == 0 ? 4 : 1;
        const long bands = (d->lines + p.band - 1) / p.band;
        const dim3 grid((unsigned) ((chunks + kChunksX - 1) / kChunksX), (unsigned) ((bands + kBandsY - 1) / kBandsY), (unsigned) d->frames);
        hipStream_t st = (hipStream_t) stream;
        switch (cls) {
        case C8: launch<C8>(mode, grid, st, p); break;
        case C16: launch<C16>(mode, grid, st, p); break;
        case CV210: launch<CV210>(mode, grid, st, p); break;
        case CR10K: launch<CR10K>(mode, grid, st, p); break;
        default: launch<CR12L>(mode, grid, st, p); break;
        }
        UG_HIP_LAUNCH_CHECK();
        return UG_HIP_SUCCESS;
}
