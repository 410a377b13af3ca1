// dxt_encode.hip -- fused pixel-format unpack + colour conversion + DXT1 / DXT5-YCoCg 4x4
// block encode for gfx950 (CDNA4).
//
// Replaces, in one pass and with no intermediate buffer:
//   - the CPU decoder_t line loop of the compress modules (cuda_dxt.cpp:206-220,
//     dxt_glsl.cpp:277-289): v210 -> UYVY (pixfmt_conv.c:86-130) is folded into the load;
//   - cuda_yuv422_to_yuv444 / yuv422_to_yuv444.glsl (chroma replication, a full-frame pass
//     in the reference: cuda_dxt.cu:697-732, dxt_encoder.c:482-542);
//   - the block encoders dxt_kernel<...> (cuda_dxt.cu:622-695) / fp_compress_dxt5ycocg
//     (compress_dxt5ycocg_fp.glsl:326-377) / fp_compress_dxt1 (compress_dxt1_fp.glsl:177-229).
//
// Numerics contract: bit-identical to oracle/dxt_oracle.c, the strict-fp32 restatement of
// the shaders.  Every source-level operation is one IEEE binary32 operation; this file is
// compiled with -ffp-contract=off.  Where an operation is fused or strength-reduced below,
// the comment states why the result is bit-identical (exact products by powers of two).
//
// Mapping: one lane encodes one 4x4 block (v210: three consecutive blocks = one 32-byte
// group pair per row).  Consecutive lanes take consecutive blocks of a block-row, so a
// wave's row loads are contiguous (64 x 8 B UYVY, 64 x 12 B RGB, 64 x 32 B v210) and its
// 64 x 16 B (DXT5) / 64 x 8 B (DXT1) stores form one contiguous 1 KiB / 512 B burst.
// The work is VALU-bound: no LDS staging is needed because each input
// byte is read by exactly one lane.  LDS only holds each lane's own lookup columns of the fast
// index stages (IndexTables below): the threshold / palette pair a pixel's one open comparison needs.
//
// Frame sizes that are not multiples of 4 (dxt_util.h:59-67, dxt_encoder.c:362-364,380-394; what -c RTDXT accepts): the stream holds
// (w+3)/4 x (h+3)/4 blocks and pixels past the picture repeat its last column / last line (oracle/dxt_oracle.c, encode_rows, says how
// that is pinned to the executed shaders and where the reference itself slips).  Such frames run the EDGE instantiation of the same
// kernel: line numbers are clamped on the scalar unit, the one lane per block row that holds the cut block fills its registers
// through Loader::load_edge (nothing past the last byte of a line is read), and lines may start at any alignment the packed width
// gives them.  Frames whose sizes ARE multiples of 4 never see any of it: their instantiation is the code it was before.
#include "ug_common.h"

namespace {

constexpr float kInv255  = 0.00392156862745f;           // cuda_dxt.cu:666
constexpr float kOffset  = (float) (128.0 / 255.0);     // compress_dxt5ycocg_fp.glsl:25
constexpr float kInsetC  = (float) ((8.0 / 255.0) / 16.0);
constexpr float kInsetY  = (float) ((16.0 / 255.0) / 32.0);

__device__ __forceinline__ float clamp01(float v) { return fminf(1.0f, fmaxf(0.0f, v)); }

// GLSL round() leaves the direction of exact .5 ties to the implementation, and so does the order in which dot(vec3) is summed.
// Both choices are a RUN-TIME option of the library (UG_DXT_TIES_*, include/ug_mi355x.h), compiled as a template parameter:
//   TIES_EVEN (default): round() ties to even, dot(vec3) summed from the last component -- what the reference's shaders compute when
//                        they are EXECUTED (Mesa llvmpipe, oracle/glsl_ref.c; tests/golden/dxt_glsl_ref.npz pins every block);
//   TIES_AWAY          : roundf() half away from zero, dot() left to right -- the reference's CUDA text (cuda_dxt.cu:106-108,122-124).
// (uint32_t) rintf(x) is v_rndne_f32 + v_cvt_u32_f32.  (uint32_t) roundf(x) for 0 <= x < 2^22: for x >= 0.5 the fp32 sum x + 0.5f
// truncates to the right integer: it is exact unless it lands in a higher binade than x, which only happens for
// x in [2^k - 0.5, 2^k), where both roundf(x) and the (rounded) sum's integer part are 2^k.  Below 0.5 the sum can
// round up to 1.0 (x = 0.5 - 2^-25), so that range is selected to 0 explicitly.  4 instructions instead of roundf's 7.
template <bool AWAY>
__device__ __forceinline__ uint32_t round_u32(float x)
{
        if (!AWAY) {
                return (uint32_t) rintf(x);
        }
        const uint32_t r = (uint32_t) (x + 0.5f);
        return x < 0.5f ? 0u : r;
}

// x / 14.0f without the IEEE division sequence (v_div_scale x2, v_rcp, v_div_fmas, v_div_fixup + 4 fma: five of them on the slow
// pipe, the reciprocal at quarter rate): q = RN(x * RN(1/14)), exact residual, one correction.  Bit-identical to the division for
// x = 0 and EVERY fp32 x in [2^-100, 1], checked exhaustively on the device (ug_hip_selftest_dxt_encode); below 2^-125 the
// quotient is denormal and the residual no longer exact, so callers route (0, 2^-100) to the real division.
constexpr uint32_t kDiv14Exact = 0x0d800000u; // bits of 2^-100
__device__ __forceinline__ float div14(float x)
{
        constexpr float rc = 1.0f / 14.0f;
        const float q = x * rc;
        const float r = __builtin_fmaf(-q, 14.0f, x);
        return __builtin_fmaf(r, rc, q);
}

// GLSL mix(a,b,q) = a*(1-q) + b*q, w = 1-q precomputed in fp32 (cuda_dxt.cu:126-128)
__device__ __forceinline__ float lerp_w(float a, float b, float w, float q)
{
        float p0 = a * w;
        float p1 = b * q;
        return p0 + p1;
}

__device__ __forceinline__ uint32_t palette_index(float d0, float d1, float d2, float d3)
{
        // compress_dxt5ycocg_fp.glsl:237-244
        uint32_t b0 = d0 > d3, b1 = d1 > d2, b2 = d0 > d2, b3 = d1 > d3, b4 = d2 > d3;
        return (b0 & b4) | (((b1 & b2) | (b0 & b3)) << 1);
}


typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32_any __attribute__((aligned(1))); // a dword wherever it lies (lines of 3 * width bytes, EDGE instantiations only)

#ifdef UG_FORCE_ALPHA_LINEAR // test build: the DXT5-YCoCg alpha indices always take the reference-form path (tests/test_gpu_dxt.py)
constexpr bool kForceAlphaLinear = true;
#else
constexpr bool kForceAlphaLinear = false;
#endif

// acc = 2*acc + bit in ONE VALU instruction: the boolean lives in an SGPR lane mask (it is the
// result of v_cmp / SALU mask logic) and is consumed as the carry-in of v_addc_co_u32.
typedef unsigned long long lanemask_t;
// lane mask of a comparison: the SGPR pair v_cmp writes; mask logic on these runs on the scalar unit
#define LANEMASK(cmp) __builtin_amdgcn_ballot_w64(cmp)
__device__ __forceinline__ uint32_t shift_in(uint32_t acc, lanemask_t mask)
{
        lanemask_t carry_out;
        uint32_t r;
        asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(carry_out) : "v"(acc), "s"(mask));
        return r;
}
// the full forms of both encoders: the two index bits of one pixel (glsl:237-244, as palette_index) shifted into w on the lane masks
__device__ __forceinline__ uint32_t shift_in_palette_index(uint32_t w, float d0, float d1, float d2, float d3)
{
        const lanemask_t b0 = LANEMASK(d0 > d3), b1 = LANEMASK(d1 > d2), b2 = LANEMASK(d0 > d2),
                         b3 = LANEMASK(d1 > d3), b4 = LANEMASK(d2 > d3);
        w = shift_in(w, (b1 & b2) | (b0 & b3)); // bit 2i+1
        return shift_in(w, b0 & b4);            // bit 2i
}

// acc + carry (v_addc with a zero addend): adds the boolean of a lane mask to a count
__device__ __forceinline__ uint32_t add_mask(uint32_t acc, lanemask_t mask)
{
        lanemask_t carry_out;
        uint32_t r;
        asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(carry_out) : "v"(acc), "s"(mask));
        return r;
}
// v_cvt_u32_f32 as the hardware defines it (truncation, negative -> 0, no poison for out-of-range input as with a C cast)
__device__ __forceinline__ uint32_t cvt_u32_sat(float x)
{
        uint32_t r;
        asm("v_cvt_u32_f32_e32 %0, %1" : "=v"(r) : "v"(x));
        return r;
}
// bit i of x -> bit 2i (x < 2^16)
__device__ __forceinline__ uint32_t spread16(uint32_t x)
{
        x = (x | (x << 8)) & 0x00ff00ffu;
        x = (x | (x << 4)) & 0x0f0f0f0fu;
        x = (x | (x << 2)) & 0x33333333u;
        x = (x | (x << 1)) & 0x55555555u;
        return x;
}

// Per-wave LDS tables of the fast index stages: every lane owns one column, nothing is shared
// between lanes, so no barrier is involved.  Row-major by entry: a wave's access to one row is 64 consecutive words / 16-byte units.
// pixels per group of the fast stages' software pipelines (table reads of group n + 1 in flight while group n is evaluated).
// Measured, interleaved A/B on UYVY->DXT5 4K: colour groups of 2 / 4 and luma groups of 4 / 8 are equal within 0.3 %; 8 / 16 spill.
constexpr int kDxt1FastGroup = 2, kDxt5FastGroup = 4, kDxt5AlphaGroup = 8;
// DXT5-YCoCg fast stages: the row of the lookup table is read from the mantissa of fma(u, rows - 1, 2^23) instead of
// v_cvt_u32_f32(u * rows).  kIndexBias + n, n = 0 .. 7, is the integer 2^23 + n: one ulp = 1 in that binade.
constexpr float kIndexBias = 8388608.0f;      // 2^23
constexpr uint32_t kIndexBits = 0x4b000000u;  // its bits: lowest set bit 24, so kIndexBits << 8 == 0 (mod 2^32) -- a row offset needs no correction
// what `fields` accumulations acc = (acc << shift) + (kIndexBits + n) leave in a 32-bit word besides the n (wrap-around arithmetic)
constexpr uint32_t index_bias_sum(int fields, int shift)
{
        uint32_t s = 0;
        for (int n = 0; n < fields && n * shift < 32; n++) s += kIndexBits << (n * shift);
        return s;
}
// DXT5-YCoCg colour stage, chroma pairs: the certificate of the index taken from the projection (derived at the stage),
//   eps = (kProjEpsSeg sqrt(vv) + kProjEpsDiag sqrt(dmax) + kProjEpsDmax dmax) / vv,   in thirds of the palette segment
constexpr float kProjEpsSeg = 8.5e-6f, kProjEpsDiag = 7.2e-6f, kProjEpsDmax = 4.3e-6f;
// Diagnostics: waves that left a certified or fast stage for a reference-form side, counted in those sides only.  None of the sides is
// rare on all content -- the per-pixel distances take a few percent of the waves of ordinary video, the exact covariance half the
// waves of flat-chroma content -- and atomics on ONE address are served one after the other: 129 600 counting waves per launch cost
// 1.4 ms beside 0.14 ms of encoding, 62 000 of them 0.6 ms.  So every count is kept in kPairSlots slots, each in a 128-byte line of its
// own, chosen by workgroup and wave; the ug_hip_dxt_encode_stats* functions add them up.
constexpr int kPairSlots = 256, kPairSlotStride = 16; // 16 x 8 B = one line
constexpr int kCounterWords = kPairSlots * kPairSlotStride;
// BY_WAVE = false chooses the slot by workgroup alone: for the count that every kernel of this file holds, so that none of them keeps
// threadIdx.y alive for a cold side (the chroma-pair kernels keep it anyway)
template <bool BY_WAVE = true>
__device__ __forceinline__ void count_slotted(unsigned long long *lines, unsigned long long n)
{
        if ((int) threadIdx.x == __builtin_amdgcn_readfirstlane((int) threadIdx.x)) {
                // block = 64 lanes x up to 4 waves; the wave's number is uniform, and said to be: the slot and its address stay scalar
                const uint32_t wave = BY_WAVE ? (uint32_t) __builtin_amdgcn_readfirstlane((int) threadIdx.y) : 0u;
                const uint32_t slot = ((blockIdx.x + 17u * blockIdx.y + 101u * blockIdx.z) * 4u + wave) & (kPairSlots - 1);
                atomicAdd(&lines[slot * kPairSlotStride], n);
        }
}
// ug_hip_dxt_encode_stats: waves that left a fast index stage for the reference's full form
__device__ unsigned long long g_full_form_waves[2][kCounterWords]; // [0] colour indices, [1] alpha indices
__device__ __forceinline__ void count_full_form(int which) { count_slotted<false>(g_full_form_waves[which], 1ull); }
// the same for the diagonal stage (ug_hip_dxt_encode_stats_ex): waves that formed the reference's covariance sum.  A counter of its own:
// the two above keep meaning what they meant.
__device__ unsigned long long g_exact_cov_waves[kCounterWords];
__device__ __forceinline__ void count_exact_cov() { count_slotted(g_exact_cov_waves, 1ull); }
// and for the colour stage's index from the projection: waves that went on to the per-pixel distances
__device__ unsigned long long g_exact_pair_waves[kCounterWords];
__device__ __forceinline__ void count_exact_pair() { count_slotted(g_exact_pair_waves, 1ull); }
// of those waves, the pair slots (0 .. 7) in which a lane held an uncertified pair and whose two pixels got the distances: one
// addition per wave of what its slot branches counted (ug_hip_dxt_encode_stats_pair_slots)
__device__ unsigned long long g_pair_slot_evaluations[kCounterWords];
__device__ __forceinline__ void count_pair_slots(uint32_t n) { count_slotted(g_pair_slot_evaluations, n); }
// and for the alpha stage's count from the location (chroma-pair loaders): waves that went on to the thresholds and the reference's
// comparison.  A few percent of the waves of ordinary video, every wave of content with few luma levels
// (ug_hip_dxt_encode_stats_alpha adds them up).
__device__ unsigned long long g_exact_alpha_waves[kCounterWords];
__device__ __forceinline__ void count_exact_alpha() { count_slotted(g_exact_alpha_waves, 1ull); }
// DXT5-YCoCg alpha stage, chroma pairs: the certificate of the count taken from the location (derived at the stage),
//   eps = kAlphaEpsFixed + kAlphaEpsRange / range,   in steps of range / 7
constexpr float kAlphaEpsFixed = 2.2e-6f, kAlphaEpsRange = 5.7e-6f;
struct IndexTables {
        float *alpha;   // [8][64] floats: thresholds in DESCENDING order, row 7 = -inf
        float4 *colour;   // DXT5-YCoCg: [3][64] (A.x, A.y, B.x, B.y) of the palette pair whose bisector crosses zone k; DXT1: [6][64], rows 2k / 2k + 1 = A / B (xyz)
};

// ---------------------------------------------------------------------------------------
// colour front ends: bytes -> normalised (c0,c1,c2) per pixel
// ---------------------------------------------------------------------------------------
struct Px16 {
        float a[16], b[16], c[16];
};

// ConvertYUVToRGB (compress_dxt5ycocg_fp.glsl:12-23) for a pixel pair sharing chroma.
__device__ __forceinline__ void yuv_pair_to_rgb(float y0, float y1, float u, float v, Px16 &p, int i)
{
        const float U = u - 0.5f, V = v - 0.5f;
        const float rv = 1.7926f * V, gu = 0.2132f * U, gv = 0.5328f * V, bu = 2.1124f * U;
        const float Y0 = 1.1643f * (y0 - 0.0625f), Y1 = 1.1643f * (y1 - 0.0625f);
        p.a[i] = Y0 + rv;
        p.b[i] = (Y0 - gu) - gv;
        p.c[i] = Y0 + bu;
        p.a[i + 1] = Y1 + rv;
        p.b[i + 1] = (Y1 - gu) - gv;
        p.c[i + 1] = Y1 + bu;
}

__device__ __forceinline__ float byte_f(uint32_t w, int k) { return (float) ((w >> (8 * k)) & 0xffu) * kInv255; }

// 4 pixels of one row from three RGB words (12 B)
__device__ __forceinline__ void row_rgb(const uint32_t *w, Px16 &p, int i)
{
        p.a[i + 0] = byte_f(w[0], 0); p.b[i + 0] = byte_f(w[0], 1); p.c[i + 0] = byte_f(w[0], 2);
        p.a[i + 1] = byte_f(w[0], 3); p.b[i + 1] = byte_f(w[1], 0); p.c[i + 1] = byte_f(w[1], 1);
        p.a[i + 2] = byte_f(w[1], 2); p.b[i + 2] = byte_f(w[1], 3); p.c[i + 2] = byte_f(w[2], 0);
        p.a[i + 3] = byte_f(w[2], 1); p.b[i + 3] = byte_f(w[2], 2); p.c[i + 3] = byte_f(w[2], 3);
}

template <int IN>
struct Loader;

// ---- RGB / YUV444: 12 B per block row ----
template <bool YUV>
struct Loader3 {
        static constexpr int kBlocks = 1;
        static constexpr bool kChromaPairs = false; // every pixel has its own chroma
        uint32_t w[4][3];
        template <bool EDGE = false>
        __device__ __forceinline__ void load(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4])
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        if (EDGE) { // 3 * width bytes per line: a line starts wherever it starts
                                const u32_any *p = (const u32_any *) (src + ((uint32_t) rows[r] * pitch + unit_x * 12u));
                                w[r][0] = p[0]; w[r][1] = p[1]; w[r][2] = p[2];
                        } else {
                                const uint32_t *p = (const uint32_t *) (src + ((uint32_t) rows[r] * pitch + unit_x * 12u));
                                w[r][0] = p[0]; w[r][1] = p[1]; w[r][2] = p[2];
                        }
                }
        }
        // The block at the right edge of a picture whose width is not a multiple of 4: `valid` (1..3) of its pixel columns exist, the
        // others repeat the last one (GL_CLAMP_TO_EDGE, dxt_encoder.c:362-364).  Nothing past the last byte of a line is read.
        __device__ __forceinline__ void load_edge(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4], int valid)
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const uint8_t *p = src + ((uint32_t) rows[r] * pitch + unit_x * 12u);
                        uint32_t b[12];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                                const int jj = 3 * min(j, valid - 1);
                                b[3 * j] = p[jj]; b[3 * j + 1] = p[jj + 1]; b[3 * j + 2] = p[jj + 2];
                        }
#pragma unroll
                        for (int k = 0; k < 3; k++) w[r][k] = b[4 * k] | b[4 * k + 1] << 8 | b[4 * k + 2] << 16 | b[4 * k + 3] << 24;
                }
        }
        __device__ __forceinline__ void block(int, Px16 &p) const
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        row_rgb(w[r], p, 4 * r);
                }
                if (YUV) { // cuda_dxt.cu:686-691 (per pixel, no chroma sharing in 4:4:4)
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                                const float U = p.b[i] - 0.5f, V = p.c[i] - 0.5f;
                                const float Y = 1.1643f * (p.a[i] - 0.0625f);
                                p.a[i] = Y + 1.7926f * V;
                                p.b[i] = (Y - 0.2132f * U) - 0.5328f * V;
                                p.c[i] = Y + 2.1124f * U;
                        }
                }
        }
};

// ---- RGBA: 16 B per block row, alpha ignored (compress_dxt1_fp.glsl:41 reads .rgb) ----
struct LoaderRGBAWords {
        static constexpr int kBlocks = 1;
        static constexpr bool kChromaPairs = false; // every pixel has its own chroma
        uint4 w[4];
        template <bool EDGE = false>
        __device__ __forceinline__ void load(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4])
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        if (EDGE) { // 4 * width bytes per line: 4-byte alignment is all a line has
                                const uint32_t *q = (const uint32_t *) (src + ((uint32_t) rows[r] * pitch + unit_x * 16u));
                                w[r] = make_uint4(q[0], q[1], q[2], q[3]);
                        } else {
                                w[r] = *(const uint4 *) (src + ((uint32_t) rows[r] * pitch + unit_x * 16u));
                        }
                }
        }
        __device__ __forceinline__ void load_edge(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4], int valid)
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const uint32_t *q = (const uint32_t *) (src + ((uint32_t) rows[r] * pitch + unit_x * 16u));
                        w[r] = make_uint4(q[0], q[min(1, valid - 1)], q[min(2, valid - 1)], q[min(3, valid - 1)]);
                }
        }
        __device__ __forceinline__ void block(int, Px16 &p) const
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const uint32_t q[4] = { w[r].x, w[r].y, w[r].z, w[r].w };
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                                p.a[4 * r + c] = byte_f(q[c], 0);
                                p.b[4 * r + c] = byte_f(q[c], 1);
                                p.c[4 * r + c] = byte_f(q[c], 2);
                        }
                }
        }
};

// ---- UYVY: 8 B per block row; chroma replicated (yuv422_to_yuv444.glsl:22-30) ----
// The texture-address unit does the byte -> float conversion: typed buffer loads with format 8_8_8_8 USCALED return
// float(byte) for the four bytes of a word (exact), so the 32 v_cvt_f32_ubyte of a block -- slow-pipe VALU work -- disappear; the
// multiplication by kInv255 stays in the shader arithmetic.  Costs 24 more VGPRs (the raw block is held as 32 floats).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
template <bool CONVERT>
struct LoaderUYVYTyped {
        static constexpr int kBlocks = 1;
        static constexpr bool kChromaPairs = CONVERT; // pixels 2j, 2j + 1 of a row come out of one yuv_pair_to_rgb call (raw Y,Cb,Cr in the RGB channels: the pair shares g and b only, not Co / Cg)
        f32x4 f[4][2];
        // width = 2 (mod 4): one U Y0 V Y1 group exists; the second one repeats its last pixel: U Y1 V Y1.  (float) byte is what the
        // USCALED typed load returns.
        __device__ __forceinline__ void load_edge(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4], int)
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const uint32_t q = *(const uint32_t *) (src + ((uint32_t) rows[r] * pitch + unit_x * 8u));
                        const float u = (float) (q & 0xffu), y0 = (float) ((q >> 8) & 0xffu), v = (float) ((q >> 16) & 0xffu), y1 = (float) (q >> 24);
                        f[r][0] = f32x4{ u, y0, v, y1 };
                        f[r][1] = f32x4{ u, y1, v, y1 };
                }
        }
        template <bool EDGE = false> // (the typed loads take 4-byte elements: a line that is only 4-byte aligned is no different)
        __device__ __forceinline__ void load(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4])
        {
                const uint64_t base = (uint64_t) src;
                // V#: base, stride 0, num_records = max, dst_sel xyzw = R G B A, data format 8_8_8_8, type buffer
                const i32x4 desc = { (int) (uint32_t) base, (int) ((uint32_t) (base >> 32) & 0xffffu), -1, 0x52FAC };
                uint32_t off[4];
#pragma unroll
                for (int r = 0; r < 4; r++) off[r] = (uint32_t) rows[r] * pitch + unit_x * 8u;
                asm volatile("tbuffer_load_format_xyzw %0, %8, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen\n"
                             "tbuffer_load_format_xyzw %1, %8, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen offset:4\n"
                             "tbuffer_load_format_xyzw %2, %9, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen\n"
                             "tbuffer_load_format_xyzw %3, %9, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen offset:4\n"
                             "tbuffer_load_format_xyzw %4, %10, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen\n"
                             "tbuffer_load_format_xyzw %5, %10, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen offset:4\n"
                             "tbuffer_load_format_xyzw %6, %11, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen\n"
                             "tbuffer_load_format_xyzw %7, %11, %12, 0 format:[BUF_DATA_FORMAT_8_8_8_8,BUF_NUM_FORMAT_USCALED] offen offset:4\n"
                             "s_waitcnt vmcnt(0)"
                             : "=&v"(f[0][0]), "=&v"(f[0][1]), "=&v"(f[1][0]), "=&v"(f[1][1]), "=&v"(f[2][0]), "=&v"(f[2][1]), "=&v"(f[3][0]), "=&v"(f[3][1])
                             : "v"(off[0]), "v"(off[1]), "v"(off[2]), "v"(off[3]), "s"(desc)
                             : "memory");
        }
        __device__ __forceinline__ void block(int, Px16 &p) const
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
#pragma unroll
                        for (int k = 0; k < 2; k++) {
                                const float u = f[r][k].x * kInv255, y0 = f[r][k].y * kInv255;
                                const float v = f[r][k].z * kInv255, y1 = f[r][k].w * kInv255;
                                const int i = 4 * r + 2 * k;
                                if (CONVERT) {
                                        yuv_pair_to_rgb(y0, y1, u, v, p, i);
                                } else { // DXT1_YUV: YCbCr stored in the RGB channels (dxt_encoder.c:318-323)
                                        p.a[i] = y0; p.b[i] = u; p.c[i] = v;
                                        p.a[i + 1] = y1; p.b[i + 1] = u; p.c[i + 1] = v;
                                }
                        }
                }
        }
};
template <> struct Loader<UG_PF_UYVY> : LoaderUYVYTyped<true> {};
template <> struct Loader<UG_PF_UYVY_RAW> : LoaderUYVYTyped<false> {};
// RGB / YUV444 / RGBA keep word loads: measured with typed loads RGBA is equal and RGB (three 4-byte typed loads per 12-byte row) twice
// as slow -- the address unit, not the VALU, becomes the limit.
template <> struct Loader<UG_PF_RGB> : Loader3<false> {};
template <> struct Loader<UG_PF_YUV444> : Loader3<true> {};
template <> struct Loader<UG_PF_RGBA> : LoaderRGBAWords {};

// ---- v210: 12 px = 3 blocks = 32 B per row.  The 10-bit samples come in UYVY order, three
// per little-endian word; the reference converts to 8-bit UYVY by >>2 first
// (vc_copylinev210, pixfmt_conv.c:86-130, selected by cuda_dxt.cpp:162) ----
template <>
struct Loader<UG_PF_V210> {
        static constexpr int kBlocks = 3;
        static constexpr bool kChromaPairs = true; // pixels 2j, 2j + 1 of a row come out of one yuv_pair_to_rgb call
        uint32_t w[4][8];
        template <bool EDGE = false> // (a v210 line is padded to 128 bytes whatever the width, video_codec.c:507-521: whole units are always there)
        __device__ __forceinline__ void load(const uint8_t *src, uint32_t pitch, uint32_t unit_x, const int (&rows)[4])
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const uint4 *p = (const uint4 *) (src + ((uint32_t) rows[r] * pitch + unit_x * 32u));
                        const uint4 q0 = p[0], q1 = p[1];
                        w[r][0] = q0.x; w[r][1] = q0.y; w[r][2] = q0.z; w[r][3] = q0.w;
                        w[r][4] = q1.x; w[r][5] = q1.y; w[r][6] = q1.z; w[r][7] = q1.w;
                }
        }
        // sample s (0..23) of the row, top 8 bits of the 10-bit field
        __device__ __forceinline__ float samp(int r, int s) const
        {
                return (float) ((w[r][s / 3] >> (10 * (s % 3) + 2)) & 0xffu) * kInv255;
        }
        __device__ __forceinline__ void block(int k, Px16 &p) const
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
#pragma unroll
                        for (int pr = 0; pr < 2; pr++) {
                                const int s = 8 * k + 4 * pr; // U Y0 V Y1
                                yuv_pair_to_rgb(samp(r, s + 1), samp(r, s + 3), samp(r, s), samp(r, s + 2), p, 4 * r + 2 * pr);
                        }
                }
        }
        // the same for a block that may be the cut one of a width = 2 (mod 4): `half` = only its first pixel pair exists, the
        // second repeats the pair's last pixel (Y1 with the pair's chroma)
        __device__ __forceinline__ void block_edge(int k, Px16 &p, bool half) const
        {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const int s = 8 * k;
                        const float u0 = samp(r, s), y00 = samp(r, s + 1), v0 = samp(r, s + 2), y01 = samp(r, s + 3);
                        yuv_pair_to_rgb(y00, y01, u0, v0, p, 4 * r);
                        const float u1 = half ? u0 : samp(r, s + 4), y10 = half ? y01 : samp(r, s + 5), v1 = half ? v0 : samp(r, s + 6), y11 = half ? y01 : samp(r, s + 7);
                        yuv_pair_to_rgb(y10, y11, u1, v1, p, 4 * r + 2);
                }
        }
};

// ---------------------------------------------------------------------------------------
// DXT5-YCoCg block encode (compress_dxt5ycocg_fp.glsl:326-377 / cuda_dxt.cu:471-509)
// ---------------------------------------------------------------------------------------
// The stages that stand alone are functions named after the shader's routines; the others follow in encode_dxt5ycocg, in the shader's order.
// PAIRS (select_ycocg_diagonal, encode_dxt5ycocg): pixels 2j, 2j + 1 of a row share their chroma sample (Loader::kChromaPairs).
//
// Exact products by powers of two, for every stage below:
// ConvertRGBToYCoCg (glsl:27-34).  2.0*x and *0.25 are exact (powers of two), so
//   (r + 2g + b)*0.25      : fma(g,2,r) == r + 2g bit-for-bit (2g exact)
//   (2r - 2b)*0.25 + off   : 2r-2b == 2(r-b) exactly, *0.25 exact -> (r-b)*0.5 + off,
//                            and fma(r-b, 0.5, off) == ((r-b)*0.5) + off (product exact)
//   (-r + 2g - b)*0.25+off : fma(g,2,-r) == -r + 2g ; fma(t,0.25,off) == t*0.25 + off
//
// The same rule through the rest of encode_dxt5ycocg.  x * 2^k is exact unless it underflows, so
// RN(x * 2^k + c) == fma(x, 2^k, c) and RN(2^k x) == 2^k RN(x): wherever the reference multiplies by 2, 4, 8, 16, 1/2, 1/4, 1/16 or
// 1/32 and adds, the product moves into the fma of the sum, and the luma is never scaled at all: Y4 = r + 2 g + b = 4 Y is kept, and
// what it feeds is homogeneous of degree 1 (fmin / fmax commute with the scale, +, - and * by a constant scale with it), so the
// alpha stage compares Y4 <= 4 T where the reference compares Y <= T.  Sites, with the smallest non-zero magnitude the scaled
// operand takes (tests/test_dxt_pow2_fold_bound.py enumerates the first, and restates every site in strict fp32):
//   Y4 = t + b       the deleted * 0.25.  RGB front ends: r, g, b are bytes / 255, a non-zero r + 2 g + b is >= 1 / 255.  YUV front
//                    ends: r, g, b are sums of 1.1643 (y - 1/16) and products of (u | v) - 1/2 by constants of 0.2 .. 2.1, y, u, v
//                    bytes / 255.  y - 1/16 and u - 1/2 are 0 or multiples of the byte's last place, >= 2^-31 (a byte / 255 is
//                    >= 2^-8), and at least 2^-12 (|16 / 255 - 1/16|, |127.5 - 127| / 255) in magnitude, so every term is 0 or >= 2^-15
//                    with its last place >= 2^-39, and so is the last place of any sum of them: a non-zero t + b is >= 2^-39.
//                    The enumeration of every (y, u, v) finds 3 * 2^-28 at the least.
//   box ends         mnY + inset = fma(mn4, 1/4, inset) and inset = fma(mx4 - mn4, 1/128, -kInsetY): mx4 - mn4 = 4 (mxY - mnY)
//                    exactly, and / 128 of it is the reference's / 32.  The two ends leave the 4 x domain here, BEFORE the clamp
//                    and the * 255 rounding, through the fma they needed anyway (clamp modifier as before: no v_med3 to [0, 4],
//                    no 63.75, no instruction more than the reference's own inset: chosen over clamping in the 4 x domain, which
//                    costs two v_med3, at equal registers).  The thresholds go back up through their CONSTANTS: see there.
//   chroma ends      fma(mx - off, fs, off), fs = 1, 2, 4; insets fma(a - b, 1/16, -kInsetC); dequantised ends
//                    fma(x / 255 - off, rfs, off), rfs = 1, 1/2, 1/4.  Co, Cg and the end points are floats in (-2, 3) built from the
//                    terms above and off = 128 / 255, so multiples of 2^-39 again; mx - off, a - b and x / 255 - off are differences
//                    of two of them, or of one and a constant of that kind: equal, or >= 2^-39 apart (>= 2^-25 where both are near 1/2).
//   thresholds       (8 - k) mx + (k - 1) mn with one multiplier a power of two: that product inside the fma.
// No operand comes anywhere near 2^-124, below which a product by 1/32 would be denormal.  Overflow is out of the question
// (|values| < 16).  The reference writes one operation per product: (t + b) * 0.25 here, and so on at every site.

//
// The difference domain (PAIRS).  The reference reaches Co and Cg through d = r - b and e = fma(g, 2, -r) - b:
//   Co = f(d) = RN(d / 2 + off),   Cg = f'(e) = RN(e / 4 + off).
// d / 2 and e / 4 are exact, + off is monotone in real arithmetic and RN is monotone non-decreasing, so f and f' are monotone
// non-decreasing maps of fp32 to fp32, and a monotone map commutes with min and max: min_i f(d_i) = f(min_i d_i), the SAME float,
// bit for bit, and so for max and for f'.  No NaN occurs (|d|, |e| < 4), and d = -0 gives off as +0 does.  So for chroma-pair
// loaders the pixels stay (4 Y, d, e): the box is taken over d and e and its FOUR ends go through f / f' -- the reference's own
// mnCo .. mxCg, from all sixteen pixels -- instead of all thirty-two values.  What else read Co[i] / Cg[i] on the main line, the
// diagonal's rough sum and the colour stage's projection, only locates under a certificate and takes d, e as they are (1/2, 1/4 and
// off folded into its constants: derived at each); the reference-form sides (exact covariance, per-pixel distances, full form,
// flat blocks) form Co[i] = f(d[i]), Cg[i] = f'(e[i]) behind their own branch, the reference's operations in the reference's order.
// tests/test_dxt_pair_difference_bound.py checks the ends on every block of its frames and the monotonicity over the d and e of
// every (y, u, v) of bytes.

// ConvertRGBToYCoCg (glsl:27-34, the first lines of the block comment above): (r, g, b) in p.a / p.b / p.c -> (4 Y, Co, Cg) in place;
// PAIRS: -> (4 Y, d, e), the reference's own intermediate values
template <bool PAIRS>
__device__ __forceinline__ void convert_rgb_to_ycocg(Px16 &p)
{
#pragma unroll
        for (int i = 0; i < 16; i++) {
                const float r = p.a[i], g = p.b[i], b = p.c[i];
                const float t = __builtin_fmaf(g, 2.0f, r);
                p.a[i] = t + b; // Y4 = 4 Y
                if constexpr (PAIRS) {
                        p.b[i] = r - b;
                        p.c[i] = __builtin_fmaf(g, 2.0f, -r) - b;
                } else {
                        p.b[i] = __builtin_fmaf(r - b, 0.5f, kOffset);
                        p.c[i] = __builtin_fmaf(__builtin_fmaf(g, 2.0f, -r) - b, 0.25f, kOffset);
                }
        }
}
// Co / Cg of a pixel from what the conversion left in p.b / p.c: f(d), f'(e) for PAIRS, the value itself otherwise.  `off` is kOffset;
// a reference-form side hands in its own copy (side_offset): to the compiler the sides' values then have nothing in common, and it
// cannot make the later sides' "redundant" by computing all thirty-two ahead of the first branch (which it does otherwise).  The
// copy is made by the asm's own instruction, so that it stays on the side, too.
template <bool PAIRS>
__device__ __forceinline__ float side_offset()
{
        float off = kOffset;
        if constexpr (PAIRS) {
                asm volatile("v_mov_b32_e32 %0, %1" : "=v"(off) : "i"(__builtin_bit_cast(uint32_t, kOffset)));
        }
        return off;
}
template <bool PAIRS>
__device__ __forceinline__ float co_of(float x, float off) { return PAIRS ? __builtin_fmaf(x, 0.5f, off) : x; }
template <bool PAIRS>
__device__ __forceinline__ float cg_of(float x, float off) { return PAIRS ? __builtin_fmaf(x, 0.25f, off) : x; }

// FindMinMaxColorsBox (glsl:69-78).  Y[] holds Y4, and so do mnY / mxY
__device__ __forceinline__ void find_min_max_colors_box(const float *Y, const float *Co, const float *Cg, float &mnY, float &mxY, float &mnCo,
                                                        float &mxCo, float &mnCg, float &mxCg)
{
        mnY = Y[0]; mxY = Y[0]; mnCo = Co[0]; mxCo = Co[0]; mnCg = Cg[0]; mxCg = Cg[0];
#pragma unroll
        for (int i = 1; i < 16; i++) {
                mnY = fminf(mnY, Y[i]);    mxY = fmaxf(mxY, Y[i]);
                mnCo = fminf(mnCo, Co[i]); mxCo = fmaxf(mxCo, Co[i]);
                mnCg = fminf(mnCg, Cg[i]); mxCg = fmaxf(mxCg, Cg[i]);
        }
}

// SelectYCoCgDiagonal (glsl:169-183): sequential sum, i = 0..15.  True where the covariance is negative: the caller swaps the Cg ends.
// PAIRS: Co[] / Cg[] hold d / e (the difference domain, at the conversion), mnd .. mxe are their box; mnCo .. mxCg are the reference's ends.
template <bool PAIRS>
__device__ __forceinline__ bool select_ycocg_diagonal(const float *Co, const float *Cg, float mnCo, float mxCo, float mnCg, float mxCg,
                                                      float mnd, float mxd, float mne, float mxe)
{
        if constexpr (!PAIRS) {
                const float midx = (mxCo + mnCo) * 0.5f, midy = (mxCg + mnCg) * 0.5f;
                float cov = 0.0f;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                        const float tx = Co[i] - midx, ty = Cg[i] - midy;
                        cov = cov + tx * ty;
                }
                return cov < 0.0f;
        } else {
                // One product per chroma pair (PAIRS).  The reference uses cov for its SIGN only, so the sign is found
                // from a cheaper sum and the reference's own sum is kept for the blocks where that one cannot tell.
                //   rough = sum over the 8 EVEN pixels of tx ty, accumulated with fma: half of cov, up to the errors below.
                // With hx = mxCo - mnCo, hy = mxCg - mnCg every |tx| <= hx / 2, |ty| <= hy / 2 (+ half an ulp of mid's own rounding, < 6e-8,
                // which the slack at the end covers), so every product and every partial sum is bounded through hx hy / 4 per term.
                //   Odd pixel replaced by its even one: the pixels of a pair differ by |dCo|, |dCg| < 5e-7 (the pair-location comment in the
                //   colour stage; tests/test_dxt_pair_chroma_bound.py), and (tx + dx) (ty + dy) - tx ty = dx (ty + dy) + tx dy with the odd
                //   pixel's own |ty + dy| <= hy / 2: <= 5e-7 (hx + hy) / 2 per pair, <= 2e-6 (hx + hy) over the eight.
                //   The reference's roundings: 16 products of <= hx hy / 4 and 16 partial sums, the k-th <= k hx hy / 4, 2^-24 relative
                //   each: (4 + 34) 2^-24 hx hy < 4e-6 hx hy.
                //   The rough sum's roundings: 8 fma, the k-th partial sum <= k hx hy / 4: 9 * 2^-24 hx hy < 1e-6 hx hy, doubled with the sum.
                // So |2 rough - cov| < 2e-6 (hx + hy) + 6e-6 hx hy, and the sign of rough is the sign of cov wherever
                //   |2 rough| > eps = 1e-5 (hx + hy + hx hy):
                // a factor > 2 over the analysis (tests/test_dxt_pair_cov_bound.py restates the stage in strict fp32 and finds
                // |2 rough - cov| < 0.04 eps over its content).  The 2 is folded into the constant.  These fma only locate; no
                // result of theirs is an operation of the reference.
                // Exactly flat axis, hx hy == 0: with Co flat midx is mxCo itself (2 x * 0.5), every tx is exactly 0, the reference's
                // cov is +-0 and it does not swap; with Cg flat the swap exchanges equal values.  Such blocks are certified without the
                // comparison (for a sum over Co / Cg themselves rough would be +-0 in both; for the sum actually formed see the end of the next paragraph).
                // A wave that holds a block the certificate does not cover (smooth content: one chroma sample under varying luma leaves
                // spreads of rounding size) evaluates the reference's sum for all of its blocks and decides from it.
                //
                // In the difference domain.  The sum is taken over tx' = d - midd, ty' = e - mide with midd = (mxd + mnd) / 2,
                // mide = (mxe + mne) / 2: in real arithmetic tx' = 2 tx and ty' = 4 ty, so the sum is 8 rough and is compared with 8 x the
                // bound.  What is new in |rough' / 4 - cov| (rough' / 4 standing for 2 rough), with u = 2^-24:
                //   tx - tx' / 2 = rho_i - (rho_mx + rho_mn) / 2 - mu_x + mu_d / 2:  Co's own rounding at the pixel and at the two ends
                //   (|Co| < 2: <= u each), the rounding of midx (the reference's; counted here, not left to the slack) and of midd
                //   (|mxd + mnd| < 4: <= 2 u, halved, and halved again into tx's scale), |.| <= 3.5 u = 2.1e-7 =: dx; ty - ty' / 4 the
                //   same with |Cg| < 2, |mxe + mne| < 8 (4 u, halved, quartered): <= 3.5 u = dy.  Per product dx |ty| + |tx| dy + dx dy with
                //   |tx| <= hx / 2, |ty| <= hy / 2; sixteen of them (eight, doubled): 1.7e-6 (hx + hy) + 7e-13.
                //   tx', ty' round as tx, ty do (relative u on each factor): 8 * 2 u * 2 hx hy / 4 = 5e-7 hx hy.
                // With the terms above: |rough' / 4 - cov| < 3.7e-6 (hx + hy) + 6.5e-6 hx hy + 7e-13.  hx <= 1.96 and hy <= 1.36 (the YUV
                // front ends' ranges), so hx hy <= 0.8 (hx + hy) and 2 x that stays under
                //   eps = 1e-5 (hx + hy + hx hy) + 1.5e-12:
                // the present factor still covers the (hx + hy) and hx hy terms; the absolute term is new (the product of two
                // differences of rounding size, which spreads of a few ulp do not bound) and rides in the fma that scales the bound.
                // tests/test_dxt_pair_difference_bound.py restates this form in strict fp32 and holds |rough' / 4 - cov| to eps / 4.
                // Exactly flat Co: mnCo == mxCo no longer implies mnd == mxd -- two d an ulp apart can round to one Co -- so rough' may
                // be non-zero, of either sign, on a block whose every tx is 0 in the reference (cov = +-0: no swap).  The swap is
                // therefore rough' < 0 AND hx != 0 (lane masks, on the scalar unit).  Such blocks exist for UYVY bytes: the test
                // finds them by enumeration (one chroma sample under two lumas; 1.75 million (u, v, y, y') of those it tries have
                // rough' < 0).  Their Cg spread is of rounding size as well, and on the 400 000 looked at the exchanged ends quantise
                // to the same codes: the rule is what makes mnCg / mxCg the reference's floats, which the contract asks for, not
                // something a byte of output has shown so far.  With Cg flat the swap exchanges equal values and nothing is needed.
                const float midd = (mxd + mnd) * 0.5f, mide = (mxe + mne) * 0.5f;
                const float hx = mxCo - mnCo, hy = mxCg - mnCg;
                float rough = 0.0f;
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                        rough = __builtin_fmaf(Co[i] - midd, Cg[i] - mide, rough);
                }
                const lanemask_t certain = LANEMASK(fabsf(rough) > __builtin_fmaf(__builtin_fmaf(hx, hy, hx + hy), 4e-5f, 6e-12f)) | LANEMASK(hx * hy == 0.0f);
                bool swap;
                if (__builtin_expect(certain == LANEMASK(true), 1)) { // __all, on the two comparisons' own lane masks
                        swap = (rough < 0.0f) & (hx != 0.0f);
                } else {
                        // The empty asm keeps this a real branch (see the alpha stage's fallback); the reference's mids are formed behind it,
                        // from ends that pass through it, and so are Co[i] / Cg[i]: nothing of this side is computed ahead of the branch.
                        float x0 = mnCo, x1 = mxCo, y0 = mnCg, y1 = mxCg;
                        asm volatile("; exact covariance" : "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1) :: "memory");
                        const float off = side_offset<PAIRS>();
                        count_exact_cov();
                        const float mx = (x1 + x0) * 0.5f, my = (y1 + y0) * 0.5f;
                        float cov = 0.0f;
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                                const float tx = co_of<PAIRS>(Co[i], off) - mx, ty = cg_of<PAIRS>(Cg[i], off) - my;
                                cov = cov + tx * ty;
                        }
                        swap = cov < 0.0f;
                }
                return swap;
        }
}

// The reference's form of EmitIndicesYCoCgDXT5 (glsl:217-250), for the waves the fast stage in encode_dxt5ycocg does not take.  The four squared
// distances of TWO horizontally adjacent pixels are computed with packed fp32 (v_pk_add/v_pk_mul: IEEE per component, so
// bit-identical to the scalar form).  PAIRS: Co[] / Cg[] hold d / e, and the pixels' Co / Cg are formed here.
template <bool PAIRS>
__device__ __forceinline__ uint32_t emit_indices_ycocg_full_form(const float *Co, const float *Cg, const float (&cx)[4], const float (&cy)[4], float off)
{
        uint32_t w_cidx = 0;
        f32x2 cx2[4], cy2[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
                cx2[k] = (f32x2) { cx[k], cx[k] };
                cy2[k] = (f32x2) { cy[k], cy[k] };
        }
#pragma unroll
        for (int i = 14; i >= 0; i -= 2) { // pixel pairs, last first: bits are shifted in MSB first
                const f32x2 co = { co_of<PAIRS>(Co[i], off), co_of<PAIRS>(Co[i + 1], off) }, cg = { cg_of<PAIRS>(Cg[i], off), cg_of<PAIRS>(Cg[i + 1], off) };
                f32x2 d[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                        const f32x2 tx = co - cx2[k], ty = cg - cy2[k];
                        d[k] = tx * tx + ty * ty;
                }
#pragma unroll
                for (int h = 1; h >= 0; h--) { // pixel i+1, then pixel i
                        w_cidx = shift_in_palette_index(w_cidx, d[0][h], d[1][h], d[2][h], d[3][h]);
                }
        }
        return w_cidx;
}

template <bool AWAY, bool PAIRS>
__device__ __forceinline__ uint4 encode_dxt5ycocg(Px16 &p, const IndexTables &tab)
{
        convert_rgb_to_ycocg<PAIRS>(p);
        const float *Y = p.a, *Co = p.b, *Cg = p.c; // Y[] holds Y4, and so do mnY / mxY up to InsetYBBox.  PAIRS: Co[] / Cg[] hold d / e (co_of, cg_of)

        float mnY, mxY, mnCo, mxCo, mnCg, mxCg;
        find_min_max_colors_box(Y, Co, Cg, mnY, mxY, mnCo, mxCo, mnCg, mxCg);
        // PAIRS: that was the box of d and e; its ends through the monotone maps are the reference's ends, bit for bit (the difference domain, at the conversion)
        const float mnd = mnCo, mxd = mxCo, mne = mnCg, mxe = mxCg;
        mnCo = co_of<PAIRS>(mnd, kOffset); mxCo = co_of<PAIRS>(mxd, kOffset); mnCg = cg_of<PAIRS>(mne, kOffset); mxCg = cg_of<PAIRS>(mxe, kOffset);

        if (select_ycocg_diagonal<PAIRS>(Co, Cg, mnCo, mxCo, mnCg, mxCg, mnd, mxd, mne, mxe)) {
                const float t = mxCg; mxCg = mnCg; mnCg = t;
        }

        // ScaleYCoCg (glsl:150-167)
        uint32_t scale = 1;
        float fs = 1.0f, rfs = 1.0f; // float(scale) and its exact reciprocal
        {
                const float m0 = fmaxf(fabsf(mnCo - kOffset), fabsf(mnCg - kOffset));
                const float m1 = fmaxf(fabsf(mxCo - kOffset), fabsf(mxCg - kOffset));
                const float m = fmaxf(m0, m1);
                if (m < (float) (64.0 / 255.0)) { scale = 2; fs = 2.0f; rfs = 0.5f; }
                if (m < (float) (32.0 / 255.0)) { scale = 4; fs = 4.0f; rfs = 0.25f; }
        }

        // EmitEndPointsYCoCgDXT5 (glsl:185-215) with InsetCoCgBBox (glsl:92-97).  cmx / cmn: the dequantised ends the palette is built from.
        // "/ 16.0" and "/ float(scale)" are multiplications by exact powers of two.
        uint32_t w_end;
        float cmx[2], cmn[2];
        {
                const float q[2] = { 31.0f, 63.0f };
                const float mx_in[2] = { mxCo, mxCg }, mn_in[2] = { mnCo, mnCg };
                uint32_t imax[2], imin[2];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                        float a = __builtin_fmaf(mx_in[k] - kOffset, fs, kOffset);
                        float b = __builtin_fmaf(mn_in[k] - kOffset, fs, kOffset);
                        const float inset = __builtin_fmaf(a - b, 0.0625f, -kInsetC);
                        b = clamp01(b + inset);
                        a = clamp01(a - inset);
                        imax[k] = round_u32<AWAY>(a * q[k]);
                        imin[k] = round_u32<AWAY>(b * q[k]);
                }
                w_end = ((imax[0] << 11) | (imax[1] << 5) | (scale - 1)) |
                        (((imin[0] << 11) | (imin[1] << 5) | (scale - 1)) << 16);
                imax[0] = (imax[0] << 3) | (imax[0] >> 2);
                imax[1] = (imax[1] << 2) | (imax[1] >> 4);
                imin[0] = (imin[0] << 3) | (imin[0] >> 2);
                imin[1] = (imin[1] << 2) | (imin[1] >> 4);
                const float inv255 = (float) (1.0 / 255.0);
#pragma unroll
                for (int k = 0; k < 2; k++) {
                        cmx[k] = __builtin_fmaf((float) imax[k] * inv255 - kOffset, rfs, kOffset);
                        cmn[k] = __builtin_fmaf((float) imin[k] * inv255 - kOffset, rfs, kOffset);
                }
        }

        // InsetYBBox (glsl:86-91): in come the ends of Y4, out go the reference's own ends (the site list ahead of the stage functions)
        const float inset = __builtin_fmaf(mxY - mnY, 0.0078125f, -kInsetY);
        mnY = clamp01(__builtin_fmaf(mnY, 0.25f, inset));
        mxY = clamp01(__builtin_fmaf(mxY, 0.25f, -inset));
        // EmitAlphaEndPointsYCoCgDXT5 (glsl:252-259)
        uint32_t w0 = (round_u32<AWAY>(mnY * 255.0f) << 8) | round_u32<AWAY>(mxY * 255.0f);
        uint32_t w1 = 0;
        // EmitAlphaIndicesYCoCgDXT5 (glsl:262-312): count c = #{k : a <= ab_k}, index = f(c).
        {
                // raw counts, 3 bits per pixel: lo = px 0..9 (30 bits), hi = px 10..15 (18 bits)
                uint32_t lo = 0, hi = 0;
                float range = mxY - mnY;
                bool located = false; // wave-uniform: lo / hi hold the counts already
                // Count from the location alone (chroma-pair loaders).  In the notation of the fast form below: the thresholds are D_m,
                // descending, range / 7 apart, with a <= D_m <=> t >= m - 1/2 for t = 7 - (a - mnY) * 7 / range in real arithmetic on the
                // reference's fp32 ends and range, so the reference's count #{m : a <= D_m} is RN(clamp(t, 0, 7)) wherever t is not next to a
                // half-integer.  The pixels are Y4 (their factor takes the exact 1/4):
                //   u = clamp01(fma(Y4, -inv / 4, fma(mnY, inv, 1))) = t / 7,   inv = rcp(range),
                //   r = fma(u, 7, 2^23) = the integer 2^23 + c, c = RN(7 u) = 0 .. 7 (float bits, collected as the rows below are),
                //   dist = fma(u, 7, 2^23 - r) = 7 u - c  (the difference is exact),
                // and a block is certified where max |dist| < 1/2 - eps over its sixteen pixels: no pixel within eps of a half-integer of t.
                // eps, in steps of range / 7, with R = range (fp32), mnY, mxY in [0, 1] and R > 2^-10 (the wave test in front):
                //   the reference's thresholds   4 D_m as formed below against the real 4 mnY + 4 R (15 - 2 m) / 14 (the 4x domain, one step =
                //                  4 R / 7, so an absolute error E there is 1.75 E / R steps): the product (8 - k) 4 mxY or (k - 1) 4 mnY <= 24 and
                //                  the sum <= 28 round by <= 2^-20 each, and * 1/7 leaves (2^-19) / 7 = 2.7e-7;  RN(1/7) is off by 4.5e-8
                //                  relative, on a quotient <= 4: 1.8e-7;  the quotient's and the final fma's rounding at magnitude <= 4: 2^-23
                //                  = 1.2e-7 each;  mid = RN(R / 14) <= 1/14 by 2^-28, times 4: 1.5e-8;  the sum carries mxY - mnY where mid carries
                //                  R = RN(mxY - mnY): (6/7) 4 * 2^-25 = 1.0e-7.  E <= 8.1e-7: 1.41e-6 / R.  (D_7 = fma(mid, 4, 4 mnY) rounds once.)
                //   inv            rcp at 1 ulp scales t about 7 (a = mnY) by 2^-23: (a - mnY) / R <= 1 where a threshold is, 7 * 2^-23 = 8.3e-7.
                //   t0             fma(mnY, inv, 1) rounds at magnitude 1 + mnY / R <= 1 / R (mnY <= 1 - R): 2^-24 / R, times 7 = 4.2e-7 / R.
                //   the pixel's fma  one rounding of a result in [0, 1]: 7 * 2^-25 = 2.1e-7.  r is exact (that IS RN), dist rounds at <= 1/2
                //                  (1.5e-8), and so does 1/2 - eps (3e-8).
                // In all |7 u - (t of the reference's own comparison)| < 1.09e-6 + 1.83e-6 / R.  A factor 2 over that is 2.2e-6 + 3.7e-6 / R;
                // the 1 / R part is set larger, so that the thresholds' term ALONE (1.41e-6 / R, three quarters of the whole for small R)
                // keeps a factor 4, as the location's terms (1.09e-6 + 0.42e-6 / R) then do as well:
                //   eps = 2.2e-6 + 5.7e-6 / R      (kAlphaEpsFixed, kAlphaEpsRange)
                // (tests/test_dxt_alpha_location_bound.py restates the stage in strict fp32 and holds each of the two to eps / 4).  The
                // mnY / R term is a seventh of the 1 / R part, so the pixels are not shifted by 4 mnY first (one more instruction each).
                // A clamped u (luma beyond an inset end) has dist = 0: decided, c = 0 or 7 as the reference counts.  An exact tie has
                // |dist| = 1/2 and is never certified: the reference's <= counts it, RN to even may not.  A wave that holds an
                // uncertified block does what the stage does for every other loader: thresholds, rows, g' and the reference's own
                // comparison for every pixel of all its blocks, from operands that pass through the empty asm so that nothing of that
                // side is formed ahead of the branch.  These fma only locate; no result of theirs is an operation of the reference.
                if constexpr (PAIRS && !kForceAlphaLinear) {
                        if (__builtin_expect(__all(range > 0.0009765625f), 1)) {
                                const float inv = __builtin_amdgcn_rcpf(range);
                                const float t0 = __builtin_fmaf(mnY, inv, 1.0f), ninv = inv * -0.25f;
                                float worst = 0.0f; // the block's largest |7 u - c|
#pragma unroll
                                for (int i = 14; i >= 0; i -= 2) { // two pixels per step: one v_max3_f32 with abs modifiers
                                        float dist[2];
#pragma unroll
                                        for (int h = 1; h >= 0; h--) {
                                                const float u = clamp01(__builtin_fmaf(Y[i + h], ninv, t0));
                                                const float r = __builtin_fmaf(u, 7.0f, kIndexBias); // the integer 2^23 + c
                                                uint32_t &acc = i >= 10 ? hi : lo;
                                                acc = (acc << 3) + __float_as_uint(r);
                                                dist[h] = __builtin_fmaf(u, 7.0f, kIndexBias - r);   // 7 u - c
                                        }
                                        worst = fmaxf(fmaxf(worst, fabsf(dist[0])), fabsf(dist[1]));
                                }
                                const float eps = __builtin_fmaf(kAlphaEpsRange, inv, kAlphaEpsFixed);
                                const lanemask_t certain = LANEMASK(worst < 0.5f - eps);
                                if (__builtin_expect(certain == LANEMASK(true), 1)) { // __all, on the comparison's own lane mask
                                        lo -= index_bias_sum(10, 3);
                                        hi -= index_bias_sum(6, 3);
                                        located = true;
                                } else {
                                        asm volatile("; alpha thresholds and comparisons" : "+v"(range), "+v"(mnY), "+v"(mxY) :: "memory");
                                        count_exact_alpha();
                                        lo = 0;
                                        hi = 0;
                                }
                        }
                }
                if (!located) {
                        const float inv7 = (float) (1.0 / 7.0);
                        // (mxY - mnY) / 14.0f.  div14() is bit-identical to the division for x = 0 and for every x >= 2^-100 (exhaustive
                        // device self-test); differences of byte-derived luma never fall in between, but the contract does not rest
                        // on that: a wave that sees such a value takes the IEEE division.
                        float mid = div14(range);
                        if (__builtin_expect(__any((__float_as_uint(range) - 1u) < (kDiv14Exact - 1u)), 0)) {
                                mid = range / 14.0f;
                        }
                        // ab[k] = 4 x the reference's threshold, bit for bit, for the comparisons with Y4.  The ends, range and mid stay
                        // the reference's (so the range test, div14 and its route to the IEEE division are untouched: nothing here divides a
                        // scaled value); the 4 goes into the multipliers, RN(4 (8 - k) mx) = 4 RN((8 - k) mx), of which one per threshold is
                        // 4, 8 or 16 and rides in the fma of the sum; * inv7 scales with its operand, and + mid becomes fma(mid, 4, .).
                        // ab[1] = RN(4 mn + 4 mid) takes the one multiplication this form adds.
                        float ab[8];
                        ab[1] = __builtin_fmaf(mid, 4.0f, mnY * 4.0f);
#pragma unroll
                        for (int k = 2; k <= 7; k++) {
                                const float cx_ = (float) (4 * (8 - k)), cn_ = (float) (4 * (k - 1));
                                const float sum = k <= 3 || k == 5 ? __builtin_fmaf(mnY, cn_, cx_ * mxY) : __builtin_fmaf(mxY, cx_, cn_ * mnY);
                                ab[k] = __builtin_fmaf(mid, 4.0f, sum * inv7);
                        }

                        // EmitAlphaIndicesYCoCgDXT5 (glsl:262-312): count c = #{k : a <= ab_k}, index = f(c).  Y[] holds Y4 and ab[] 4 x the thresholds
                        // Thresholds in ascending order are T1..T7 = ab1, ab7, ab6, ab5, ab4, ab3, ab2 whenever they are
                        // monotone (always, except degenerate blocks whose clamped min == max).  For a monotone set the
                        // count is a 3-step binary search (3 compares + 4 selects instead of 7 compares + 7 adds); it is
                        // the SAME function of (a, ab[]) as the reference's linear count, so results stay bit-identical.
                        const float T1 = ab[1], T2 = ab[7], T3 = ab[6], T4 = ab[5], T5 = ab[4], T6 = ab[3], T7 = ab[2];
                        // Monotone for sure when the clamped range exceeds 2^-10: consecutive thresholds are range/7 apart in exact
                        // arithmetic and each carries < 2^-22 of rounding error (operands <= 7, results <= 1), so 2^-10/7 of spacing
                        // cannot be overturned.  After the inset the range is >= 16/255/16 unless both ends clamp to the same bound,
                        // so one compare decides for practically every block; only a wave that sees a narrower range evaluates the six
                        // explicit comparisons.
                        bool all_mono, all_wide = false; // both wave-uniform
                        if (__builtin_expect(__all(range > 0.0009765625f), 1)) {
                                all_mono = true;
                                all_wide = true;
                        } else {
                                asm volatile("; explicit monotonicity check" ::: "memory");
                                count_full_form(1);
                                all_mono = __all((T1 <= T2) & (T2 <= T3) & (T3 <= T4) & (T4 <= T5) & (T5 <= T6) & (T6 <= T7));
                        }
                        // Fast form of the same count, valid under the wave-uniform range > 2^-10 test above.  The thresholds sit range/7
                        // apart (+- 2^-21), so the position of a among them is known from ONE multiply-add up to the nearest threshold:
                        //   t = 7 - (a - mnY) * 7/range (clamped to [0, 8)) puts threshold T(8-m) at t = m - 1/2  (m = 1..7, descending thresholds D_m = T(8-m));
                        //   g = trunc(t) (saturating at 0): every D_m with m <= g lies >= 0.49 steps above a, every D_m with m >= g + 2 lies
                        //   >= 0.49 steps below it (error of t < 6e-4 steps: rcp 1 ulp, mnY*inv rounded at magnitude <= 7168, fma rounding), so
                        //   c = #{m : a <= D_m} = g + (a <= D_(g+1)) -- and THAT comparison is the reference's own, on the reference's own
                        //   fp32 threshold (read back from the per-lane LDS column).  Row 7 = -inf serves g = 7 (a below every threshold).
                        // 1 fma + cvt + address + compare + 2 integer ops per pixel instead of 3 compares + 4 selects + 3 carries.
                        if (!kForceAlphaLinear && __builtin_expect(all_wide, 1)) {
                                float *const ta = tab.alpha;
                                ta[0 * 64] = T7; ta[1 * 64] = T6; ta[2 * 64] = T5; ta[3 * 64] = T4;
                                ta[4 * 64] = T3; ta[5 * 64] = T2; ta[6 * 64] = T1; ta[7 * 64] = -__builtin_inff();
                                // The same g without the conversion: u = (t - 1/2) / 7 = 6.5/7 - (a - mnY) / range with the clamp modifier (luma of
                                // YUV sources can lie far outside [mnY, mxY]), then r = fma(u, 7, 2^23): r is the integer 2^23 + RN(7 u), so the low
                                // bits of its pattern are g' = RN(clamp(t - 1/2, 0, 7)) = 0 .. 7.  g' = trunc(t) except where t is within its error
                                // (< 6e-4 steps as above: rcp 1 ulp, mnY * inv rounded at magnitude <= 1024, two fma roundings) of an integer, or
                                // exactly on it, where g' may be the neighbour of trunc(t).  There a lies 1/2 step from both nearest thresholds and
                                // both rows give the same count: row g: g + (a <= D_(g+1)) = g + 1 (D_(g+1) is 1/2 step ABOVE a), row g + 1:
                                // g + 1 + (a <= D_(g+2)) = g + 1 (D_(g+2) is 1/2 step BELOW a) -- the 0.49-step argument above covers either.
                                // These fma are locating arithmetic only: no result of theirs is an operation of the reference.
                                // The pattern kIndexBits + g' is used as it is: << 8 (the row offset) drops kIndexBits altogether, and the
                                // index words collect it as a known sum that is subtracted once per word (the true words are 30 and 18 bits).
                                const float inv = __builtin_amdgcn_rcpf(range);
                                // t as above from the reference's ends; the pixels are Y4, so their factor takes the 1/4 (exact: the same t)
                                const float t0 = __builtin_fmaf(mnY, inv, (float) (6.5 / 7.0)), ninv = inv * -0.25f;
                                constexpr int kA = kDxt5AlphaGroup;
#pragma unroll
                                for (int h = 16 / kA - 1; h >= 0; h--) { // groups of kA pixels: kA table reads in flight, bounded register use
                                        float D[kA];
                                        uint32_t g[kA];
#pragma unroll
                                        for (int j = kA - 1; j >= 0; j--) {
                                                g[j] = __float_as_uint(__builtin_fmaf(clamp01(__builtin_fmaf(Y[kA * h + j], ninv, t0)), 7.0f, kIndexBias));
                                                D[j] = *(const float *) ((const char *) ta + (uint32_t) (g[j] << 8)); // rows of 64 floats
                                        }
                                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                        for (int j = kA - 1; j >= 0; j--) {
                                                const int i = kA * h + j;
                                                uint32_t &acc = i >= 10 ? hi : lo;
                                                acc = add_mask((acc << 3) + g[j], LANEMASK(Y[i] <= D[j]));
                                        }
                                        __builtin_amdgcn_sched_barrier(0);
                                }
                                lo -= index_bias_sum(10, 3);
                                hi -= index_bias_sum(6, 3);
                        } else if (!kForceAlphaLinear && __builtin_expect(all_mono, 1)) {
#pragma unroll
                                for (int i = 15; i >= 0; i--) {
                                        const float a = Y[i];
                                        const bool g4 = a <= T4;
                                        const float t2 = g4 ? T2 : T6, t15 = g4 ? T1 : T5, t37 = g4 ? T3 : T7;
                                        const bool g2 = a <= t2;
                                        const float t1 = g2 ? t15 : t37;
                                        const bool g1 = a <= t1;
                                        uint32_t &acc = i >= 10 ? hi : lo;
                                        acc = shift_in(acc, LANEMASK(g4));
                                        acc = shift_in(acc, LANEMASK(g2));
                                        acc = shift_in(acc, LANEMASK(g1));
                                }
                        } else { // reference form, 7 compares per pixel, for every lane of the wave (degenerate blocks only)
                                // The empty asm keeps this a real branch: without it the compiler if-converts the two
                                // sides and every block pays for both.
                                asm volatile("; alpha linear fallback" ::: "memory");
#pragma unroll
                                for (int i = 15; i >= 0; i--) {
                                        const float a = Y[i];
                                        uint32_t c = 0;
#pragma unroll
                                        for (int k = 1; k <= 7; k++) {
                                                c += (a <= ab[k]) ? 1u : 0u;
                                        }
                                        uint32_t &acc = i >= 10 ? hi : lo;
                                        acc = (acc << 3) | c;
                                }
                        }
                }
                // index = ((c + 1) & 7) ^ (((c + 1) & 7) < 2)   (glsl:281-290), i.e. 0->0, 1..6 -> c+1, 7->1,
                // applied to all 3-bit fields of a word at once: with field bits (c2 c1 c0)
                //   i0 = (~c0 & (c1 | c2)) | (c0 & c1 & c2),  i1 = c1 ^ c0,  i2 = c2 ^ (c1 & c0)
                auto map_fields = [](uint32_t w) {
                        const uint32_t M = 0x09249249u; // bit 0 of every 3-bit field
                        const uint32_t c0 = w & M, c1 = (w >> 1) & M, c2 = (w >> 2) & M;
                        const uint32_t t = c1 & c0;
                        const uint32_t i0 = ((c0 ^ M) & (c1 | c2)) | (t & c2);
                        const uint32_t i1 = c1 ^ c0, i2 = c2 ^ t;
                        return i0 | (i1 << 1) | (i2 << 2);
                };
                lo = map_fields(lo);
                hi = map_fields(hi);
                // 48-bit index field F = lo | hi << 30: word0[31:16] = F[15:0], word1 = F[47:16]  (glsl:291-308)
                w0 |= lo << 16;
                w1 = (lo >> 16) | (hi << 14);
        }

        // EmitIndicesYCoCgDXT5 (glsl:217-250): the palette from the dequantised ends, then one 2-bit index per pixel
        uint32_t w_cidx = 0;
        {
                const float q1 = (float) (1.0 / 3.0), q2 = (float) (2.0 / 3.0);
                const float w1 = 1.0f - q1, w2 = 1.0f - q2;
                float cx[4], cy[4];
                cx[0] = cmx[0]; cy[0] = cmx[1];
                cx[1] = cmn[0]; cy[1] = cmn[1];
                cx[2] = lerp_w(cx[0], cx[1], w1, q1); cy[2] = lerp_w(cy[0], cy[1], w1, q1);
                cx[3] = lerp_w(cx[0], cx[1], w2, q2); cy[3] = lerp_w(cy[0], cy[1], w2, q2);
                // Fast form (wave-uniform choice).  The palette lies on the segment c0 -> c1 in the order c0, c2, c3, c1 (s = 0, 1/3, 2/3, 1)
                // and the index formula of glsl:237-244 is "nearest of the four": with s = the pixel's projection on the segment,
                //   b2 = [d0 > d2] flips at s = 1/6, b0 = [d0 > d3] at 1/3, b4 = [d2 > d3] at 1/2, b1 = [d1 > d2] at 2/3, b3 = [d1 > d3] at 5/6,
                //   bit0 = b0 & b4,  bit1 = (b1 & b2) | (b0 & b3).
                // In the third of the segment that holds the pixel (zone k = trunc(3 s), s clamped to [0, 1)) exactly ONE of the three
                // decisive comparisons (b2 | b4 | b3) is open; for the other bits either the pixel is >= 1/12 of the segment away
                // from the comparison's bisector, or the bit cannot change the result (b0 near 1/3 and b1 near 2/3 are masked by
                // their partners):   k = 0: index = 2 b2;   k = 1: index = 2 + b4;   k = 2: index = 1 + 2 b3.
                // The open comparison is evaluated exactly as the reference does (both squared distances in the reference's
                // operation order, strict >), so the result is the reference's whenever the "certain" bits are certain in fp32:
                //   a computed distance is off by < 2^-22 |p - c|^2 <= 2^-22 dmax (dmax = squared diagonal of the box around pixels and
                //   end points); two distances whose bisector is m segment-lengths away differ by >= (2/3) m vv (vv = |c1 - c0|^2).
                //   With vv * 256 > dmax and m >= 1/12 - 4e-4 that is > 200 x the rounding error; c2 / c3 are off their ideal
                //   places by < 2e-7 absolute = < 6e-5 of a segment with vv >= 1e-5 (a non-zero segment of 8-bit-expanded end points
                //   has vv >= 1.5e-5), and s itself is estimated to < 3e-4 (reciprocal + 5 roundings at magnitudes <= 650).
                // A wave that holds a block outside that precondition (coincident end points over non-flat chroma) runs the full form below for all lanes.
                //
                // One location per chroma pair (PAIRS).  The two pixels of a 4:2:2 pair come out of one yuv_pair_to_rgb
                // call: U, V and the products rv, gu, gv, bu are shared, only the luma term differs, and it cancels in Co = (r - b) / 2 + off
                // and Cg = (2 g - r - b) / 4 + off.  What is left is rounding: r, g, b, 2 g - r and (2 g - r) - b are rounded at magnitudes
                // < 4 (<= 2^-23 each), r - b and the final sums at magnitudes < 2 (<= 2^-24), which adds up to
                //   |dCo| <= 3.5 * 2^-23,  |dCg| <= 4 * 2^-23 < 5e-7
                // between the pixels of a pair (tests/test_dxt_pair_chroma_bound.py evaluates the statements in strict fp32 over every
                // (U, V) and finds 2.4e-7 for both).  The projection moves by |dCo ka + dCg kb| <= 5e-7 * sqrt(2) / sqrt(vv) < 2.3e-4 of the
                // segment with vv >= 1e-5.  So the zone found for the even pixel locates the odd one to < 3e-4 + 2.3e-4, and with the
                // rounded row (below) to < 7e-4: m >= 1/12 - 7e-4 still leaves > 200 x the rounding error.
                // A pair that straddles 1/3 or 2/3 needs no care: there either zone's formula gives the same index (at 1/3: 2 b2 = 2 =
                // 2 + b4, both 1/6 from their bisectors; at 2/3: 2 + b4 = 3 = 1 + 2 b3) -- the argument that lets a single pixel be
                // placed in either zone.  Each pixel of the pair then evaluates ITS OWN open comparison against that palette pair,
                // operands and order as in the reference.  The precondition below is the one of the per-pixel form: which waves take
                // which form stays a property of the content.
                //
                // Row from float bits: u = (3 s - 1/2) / 2 with the clamp modifier, r = fma(u, 2, 2^23) is the integer
                // 2^23 + RN(clamp(3 s - 1/2, 0, 2)): zone 0 for 3 s < 1, 1 up to 2, 2 above -- trunc(3 s) except within the error of s
                // around the borders (and RN's tie on them), which is the case of the paragraph above.  3/2 and -1/4 fold into ka, kb, kc.
                // These fma only locate; no result of theirs is an operation of the reference.  kIndexBits << 10 (rows of 64 float4)
                // is 0 mod 2^32, and the zone word collects kIndexBits as a known sum, subtracted once.
                //
                // Index from the projection (PAIRS).  The four palette entries are colinear up to the rounding of c2 and c3, so the three
                // bisectors of neighbouring entries are parallel, and in real arithmetic half of |p - A|^2 - |p - B|^2 across the bisector
                // between the k-th and the (k + 1)-th entry along the segment is  H_k(p) = (vv / 9) (3 s - k - 1/2):  the projection again.
                // Under the stage's precondition the index is "nearest of the four" (the zone argument above), so it is a function of
                // the projection alone:  j = RN(clamp(3 s, 0, 3)) picks c0, c2, c3, c1 for j = 0 .. 3.  The pair gets
                //   s = clamp(fma(Co, ka, fma(Cg, kb, kc)))   on its EVEN pixel,   k = v / vv,   kc = -(c0 . k) (rounded twice),
                //   r = fma(s, 3, 2^23) = the integer 2^23 + j (float bits, as the rows),   dist = fma(s, 3, 2^23 - r) = 3 s - j,
                // one 4-bit field per pair in a word, mapped to the index for all sixteen pixels at once (as map_fields does for alpha), and
                // a block is certified where max |dist| < 1/2 - eps over its eight pairs: no pair within eps of a half-integer of 3 s.
                // eps, in thirds of the segment, with u = 2^-24, l = sqrt(vv), |Co| < 1.5 and |Cg| < 1.2 (the YUV front ends: Co = 128 / 255
                // +- 0.98, Cg = 128 / 255 +- 0.68), palette coordinates in [0, 1], so |ka|, |kb| <= 1 / l and |c0 . k| <= sqrt(2) / l:
                //   evaluation     vv, its reciprocal (1 ulp) and the products by it are relative errors common to ka, kb, kc: they scale s
                //                  about c0 by < 5 u, < 1e-6 of a third where s is in [0, 1].  ka, kb rounded, in the pixel's fma: (1.5 +
                //                  1.2) u / l, in kc: 2 u / l;  kc's product and sum: (1 + 1.42) u / l;  the inner fma at magnitude <= (1.2 +
                //                  1.42) / l: 2.6 u / l;  the outer one and the two of r and dist at magnitude <= 3: negligible beside these.
                //                  9.7 u / l = 5.8e-7 / l in s, 1.75e-6 / l in thirds.
                //                  In the difference domain (the form below: s = fma(d, ka / 2, fma(e, kb / 4, kc')), kc' = fma(off - cx0, ka,
                //                  (off - cy0) kb), against the projection of the reference's own fp32 Co / Cg) the operands are smaller:
                //                  |d| / 2 <= 0.98, |e| / 4 <= 0.68, |off - c0| <= 0.71 as a vector and <= 0.51 per coordinate.  ka, kb rounded,
                //                  in the pixel's fma: (0.98 + 0.68) u / l, in kc': (0.51 + 0.51) u / l;  off - cx0, off - cy0 round at
                //                  magnitude <= 1/2 (u / 4 each, times |k|): 0.5 u / l;  kc's product and sum: (0.51 + 0.71) u / l;  the inner fma
                //                  at magnitude <= (0.68 + 0.71) / l: 1.39 u / l;  and Co's, Cg's own rounding, which the pixel no longer carries
                //                  into the projection but the reference's pixel has: |rho . k| <= 1.42 u / l.  7.2 u / l = 4.3e-7 / l in s,
                //                  1.3e-6 / l in thirds: under the 1.75e-6 / l the constants were set for, which stay as they are.
                //   the pair       the odd pixel is within 3.5 * 2^-23 in Co and 4 * 2^-23 in Cg of the even one (the pair-location
                //                  comment): |dp . k| <= 6.4e-7 / l in s, 1.9e-6 / l in thirds.
                //   c2, c3         each coordinate is two products and a sum below 1 (2^-25, 2^-26, 2^-25) with weights off 1/3, 2/3 by
                //                  < 4.5e-8: < 1.4e-7 per coordinate, delta < 2e-7 as a vector.  With n = B - A (ideal: v / 3) and m = (A + B) / 2,
                //                  H = n . (p - m) moves by dn . (p - m) - n . dm:  |dn| <= 2 delta, |p - m| <= sqrt(dmax) (both in the box),
                //                  |n . dm| <= (l / 3) delta.  Times 9 / vv:  3.6e-6 sqrt(dmax) / vv  (the tilt)  +  6e-7 / l  (the shift).
                //   the reference  each of da, db is off by < 2^-22 dmax (the fast form's own argument, above), half their difference by
                //                  < 2^-22 dmax:  2.15e-6 dmax / vv  in thirds.
                // In all |3 s - k - 1/2 - 9 H_k / vv| < (4.25e-6 l + 3.6e-6 sqrt(dmax) + 2.15e-6 dmax) / vv for either pixel of the pair, and
                //   eps = (8.5e-6 sqrt(vv) + 7.2e-6 sqrt(dmax) + 4.3e-6 dmax) / vv
                // keeps a factor 2 over the analysis (tests/test_dxt_pair_projection_bound.py restates the stage in strict fp32 and finds the fp32
                // projection within 0.05 eps of the one formed in double, and the projection margin within 0.04 eps of 9 H / vv).  A clamped s
                // (a pixel beyond an end of the segment) has dist = 0: decided.  An exact tie has |dist| = 1/2 and is never certified:
                // at 5/6 the reference's strict > gives c1 and RN could give either.  Flat blocks are certified as they are: their
                // word is replaced below.  A wave that holds an uncertified pair (a pixel next to a bisector: smooth gradients put some
                // there) does for that pair what the stage did before the index came from the projection: it finds the pair's zone from
                // RN(clamp(3 s - 1/2, 0, 2)) (the constants of the row paragraph above, formed on that side only), takes the zone's palette pair
                // (A, B) and evaluates the reference's two distances for the pair's two pixels, operands and order as in the reference; every
                // certified pair of the wave keeps the projection's index (the slot form, at the side).  These fma only locate; no result
                // of theirs is an operation of the reference.
                const float vx = cx[1] - cx[0], vy = cy[1] - cy[0];
                const float vv = vx * vx + vy * vy;
                const float e0 = fmaxf(fmaxf(mxCo, cx[0]), cx[1]) - fminf(fminf(mnCo, cx[0]), cx[1]);
                const float e1 = fmaxf(fmaxf(fmaxf(mxCg, mnCg), cy[0]), cy[1]) - fminf(fminf(fminf(mxCg, mnCg), cy[0]), cy[1]);
                const float dmax = e0 * e0 + e1 * e1;
                // A block whose 16 pixels share ONE chroma value (flat areas; its end points usually coincide) gets the reference's full
                // form for that one value, replicated; only a wave that holds such a block pays for it.
                const bool flat = (mnCo == mxCo) & (mnCg == mxCg);
                if (__builtin_expect(__all(((vv >= 1e-5f) & (vv * 256.0f > dmax)) | flat), 1)) {
                        float4 *const tc = tab.colour;
                        constexpr bool kProjection = PAIRS;
                        auto write_rows = [&](float ax, float ay, float bx, float by, float cx2, float cy2, float cx3, float cy3) {
                                tc[0 * 64] = make_float4(ax, ay, cx2, cy2);   // zone 0: d0 > d2
                                tc[1 * 64] = make_float4(cx2, cy2, cx3, cy3); // zone 1: d2 > d3
                                tc[2 * 64] = make_float4(bx, by, cx3, cy3);   // zone 2: d1 > d3
                        };
                        if constexpr (kProjection) {
                                const float rvv = __builtin_amdgcn_rcpf(vv);
                                const float ka = vx * rvv, kb = vy * rvv;
                                // the pixels are (d, e): Co ka + Cg kb + kc = d (ka / 2) + e (kb / 4) + (off - cx0) ka + (off - cy0) kb, the two
                                // scalings exact (kc' locates only, so it rounds twice; the derivation above counts both)
                                const float ka2 = ka * 0.5f, kb4 = kb * 0.25f;
                                const float kc = __builtin_fmaf(kOffset - cx[0], ka, (kOffset - cy[0]) * kb);
                                uint32_t jw = 0;      // kIndexBits + j per pair, 4 bits apart
                                float worst = 0.0f;   // the block's largest |3 s - j|
#pragma unroll
                                for (int grp = 3; grp >= 0; grp--) { // two pairs per step: one v_max3_f32 with abs modifiers
                                        float dist[2];
#pragma unroll
                                        for (int h = 1; h >= 0; h--) {
                                                const int i = 4 * grp + 2 * h;
                                                const float s = clamp01(__builtin_fmaf(Co[i], ka2, __builtin_fmaf(Cg[i], kb4, kc)));
                                                const float r = __builtin_fmaf(s, 3.0f, kIndexBias); // the integer 2^23 + j
                                                jw = (jw << 4) + __float_as_uint(r);
                                                dist[h] = __builtin_fmaf(s, 3.0f, kIndexBias - r);   // 3 s - j: the difference is exact
                                        }
                                        worst = fmaxf(fmaxf(worst, fabsf(dist[0])), fabsf(dist[1]));
                                }
                                const float sd = __builtin_amdgcn_sqrtf(dmax);
                                const float eps = __builtin_fmaf(sd, __builtin_fmaf(sd, kProjEpsDmax, kProjEpsDiag), kProjEpsSeg * __builtin_amdgcn_sqrtf(vv)) * rvv;
                                const lanemask_t certain = LANEMASK(worst < 0.5f - eps) | LANEMASK(flat);
                                if (__builtin_expect(certain == LANEMASK(true), 1)) { // __all, on the two comparisons' own lane masks
                                        jw -= index_bias_sum(8, 4);
                                        jw |= jw << 2; // pair j's field to pixel 2j + 1's as well
                                        // j -> index, all sixteen fields at once: 0 -> 0, 1 -> 2, 2 -> 3, 3 -> 1, that is bit 0 = j1, bit 1 = j1 ^ j0
                                        const uint32_t j1 = (jw >> 1) & 0x55555555u;
                                        w_cidx = j1 | (((jw ^ j1) & 0x55555555u) << 1);
                                } else {
                                        // The empty asm keeps this a real branch (see the alpha stage's fallback); vv passes through it so that
                                        // this side forms its own reciprocal and constants: nothing of it is computed ahead of the branch.
                                        // The slot form.  The certificate is per pair: `worst` is the maximum over the pairs and eps belongs to the
                                        // block, so every pair with |dist| < 1/2 - eps keeps the projection's index whatever the rest of the wave
                                        // holds.  The side forms the projection's word as the certified branch does, finds per pair slot k the lanes
                                        // whose pair k is uncertified (the main line's operations on the main line's operands: the same bits, so
                                        // the slots' masks add up to the complement of `certain`) and, behind a scalar branch per slot, gives the
                                        // two pixels of that slot the reference's distances; only the uncertified lanes take the result.
                                        // The word and the threshold pass through the asm as well: the side's arithmetic starts behind the branch.
                                        float vw = vv, thr = 0.5f - eps;
                                        uint32_t pw = jw;
                                        asm volatile("; per-pixel distances" : "+v"(vw), "+v"(pw), "+v"(thr) :: "memory");
                                        const float off = side_offset<PAIRS>();
                                        count_exact_pair();
                                        pw -= index_bias_sum(8, 4);
                                        pw |= pw << 2;
                                        const uint32_t p1 = (pw >> 1) & 0x55555555u;
                                        w_cidx = p1 | (((pw ^ p1) & 0x55555555u) << 1);
                                        const float rvw = __builtin_amdgcn_rcpf(vw);
                                        const float la = vx * rvw, lb = vy * rvw;
                                        const float la2 = la * 0.5f, lb4 = lb * 0.25f;
                                        const float lc = __builtin_fmaf(kOffset - cx[0], la, (kOffset - cy[0]) * lb);
                                        // the zone constants of the row paragraph above, as this side always formed them
                                        const float inv = 1.5f * rvw;
                                        const float za = vx * inv, zb = vy * inv;
                                        const float zc = __builtin_fmaf(-cx[0], za, __builtin_fmaf(-cy[0], zb, -0.25f));
                                        const lanemask_t notflat = ~LANEMASK(flat);
                                        uint32_t evaluated = 0; // wave-uniform
#pragma unroll
                                        for (int i = 14; i >= 0; i -= 2) {
                                                const float s = clamp01(__builtin_fmaf(Co[i], la2, __builtin_fmaf(Cg[i], lb4, lc)));
                                                const float r = __builtin_fmaf(s, 3.0f, kIndexBias);
                                                const float dist = __builtin_fmaf(s, 3.0f, kIndexBias - r);
                                                const bool uncertified = !(fabsf(dist) < thr) & !flat;
                                                if ((LANEMASK(!(fabsf(dist) < thr)) & notflat) != 0) { // scalar, on the comparison's own lane mask
                                                        asm volatile("; pair slot" ::: "memory"); // a real branch, as above
                                                        evaluated++;
                                                        const float co0 = co_of<PAIRS>(Co[i], off), cg0 = cg_of<PAIRS>(Cg[i], off); // the reference's pixels
                                                        const float co1 = co_of<PAIRS>(Co[i + 1], off), cg1 = cg_of<PAIRS>(Cg[i + 1], off);
                                                        const float sz = clamp01(__builtin_fmaf(co0, za, __builtin_fmaf(cg0, zb, zc)));
                                                        const uint32_t zone = __float_as_uint(__builtin_fmaf(sz, 2.0f, kIndexBias)) - kIndexBits; // 0, 1, 2
                                                        // the palette pair whose bisector crosses the zone: (c0, c2), (c2, c3), (c1, c3)
                                                        const bool z0 = zone == 0u, z1 = zone == 1u;
                                                        const float qx = z0 ? cx[0] : z1 ? cx[2] : cx[1], qy = z0 ? cy[0] : z1 ? cy[2] : cy[1];
                                                        const float qz = z0 ? cx[2] : cx[3], qw = z0 ? cy[2] : cy[3];
                                                        uint32_t nib = 0;
#pragma unroll
                                                        for (int h = 1; h >= 0; h--) {
                                                                const float co = h ? co1 : co0, cg = h ? cg1 : cg0;
                                                                const float ax = co - qx, ay = cg - qy, bx = co - qz, by = cg - qw;
                                                                const float da = ax * ax + ay * ay, db = bx * bx + by * by; // glsl:231-235, same operation order
                                                                const uint32_t c = da > db ? 1u : 0u, k0 = zone & 1u, k1 = zone >> 1;
                                                                nib = (nib << 2) | ((k0 & c) | k1) | ((k0 | c) << 1); // k = 0: 2 b2; 1: 2 + b4; 2: 1 + 2 b3
                                                        }
                                                        w_cidx = uncertified ? (w_cidx & ~(0xfu << (2 * i))) | (nib << (2 * i)) : w_cidx;
                                                }
                                        }
                                        count_pair_slots(evaluated);
                                }
                        } else {
                                write_rows(cx[0], cy[0], cx[1], cy[1], cx[2], cy[2], cx[3], cy[3]);
                                const float inv = 1.5f * __builtin_amdgcn_rcpf(vv);
                                const float ka = vx * inv, kb = vy * inv;
                                // (kc locates only, so it rounds twice, in two fma; s is then estimated no worse than above)
                                const float kc = __builtin_fmaf(-cx[0], ka, __builtin_fmaf(-cy[0], kb, -0.25f));
                                uint32_t zones = 0, open = 0; // 2-bit zone per pixel; the open comparison's result, one bit per pixel
                                // groups of kC pixels, the table reads of the next group issued before the distances of this one
                                constexpr int kC = kDxt5FastGroup, kGroups = 16 / kC;
                                float4 e[2][kC];
                                uint32_t kk[2][kC];
                                auto fetch = [&](int grp, int slot) {
#pragma unroll
                                        for (int j = kC - 1; j >= 0; j--) {
                                                const int i = kC * grp + j;
                                                const float s = clamp01(__builtin_fmaf(Co[i], ka, __builtin_fmaf(Cg[i], kb, kc)));
                                                kk[slot][j] = __float_as_uint(__builtin_fmaf(s, 2.0f, kIndexBias)); // kIndexBits + 0, 1, 2
                                                e[slot][j] = *(const float4 *) ((const char *) tc + (uint32_t) (kk[slot][j] << 10));
                                        }
                                };
                                fetch(kGroups - 1, (kGroups - 1) & 1);
#pragma unroll
                                for (int grp = kGroups - 1; grp >= 0; grp--) {
                                        const int slot = grp & 1;
                                        if (grp > 0) {
                                                fetch(grp - 1, slot ^ 1);
                                        }
                                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                        for (int j = kC - 1; j >= 0; j--) {
                                                const int i = kC * grp + j;
                                                const float4 q = e[slot][j];
                                                const float ax = Co[i] - q.x, ay = Cg[i] - q.y, bx = Co[i] - q.z, by = Cg[i] - q.w;
                                                const float da = ax * ax + ay * ay, db = bx * bx + by * by; // glsl:231-235, same operation order
                                                zones = (zones << 2) + kk[slot][j];
                                                open = shift_in(open, LANEMASK(da > db));
                                        }
                                        __builtin_amdgcn_sched_barrier(0);
                                }
                                zones -= index_bias_sum(16, 2);
                                const uint32_t c = spread16(open);
                                const uint32_t k0 = zones & 0x55555555u, k1 = (zones >> 1) & 0x55555555u;
                                w_cidx = ((k0 & c) | k1) | ((k0 | c) << 1);
                        }
                        if (__any(flat)) {
                                asm volatile("; flat blocks" ::: "memory");
                                const float off = side_offset<PAIRS>();
                                float4 p02, p13; // the palette, back from the table (not kept in registers) where the table holds it
                                if constexpr (kProjection) {
                                        p02 = make_float4(cx[0], cy[0], cx[2], cy[2]); p13 = make_float4(cx[1], cy[1], cx[3], cy[3]);
                                } else {
                                        p02 = tc[0 * 64]; p13 = tc[2 * 64];
                                }
                                const float px[4] = { p02.x, p13.x, p02.z, p13.z }, py[4] = { p02.y, p13.y, p02.w, p13.w };
                                const float co0 = co_of<PAIRS>(Co[0], off), cg0 = cg_of<PAIRS>(Cg[0], off); // pixel 0 stands for all sixteen
                                float d[4];
#pragma unroll
                                for (int k = 0; k < 4; k++) {
                                        const float tx = co0 - px[k], ty = cg0 - py[k];
                                        d[k] = tx * tx + ty * ty;
                                }
                                w_cidx = flat ? palette_index(d[0], d[1], d[2], d[3]) * 0x55555555u : w_cidx;
                        }
                } else {
                        asm volatile("; colour index full form" ::: "memory");
                        count_full_form(0);
                        w_cidx = emit_indices_ycocg_full_form<PAIRS>(Co, Cg, cx, cy, side_offset<PAIRS>());
                }
        }

        return make_uint4(w0, w1, w_end, w_cidx);
}

// ---------------------------------------------------------------------------------------
// DXT1 block encode, normative = GLSL (compress_dxt1_fp.glsl:177-229)
// ---------------------------------------------------------------------------------------
template <bool AWAY>
__device__ __forceinline__ uint2 encode_dxt1(const Px16 &p, const IndexTables &tab)
{
        const float *R = p.a, *G = p.b, *B = p.c;
        float mn[3] = { R[0], G[0], B[0] }, mx[3] = { R[0], G[0], B[0] };
#pragma unroll
        for (int i = 1; i < 16; i++) {
                mn[0] = fminf(mn[0], R[i]); mx[0] = fmaxf(mx[0], R[i]);
                mn[1] = fminf(mn[1], G[i]); mx[1] = fmaxf(mx[1], G[i]);
                mn[2] = fminf(mn[2], B[i]); mx[2] = fmaxf(mx[2], B[i]);
        }
        // SelectDiagonal (glsl:69-90)
        {
                const float cx = (mn[0] + mx[0]) * 0.5f, cy = (mn[1] + mx[1]) * 0.5f, cz = (mn[2] + mx[2]) * 0.5f;
                float cov_x = 0.0f, cov_y = 0.0f;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                        const float tx = R[i] - cx, ty = G[i] - cy, tz = B[i] - cz;
                        cov_x = cov_x + tx * tz;
                        cov_y = cov_y + ty * tz;
                }
                if (cov_x < 0.0f) { const float t = mx[0]; mx[0] = mn[0]; mn[0] = t; }
                if (cov_y < 0.0f) { const float t = mx[1]; mx[1] = mn[1]; mn[1] = t; }
        }
        // InsetBBox (glsl:92-97), RoundAndExpand + EmitEndPointsDXT1 (glsl:99-126)
        uint32_t cm[3], cn[3];
        {
                const float q[3] = { 31.0f, 63.0f, 31.0f };
#pragma unroll
                for (int k = 0; k < 3; k++) {
                        const float inset = (mx[k] - mn[k]) * 0.0625f - kInsetC;
                        const float lo = clamp01(mn[k] + inset), hi = clamp01(mx[k] - inset);
                        cm[k] = round_u32<AWAY>(hi * q[k]);
                        cn[k] = round_u32<AWAY>(lo * q[k]);
                }
        }
        const uint32_t code_max = (cm[0] << 11) | (cm[1] << 5) | cm[2];
        const uint32_t code_min = (cn[0] << 11) | (cn[1] << 5) | cn[2];
        cm[0] = (cm[0] << 3) | (cm[0] >> 2); cm[2] = (cm[2] << 3) | (cm[2] >> 2); cm[1] = (cm[1] << 2) | (cm[1] >> 4);
        cn[0] = (cn[0] << 3) | (cn[0] >> 2); cn[2] = (cn[2] << 3) | (cn[2] >> 2); cn[1] = (cn[1] << 2) | (cn[1] >> 4);
        const float inv255 = (float) (1.0 / 255.0);
        const bool swap = code_max < code_min;
        float c0[3], c1[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
                const float hi = (float) cm[k] * inv255, lo = (float) cn[k] * inv255;
                c0[k] = swap ? lo : hi;
                c1[k] = swap ? hi : lo;
        }
        const uint32_t w_end = swap ? (code_min | (code_max << 16)) : (code_max | (code_min << 16));

        // EmitIndicesDXT1 (glsl:128-161): packed fp32 over pixel pairs, as in the DXT5-YCoCg encoder
        uint32_t w_idx = 0;
        {
                const float q1 = (float) (1.0 / 3.0), q2 = (float) (2.0 / 3.0);
                const float w1 = 1.0f - q1, w2 = 1.0f - q2;
                float c2[3], c3[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                        c2[k] = lerp_w(c0[k], c1[k], w1, q1);
                        c3[k] = lerp_w(c0[k], c1[k], w2, q2);
                }
                // Fast form, as in the fast colour stage of encode_dxt5ycocg (the argument does not depend on the number of components): zone of the pixel's
                // projection on c0 -> c1, the one open comparison evaluated exactly as the reference does.  A distance of three squares
                // is off by < 2^-21 dmax, still > 100 x below the smallest certain difference under the same precondition; a non-zero
                // segment of 8-bit-expanded end points has vv >= 2.4e-4.  Coincident end points (flat blocks): full form for the wave.
                const float vx = c1[0] - c0[0], vy = c1[1] - c0[1], vz = c1[2] - c0[2];
                const float vv = vx * vx + vy * vy + vz * vz;
                float dmax = 0.0f;
#pragma unroll
                for (int k = 0; k < 3; k++) { // mn / mx may be swapped by SelectDiagonal
                        const float e = fmaxf(fmaxf(fmaxf(mx[k], mn[k]), c0[k]), c1[k]) - fminf(fminf(fminf(mx[k], mn[k]), c0[k]), c1[k]);
                        dmax = dmax + e * e;
                }
                const bool flat = (mn[0] == mx[0]) & (mn[1] == mx[1]) & (mn[2] == mx[2]); // one colour: full form for it, replicated
                if (__builtin_expect(__all(((vv >= 1e-5f) & (vv * 256.0f > dmax)) | flat), 1)) {
                        float4 *const tc = tab.colour;
                        tc[0 * 64] = make_float4(c0[0], c0[1], c0[2], 0.0f); tc[1 * 64] = make_float4(c2[0], c2[1], c2[2], 0.0f); // zone 0: d0 > d2
                        tc[2 * 64] = make_float4(c2[0], c2[1], c2[2], 0.0f); tc[3 * 64] = make_float4(c3[0], c3[1], c3[2], 0.0f); // zone 1: d2 > d3
                        tc[4 * 64] = make_float4(c1[0], c1[1], c1[2], 0.0f); tc[5 * 64] = make_float4(c3[0], c3[1], c3[2], 0.0f); // zone 2: d1 > d3
                        const float inv = __builtin_amdgcn_rcpf(vv);
                        const float ka = vx * inv, kb = vy * inv, kc = vz * inv;
                        const float kd = -((c0[0] * ka + c0[1] * kb) + c0[2] * kc);
                        uint32_t zones = 0, open = 0;
                        // groups of kG pixels; the table reads (2 x 12 bytes per pixel) of the next group are issued before the distances of this one
                        constexpr int kG = kDxt1FastGroup;
                        struct alignas(16) F3 { float x, y, z; };
                        F3 ea[2][kG], eb[2][kG];
                        uint32_t kk[2][kG];
                        auto fetch = [&](int grp, int slot) {
#pragma unroll
                                for (int j = kG - 1; j >= 0; j--) {
                                        const int i = kG * grp + j;
                                        const float t = clamp01(__builtin_fmaf(R[i], ka, __builtin_fmaf(G[i], kb, __builtin_fmaf(B[i], kc, kd))));
                                        kk[slot][j] = cvt_u32_sat(t * 2.9999998f); // 0, 1, 2
                                        const F3 *const q = (const F3 *) (tc + kk[slot][j] * 128);
                                        ea[slot][j] = q[0];
                                        eb[slot][j] = q[64];
                                }
                        };
                        constexpr int kGroups = 16 / kG;
                        fetch(kGroups - 1, (kGroups - 1) & 1);
#pragma unroll
                        for (int grp = kGroups - 1; grp >= 0; grp--) {
                                const int slot = grp & 1;
                                if (grp > 0) {
                                        fetch(grp - 1, slot ^ 1);
                                }
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int j = kG - 1; j >= 0; j--) {
                                        const int i = kG * grp + j;
                                        const F3 qa = ea[slot][j], qb = eb[slot][j];
                                        const float ax = R[i] - qa.x, ay = G[i] - qa.y, az = B[i] - qa.z;
                                        const float bx = R[i] - qb.x, by = G[i] - qb.y, bz = B[i] - qb.z;
                                        const float da = AWAY ? (ax * ax + ay * ay) + az * az : (az * az + ay * ay) + ax * ax; // as d[k] below
                                        const float db = AWAY ? (bx * bx + by * by) + bz * bz : (bz * bz + by * by) + bx * bx;
                                        zones = (zones << 2) + kk[slot][j];
                                        open = shift_in(open, LANEMASK(da > db));
                                }
                                __builtin_amdgcn_sched_barrier(0);
                        }
                        const uint32_t c = spread16(open), k0 = zones & 0x55555555u, k1 = (zones >> 1) & 0x55555555u;
                        w_idx = ((k0 & c) | k1) | ((k0 | c) << 1);
                        if (__any(flat)) {
                                asm volatile("; flat blocks" ::: "memory");
                                const float4 pal[4] = { tc[0 * 64], tc[4 * 64], tc[1 * 64], tc[3 * 64] }; // the palette, back from the table
                                float d[4];
#pragma unroll
                                for (int k = 0; k < 4; k++) {
                                        const float tx = R[0] - pal[k].x, ty = G[0] - pal[k].y, tz = B[0] - pal[k].z;
                                        d[k] = AWAY ? (tx * tx + ty * ty) + tz * tz : (tz * tz + ty * ty) + tx * tx;
                                }
                                w_idx = flat ? palette_index(d[0], d[1], d[2], d[3]) * 0x55555555u : w_idx;
                        }
                } else {
                asm volatile("; colour index full form" ::: "memory");
                count_full_form(0);
                const float *c[4] = { c0, c1, c2, c3 };
                f32x2 cc[4][3];
#pragma unroll
                for (int k = 0; k < 4; k++) {
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
                                cc[k][ch] = (f32x2) { c[k][ch], c[k][ch] };
                        }
                }
#pragma unroll
                for (int i = 14; i >= 0; i -= 2) {
                        const f32x2 r = { R[i], R[i + 1] }, g = { G[i], G[i + 1] }, bl = { B[i], B[i + 1] };
                        f32x2 d[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                                const f32x2 tx = r - cc[k][0], ty = g - cc[k][1], tz = bl - cc[k][2];
                                d[k] = AWAY ? (tx * tx + ty * ty) + tz * tz  // dot(v,v): x*x + y*y + z*z, left to right (cuda_dxt.cu:106-108)
                                            : (tz * tz + ty * ty) + tx * tx; // Mesa sums dot(vec3) from the last component
                        }
#pragma unroll
                        for (int h = 1; h >= 0; h--) {
                                w_idx = shift_in_palette_index(w_idx, d[0][h], d[1][h], d[2][h], d[3][h]);
                        }
                }
                }
        }
        return make_uint2(w_end, w_idx);
}

// ---------------------------------------------------------------------------------------
// kernel.  Workgroup = 64 x 4 lanes: wave w of the group encodes 64 consecutive units of block row
// blockIdx.y*4 + w (unit = Loader::kBlocks consecutive blocks), blockIdx.z = image of the batch.
// No integer division anywhere; lanes idle only at the right/bottom edge of the block grid.
// ---------------------------------------------------------------------------------------
// Occupancy target of the register allocator.  With the fast index stages the DXT5-YCoCg kernels need 100 VGPRs at 4 waves per SIMD
// or 96 at 5 (the five dwords that do not fit are spilled in the rarely taken full-form colour stage only): 5 measures 2.4 % faster
// (profiles/r03_fast_index_ab.txt).  The v210 kernels (three blocks per lane) keep the allocator's own choice.
constexpr int kMinWaves = 5;
// A wave can walk kRowsPerWave consecutive block rows, issuing the loads of row j+1 before it encodes row j.
// Measured on MI355X (interleaved A/B, 16 x 4K UYVY->DXT5): 1 row 0.2004 ms, 2 rows 0.2157, 4 rows 0.2224, 8 rows
// 0.2230 -- the prefetching loop LOSES (VGPR 104 -> 126, no cross-row scheduling), so a wave encodes one row and
// latency hiding is left to the resident waves.  With a trip count of one the loop and `nxt` compile to nothing.  They are still here only because
// deleting them changed the instruction ORDER of the DXT5-YCoCg kernels (same instructions), and the change that fixed this constant had to leave the
// compiler's output as it was; whoever next re-times these kernels can delete the loop.
constexpr int kRowsPerWave = 1;

template <int IN, int OUT, bool MIRROR, bool AWAY, bool EDGE>
__global__ __launch_bounds__(256, (Loader<IN>::kBlocks > 1 ? 1 : kMinWaves)) void dxt_encode_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                         int units_per_row, int blocks_per_row, int block_rows, int height, uint32_t pitch,
                                                         size_t src_frame_stride, size_t dst_frame_stride, int width)
{
        using L = Loader<IN>;
        constexpr bool kAlpha = OUT == UG_DXT5_YCOCG;
        constexpr int kColourRows = OUT == UG_DXT5_YCOCG ? 3 : 6;
        __shared__ float lds_alpha[kAlpha ? 4 * 8 * 64 : 1];
        __shared__ float4 lds_colour[4 * kColourRows * 64];
        IndexTables tab;
        {
                const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
                tab.alpha = lds_alpha + (kAlpha ? wave * (8 * 64) + (int) threadIdx.x : 0);
                tab.colour = lds_colour + (wave * (kColourRows * 64) + (int) threadIdx.x);
        }
        // threadIdx.y is wave-uniform (a wave is one 64-lane row of the group): keep the block row, the row base
        // pointers and the bounds test on the scalar unit -- no per-lane 64-bit multiplies in the prologue.
        const int ux = blockIdx.x * 64 + threadIdx.x;
        const int by0 = (int) (blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y)) * kRowsPerWave;
        if (by0 >= block_rows) {
                return;
        }
        if (ux >= units_per_row) {
                return;
        }
        src += (size_t) blockIdx.z * src_frame_stride;
        dst += (size_t) blockIdx.z * dst_frame_stride;

        auto load_row = [&](L &ld, int by) {
                int rows[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                        const int y = EDGE ? min(4 * by + r, height - 1) : 4 * by + r; // (scalar) lines past the picture repeat its last line
                        rows[r] = MIRROR ? height - 1 - y : y; // cuda_dxt.cu:652-655
                }
                if constexpr (EDGE && L::kBlocks == 1) {
                        const int valid = width - 4 * ux; // pixel columns of this lane's block that lie inside the picture
                        if (valid < 4) { // one lane per block row, when width % 4 != 0
                                ld.load_edge(src, pitch, ux, rows, valid);
                                return;
                        }
                }
                ld.template load<EDGE>(src, pitch, ux, rows);
        };
        L cur, nxt;
        load_row(cur, by0);
#pragma unroll 1
        for (int j = 0; j < kRowsPerWave; j++) {
                const int by = by0 + j;
                if (by >= block_rows) { // wave-uniform
                        break;
                }
                const bool more = j + 1 < kRowsPerWave && by + 1 < block_rows;
                if (more) {
                        load_row(nxt, by + 1);
                }
                // block raster order idx = bx + (w/4)*by (cuda_dxt.cu:633)
                constexpr uint32_t kBlockBytes = OUT == UG_DXT5_YCOCG ? 16 : 8;
                uint8_t *const dst_row = dst + (size_t) by * blocks_per_row * kBlockBytes; // scalar
                const uint32_t dst_off = (uint32_t) ux * (L::kBlocks * kBlockBytes);
                // A lane with several blocks (v210: 3) keeps them and stores them together at the end: stored one by one, a thousand instructions
                // apart, the three 16-byte pieces of a lane's 48 bytes reached HBM as partial lines (WRITE_SIZE 1.5 x the output, rocprofv3)
                uint4 res[L::kBlocks];
                int n_res = 0;
#pragma unroll
                for (int k = 0; k < L::kBlocks; k++) {
                        // v210, width % 12 != 0 (1280, 2048 ...): the last 32-byte unit of a line holds one or two blocks; its loads
                        // stay inside the 128-byte-padded line (video_codec.c:507-521), the blocks past the picture are not emitted
                        if (L::kBlocks > 1 && k > 0 && ux * L::kBlocks + k >= blocks_per_row) {
                                break;
                        }
                        Px16 p;
                        if constexpr (EDGE && L::kBlocks > 1) {
                                cur.block_edge(k, p, width - 4 * (ux * L::kBlocks + k) < 4);
                        } else {
                                cur.block(k, p);
                        }
                        if (OUT == UG_DXT5_YCOCG) {
                                res[k] = encode_dxt5ycocg<AWAY, L::kChromaPairs>(p, tab);
                        } else {
                                const uint2 e = encode_dxt1<AWAY>(p, tab);
                                res[k] = make_uint4(e.x, e.y, 0, 0);
                        }
                        n_res = k + 1;
                }
#pragma unroll
                for (int k = 0; k < L::kBlocks; k++) {
                        if (k < n_res) {
                                // One block per lane: a store instruction covers whole lines (64 x 16 B / 64 x 8 B contiguous) and streams past L2.
                                // Three blocks per lane (v210): an instruction writes 16 of every 48 bytes and the lines complete only with the
                                // third one -- streamed, the pieces reached HBM separately (WRITE_SIZE 157 MB for 132.7 MB of output, rocprofv3),
                                // so these go through L2 as plain stores and merge there (1.001 x).
                                uint8_t *const at = dst_row + (dst_off + k * kBlockBytes);
                                if (OUT == UG_DXT5_YCOCG) {
                                        if (L::kBlocks > 1) *(uint4 *) at = res[k]; else ug::st_stream((uint4 *) at, res[k]);
                                } else {
                                        const uint2 v = make_uint2(res[k].x, res[k].y);
                                        if (L::kBlocks > 1) *(uint2 *) at = v; else ug::st_stream((uint2 *) at, v);
                                }
                        }
                }
                if (more) {
                        cur = nxt;
                }
        }
}

// exhaustive check of div14() against the IEEE division over x = 0 and every fp32 bit pattern in [2^-100, 1]
__global__ void selftest_div14_kernel(unsigned *mismatches)
{
        const unsigned long long i = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x;
        if (i > 0x3f800000ull || (i != 0 && i < kDiv14Exact)) return;
        const float x = __uint_as_float((unsigned) i);
        volatile float d = 14.0f;
        const float want = x / d;
        if (__float_as_uint(div14(x)) != __float_as_uint(want)) atomicAdd(mismatches, 1u);
}

struct EncodeJob {
        const void *src;
        void *dst;
        int w, h, pitch, frames;
        size_t sfs, dfs;
        hipStream_t st;
};

template <int IN, int OUT, bool AWAY>
int launch(const EncodeJob &j)
{
        using L = Loader<IN>;
        const bool mirror = j.h < 0;
        const int h = mirror ? -j.h : j.h;
        const int bpr = (j.w + 3) / 4, upr = (bpr + L::kBlocks - 1) / L::kBlocks, brows = (h + 3) / 4; // dxt_util.h:59-67
        const bool edge = (j.w & 3) || (h & 3);
        if (upr == 0 || brows == 0 || j.frames == 0) return UG_HIP_SUCCESS;
        constexpr int wg_rows = 4; // waves per workgroup; 1, 2 and 4 measure the same (0.1878-0.1889 ms)
        const int rows_per_group = wg_rows * kRowsPerWave;
        if ((uint64_t) j.pitch * (uint64_t) h > 0xffffffffull) { // in-frame byte offsets are 32-bit (scalar base + lane offset)
                ug::set_last_error_msg("ug_hip_dxt_encode: image larger than 4 GiB");
                return UG_HIP_EINVAL;
        }
        if (j.frames > 65535 || (brows + rows_per_group - 1) / rows_per_group > 65535) {
                ug::set_last_error_msg("ug_hip_dxt_encode: image too tall / too many frames for one launch");
                return UG_HIP_EINVAL;
        }
        const dim3 block(64, wg_rows), grid((unsigned) ((upr + 63) / 64), (unsigned) ((brows + rows_per_group - 1) / rows_per_group), (unsigned) j.frames);
#define UG_LAUNCH_DXT(MIRROR, EDGE) hipLaunchKernelGGL((dxt_encode_kernel<IN, OUT, MIRROR, AWAY, EDGE>), grid, block, 0, j.st, (const uint8_t *) j.src, \
                                                      (uint8_t *) j.dst, upr, bpr, brows, h, (uint32_t) j.pitch, j.sfs, j.dfs, j.w)
        if (edge) {
                if (mirror) UG_LAUNCH_DXT(true, true); else UG_LAUNCH_DXT(false, true);
        } else {
                if (mirror) UG_LAUNCH_DXT(true, false); else UG_LAUNCH_DXT(false, false);
        }
#undef UG_LAUNCH_DXT
        UG_HIP_LAUNCH_CHECK();
        return UG_HIP_SUCCESS;
}

template <int IN>
int launch_out(ug_dxt_t out, int ties, const EncodeJob &j)
{
        const bool away = ties == UG_DXT_TIES_AWAY;
        switch (out) {
        case UG_DXT1: return away ? launch<IN, UG_DXT1, true>(j) : launch<IN, UG_DXT1, false>(j);
        case UG_DXT5_YCOCG: return away ? launch<IN, UG_DXT5_YCOCG, true>(j) : launch<IN, UG_DXT5_YCOCG, false>(j);
        default: break; // UG_DXT1_YUV is rewritten to UG_DXT1 over raw UYVY by the caller
        }
        return UG_HIP_EUNSUPP;
}

} // namespace

extern "C" {

size_t ug_hip_dxt_size(ug_dxt_t out, int width, int height)
{
        if (!ug::dims_ok_signed(width, height)) return 0; // not a picture: no size (never a wrapped one)
        if (height < 0) height = -height;
        const size_t px = ((size_t) width + 3) / 4 * 4 * (((size_t) height + 3) / 4 * 4); // dxt_util.h:59-67: whole 4x4 blocks
        return out == UG_DXT1 || out == UG_DXT1_YUV ? px / 2 : px;
}

int ug_hip_dxt_encode_batch_ex(ug_pixfmt_t in, ug_dxt_t out, const void *src, void *dst, int width, int height,
                               int src_pitch, int frames, size_t src_frame_stride, size_t dst_frame_stride, int ties,
                               ug_hip_stream_t stream)
{
        if (!ug::dims_ok_signed(width, height)) return ug::refuse_size("ug_hip_dxt_encode");
        const int ah = height < 0 ? -height : height;
        if (out == UG_DXT1_YUV) { // DXT1 over the Y,Cb,Cr samples: UYVY is its only input (dxt_glsl.cpp:104-110)
                if (in != UG_PF_UYVY && in != UG_PF_UYVY_RAW) {
                        ug::set_last_error_msg("ug_hip_dxt_encode: DXT1_YUV takes UYVY input only");
                        return UG_HIP_EUNSUPP;
                }
                in = UG_PF_UYVY_RAW;
                out = UG_DXT1;
        }
        if (ties != UG_DXT_TIES_EVEN && ties != UG_DXT_TIES_AWAY) {
                ug::set_last_error_msg("ug_hip_dxt_encode: unknown tie rule");
                return UG_HIP_EINVAL;
        }
        if (!src || !dst || width <= 0 || ah == 0 || frames < 0 || (15 & (uintptr_t) src) || (15 & (uintptr_t) dst)) {
                ug::set_last_error_msg("ug_hip_dxt_encode: bad size or alignment");
                return UG_HIP_EINVAL;
        }
        // Any width and height >= 1, as dxt_encoder_create takes them (dxt_glsl.cpp:150-160); the cuda_dxt.h-shaped entry points below keep
        // cuda_dxt.cu:745's multiples of 4.  A 4:2:2 line is made of pixel pairs.
        const bool edge = (width & 3) || (ah & 3);
        if ((width & 1) && (in == UG_PF_UYVY || in == UG_PF_UYVY_RAW || in == UG_PF_V210)) {
                ug::set_last_error_msg("ug_hip_dxt_encode: 4:2:2 input needs an even width");
                return UG_HIP_EINVAL;
        }
        if (src_pitch == 0) {
                src_pitch = ug::linesize(in, width);
        }
        const bool any_pitch = edge && (in == UG_PF_RGB || in == UG_PF_YUV444); // lines of 3 * width bytes start wherever they start
        if (src_pitch <= 0 || ((src_pitch & 3) && !any_pitch)) {
                ug::set_last_error_msg("ug_hip_dxt_encode: bad pitch / unsupported input format");
                return src_pitch <= 0 ? UG_HIP_EUNSUPP : UG_HIP_EINVAL;
        }
        if (!ug::span_ok(src_pitch, ah)) return ug::refuse_size("ug_hip_dxt_encode");
        if (frames > 1 && ((src_frame_stride & 15) || (dst_frame_stride & 15))) {
                ug::set_last_error_msg("ug_hip_dxt_encode: frame strides must be multiples of 16");
                return UG_HIP_EINVAL;
        }
        const EncodeJob j = { src, dst, width, height, src_pitch, frames, src_frame_stride, dst_frame_stride, (hipStream_t) stream };
        switch (in) {
        case UG_PF_RGB: return launch_out<UG_PF_RGB>(out, ties, j);
        case UG_PF_RGBA:
                if (src_pitch & (edge ? 3 : 15)) break;
                return launch_out<UG_PF_RGBA>(out, ties, j);
        case UG_PF_YUV444: return launch_out<UG_PF_YUV444>(out, ties, j);
        case UG_PF_UYVY:
                if (src_pitch & (edge ? 3 : 7)) break;
                return launch_out<UG_PF_UYVY>(out, ties, j);
        case UG_PF_UYVY_RAW:
                if (src_pitch & (edge ? 3 : 7)) break;
                return launch_out<UG_PF_UYVY_RAW>(out, ties, j);
        case UG_PF_V210:
                // 12 px = 32 B units; a last unit with fewer pixels is read whole, which the 128-byte line padding of v210
                // (vc_get_linesize, video_codec.c:507-521) always covers -- a caller-supplied pitch must cover it too
                if ((src_pitch & 15) || src_pitch < (width + 11) / 12 * 32) break;
                return launch_out<UG_PF_V210>(out, ties, j);
        default:
                ug::set_last_error_msg("ug_hip_dxt_encode: unsupported input format");
                return UG_HIP_EUNSUPP;
        }
        ug::set_last_error_msg("ug_hip_dxt_encode: pitch/width not aligned for this input format");
        return UG_HIP_EINVAL;
}

int ug_hip_dxt_encode_batch(ug_pixfmt_t in, ug_dxt_t out, const void *src, void *dst, int width, int height,
                            int src_pitch, int frames, size_t src_frame_stride, size_t dst_frame_stride,
                            ug_hip_stream_t stream)
{
        return ug_hip_dxt_encode_batch_ex(in, out, src, dst, width, height, src_pitch, frames, src_frame_stride, dst_frame_stride,
                                          UG_DXT_TIES_DEFAULT, stream);
}

int ug_hip_dxt_encode(ug_pixfmt_t in, ug_dxt_t out, const void *src, void *dst, int width, int height, int src_pitch,
                      ug_hip_stream_t stream)
{
        return ug_hip_dxt_encode_batch_ex(in, out, src, dst, width, height, src_pitch, 1, 0, 0, UG_DXT_TIES_DEFAULT, stream);
}

// cuda_dxt.h-shaped entry points: the interface of cuda_dxt.h:30-89 with its own limits -- sizes that are multiples of 4 (cuda_dxt.cu:745)
static int cuda_dxt_shaped(ug_pixfmt_t in, ug_dxt_t out, const void *src, void *dst, int sx, int sy, ug_hip_stream_t s)
{
        if ((sx & 3) || (sy & 3)) {
                ug::set_last_error_msg("ug_hip_*_to_dxt*: width and height must be multiples of 4 (cuda_dxt.cu:745); ug_hip_dxt_encode takes any size");
                return UG_HIP_EINVAL;
        }
        return ug_hip_dxt_encode(in, out, src, dst, sx, sy, 0, s);
}
int ug_hip_rgb_to_dxt1(const void *src, void *out, int sx, int sy, ug_hip_stream_t s) { return cuda_dxt_shaped(UG_PF_RGB, UG_DXT1, src, out, sx, sy, s); }
int ug_hip_yuv_to_dxt1(const void *src, void *out, int sx, int sy, ug_hip_stream_t s) { return cuda_dxt_shaped(UG_PF_YUV444, UG_DXT1, src, out, sx, sy, s); }
int ug_hip_rgb_to_dxt6(const void *src, void *out, int sx, int sy, ug_hip_stream_t s) { return cuda_dxt_shaped(UG_PF_RGB, UG_DXT5_YCOCG, src, out, sx, sy, s); }
int ug_hip_yuv_to_dxt6(const void *src, void *out, int sx, int sy, ug_hip_stream_t s) { return cuda_dxt_shaped(UG_PF_YUV444, UG_DXT5_YCOCG, src, out, sx, sy, s); }

int ug_hip_time_dxt_encode(ug_pixfmt_t in, ug_dxt_t out, const void *src, void *dst, int width, int height,
                           int src_pitch, int frames, size_t sfs, size_t dfs, int iters, ug_hip_stream_t stream,
                           float *ms_per_launch)
{
        if (!ms_per_launch || iters <= 0) return UG_HIP_EINVAL;
        hipStream_t st = (hipStream_t) stream;
        int rc = ug_hip_dxt_encode_batch(in, out, src, dst, width, height, src_pitch, frames, sfs, dfs, stream); // warm; refuses bad arguments before any device call
        if (rc != UG_HIP_SUCCESS) return rc;
        hipEvent_t e0, e1;
        UG_HIP_TRY(hipEventCreate(&e0));
        UG_HIP_TRY(hipEventCreate(&e1));
        {
                (void) hipEventRecord(e0, st);
                for (int i = 0; i < iters && rc == UG_HIP_SUCCESS; i++) {
                        rc = ug_hip_dxt_encode_batch(in, out, src, dst, width, height, src_pitch, frames, sfs, dfs, stream);
                }
                (void) hipEventRecord(e1, st);
                hipError_t e = hipEventSynchronize(e1);
                if (e != hipSuccess) {
                        ug::set_last_error(e, "hipEventSynchronize");
                        rc = UG_HIP_ERUNTIME;
                } else {
                        float ms = 0;
                        (void) hipEventElapsedTime(&ms, e0, e1);
                        *ms_per_launch = ms / iters;
                }
        }
        (void) hipEventDestroy(e0);
        (void) hipEventDestroy(e1);
        return rc;
}

} // extern "C"

// Diagnostics: waves of this process's ug_hip_dxt_encode* launches on the current device that took the full form of an index stage
// the sum over the slots of one counter, `offset` bytes into its symbol
static int sum_slotted(const void *symbol, size_t offset, unsigned long long *sum)
{
        static unsigned long long lines[kCounterWords]; // (the callers synchronise the device: diagnostics, one caller at a time)
        UG_HIP_TRY(hipMemcpyFromSymbol(lines, symbol, sizeof lines, offset));
        *sum = 0;
        for (int i = 0; i < kPairSlots; i++) *sum += lines[i * kPairSlotStride];
        return UG_HIP_SUCCESS;
}
extern "C" int ug_hip_dxt_encode_stats(unsigned long long full_form_waves[2], int reset)
{
        UG_HIP_TRY(hipDeviceSynchronize());
        if (full_form_waves) {
                for (int which = 0; which < 2; which++) {
                        const int rc = sum_slotted(HIP_SYMBOL(g_full_form_waves), which * sizeof(unsigned long long[kCounterWords]), &full_form_waves[which]);
                        if (rc != UG_HIP_SUCCESS) return rc;
                }
        }
        if (reset) {
                static const unsigned long long none[2][kCounterWords] = {};
                UG_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_full_form_waves), none, sizeof none));
                UG_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_exact_cov_waves), none, sizeof none[0]));
                UG_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_exact_pair_waves), none, sizeof none[0]));
                UG_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pair_slot_evaluations), none, sizeof none[0]));
                UG_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_exact_alpha_waves), none, sizeof none[0]));
        }
        return UG_HIP_SUCCESS;
}

// The same with the counters of the certified stages: counts[0 .. n - 1] of { colour full form, alpha full form, exact covariance sum,
// per-pixel distances after the colour stage's projection }
extern "C" int ug_hip_dxt_encode_stats_ex(unsigned long long *counts, int n, int reset)
{
        if (n < 0 || n > 4 || (n > 0 && !counts)) return UG_HIP_EINVAL;
        unsigned long long all[4] = { 0, 0, 0, 0 };
        UG_HIP_TRY(hipDeviceSynchronize());
        if (n > 0) {
                int rc = ug_hip_dxt_encode_stats(all, 0);
                if (rc == UG_HIP_SUCCESS) rc = sum_slotted(HIP_SYMBOL(g_exact_cov_waves), 0, &all[2]);
                if (rc == UG_HIP_SUCCESS) rc = sum_slotted(HIP_SYMBOL(g_exact_pair_waves), 0, &all[3]);
                if (rc != UG_HIP_SUCCESS) return rc;
                for (int i = 0; i < n; i++) counts[i] = all[i];
        }
        return reset ? ug_hip_dxt_encode_stats(nullptr, 1) : UG_HIP_SUCCESS;
}

// Of the waves of counts[3] above: the pair slots that were evaluated.  The side of the colour stage's projection keeps the projection's
// index for every certified pair and forms the reference's two distances only for the pixels of a pair slot (0 .. 7) in which some lane
// of the wave holds an uncertified pair; *slot_evaluations (may be NULL) receives the number of such (wave, slot) evaluations, between
// 1 and 8 for every wave that counts[3] counted.  Any reset clears this counter too.
extern "C" int ug_hip_dxt_encode_stats_pair_slots(unsigned long long *slot_evaluations, int reset)
{
        UG_HIP_TRY(hipDeviceSynchronize());
        if (slot_evaluations) {
                const int rc = sum_slotted(HIP_SYMBOL(g_pair_slot_evaluations), 0, slot_evaluations);
                if (rc != UG_HIP_SUCCESS) return rc;
        }
        return reset ? ug_hip_dxt_encode_stats(nullptr, 1) : UG_HIP_SUCCESS;
}

// The counter of the alpha stage's count from the location (4:2:2 sources -> DXT5-YCoCg): waves that held a block whose location
// was not certified and went on to the thresholds and the reference's comparison.  An entry point of its own: counts[0 .. 3] above
// keep their number and their meaning.  Either reset above clears this counter too.
extern "C" int ug_hip_dxt_encode_stats_alpha(unsigned long long *exact_waves, int reset)
{
        UG_HIP_TRY(hipDeviceSynchronize());
        if (exact_waves) {
                const int rc = sum_slotted(HIP_SYMBOL(g_exact_alpha_waves), 0, exact_waves);
                if (rc != UG_HIP_SUCCESS) return rc;
        }
        return reset ? ug_hip_dxt_encode_stats(nullptr, 1) : UG_HIP_SUCCESS;
}

// Device self-test of the encoder's exact strength reductions (div14): *mismatches must come back 0.
extern "C" int ug_hip_selftest_dxt_encode(unsigned *mismatches, ug_hip_stream_t stream)
{
        if (!mismatches) return UG_HIP_EINVAL;
        unsigned *dev = nullptr;
        UG_HIP_TRY(hipMalloc((void **) &dev, sizeof *dev));
        hipStream_t st = (hipStream_t) stream;
        hipError_t err = hipMemsetAsync(dev, 0, sizeof *dev, st);
        if (err == hipSuccess) {
                hipLaunchKernelGGL(selftest_div14_kernel, dim3((0x3f800000u >> 8) + 1), dim3(256), 0, st, dev);
                err = hipGetLastError();
        }
        if (err == hipSuccess) err = hipMemcpyAsync(mismatches, dev, sizeof *dev, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        (void) hipFree(dev);
        if (err != hipSuccess) {
                ug::set_last_error(err, "ug_hip_selftest_dxt_encode");
                return UG_HIP_ERUNTIME;
        }
        return UG_HIP_SUCCESS;
}
