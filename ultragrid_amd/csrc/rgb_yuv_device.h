// rgb_yuv_device.h -- the reference's 8-bit Q14 conversions between R,G,B and BT.709 limited-range Y,Cb,Cr on one pixel or one 4:2:2 pair, shared by
// pixfmt.hip (whole-frame converters) and compose.hip (the logo overlay decodes, blends and encodes in one kernel).
#pragma once

#include <stdint.h>

namespace ug {

// Q14 coefficients, BT.709 limited range (the default, color_space.c:149-191).  Values are the
// compile-time table of the reference, reproduced by oracle/pixfmt_oracle.c:oracle_color_coeffs
// and pinned against get_color_coeffs() in tests/test_oracle_pixfmt.py.
struct Cfs {
        int y_r, y_g, y_b, cb_r, cb_g, cb_b, cr_r, cr_g, cr_b, y_scale, r_cr, g_cb, g_cr, b_cb;
};
#define UG_CFS8_INIT { 2992, 10063, 1016, -1649, -5547, 7196, 7195, -6536, -659, 19077, 29371, -3494, -8733, 34610 }
constexpr int kBase = 14; // COMP_BASE, color_space.h:70-71

// one iteration of vc_copylineToUYVY (pixfmt_conv.c:1008-1053): two pixels -> the word U Y0 V Y1
__host__ __device__ __forceinline__ uint32_t rgb_pair_to_uyvy(const Cfs &c, int r0, int g0, int b0, int r1, int g1, int b1)
{
        const int y1 = ((r0 * c.y_r + g0 * c.y_g + b0 * c.y_b) >> kBase) + 16;
        int u = r0 * c.cb_r + g0 * c.cb_g + b0 * c.cb_b;
        int v = r0 * c.cr_r + g0 * c.cr_g + b0 * c.cr_b;
        const int y2 = ((r1 * c.y_r + g1 * c.y_g + b1 * c.y_b) >> kBase) + 16;
        u += r1 * c.cb_r + g1 * c.cb_g + b1 * c.cb_b;
        v += r1 * c.cr_r + g1 * c.cr_g + b1 * c.cr_b;
        u = ((u / 2) >> kBase) + 128; // C '/' truncates toward zero, '>>' floors
        v = ((v / 2) >> kBase) + 128;
        return ((uint32_t) (y2 & 0xFF) << 24) | ((v & 0xFF) << 16) | ((y1 & 0xFF) << 8) | (u & 0xFF);
}

#ifdef __HIPCC__
__device__ constexpr Cfs kCfs8  = UG_CFS8_INIT;
__device__ constexpr Cfs kCfs10 = { 2983, 10034, 1013, -1644, -5531, 7175, 7174, -6517, -657, 19133, 29457, -3504, -8758, 34712 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// hipcc (ROCm 7.2) fuses "clamp(x >> 14, 0, 255) | clamp(y >> 14, 0, 255) << 8" into gfx950's
// v_ashr_pk_u8_i32 and then ORs further bytes into the result assuming its upper 16 bits are zero;
// on MI355X the instruction leaves the destination's upper half unchanged, so stale bytes leak into
// the packed word (caught by tests/test_gpu_pixfmt.py).  Making the clamped value opaque keeps the
// clamp (v_med3_i32) and the byte packing as separate, correct instructions at zero run-time cost.
__device__ __forceinline__ int opaque(int v)
{
        asm volatile("" : "+v"(v));
        return v;
}
__device__ __forceinline__ void yuv_to_rgb8(int y, int u, int v, uint8_t *o)
{
        // copylineYUVtoRGB, pixfmt_conv.c:1065-1094: clamp [0,255]
        o[0] = opaque(clampi((y + v * kCfs8.r_cr) >> kBase, 0, 255));
        o[1] = opaque(clampi((y + u * kCfs8.g_cb + v * kCfs8.g_cr) >> kBase, 0, 255));
        o[2] = opaque(clampi((y + u * kCfs8.b_cb) >> kBase, 0, 255));
}
#endif

} // namespace ug
