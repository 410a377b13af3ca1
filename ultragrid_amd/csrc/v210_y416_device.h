// v210_y416_device.h -- one v210 group (4 words = 6 pixels) <-> six Y416 pixels (U Y V A, 16 bits each), the arithmetic of
// vc_copylineV210toY416 (pixfmt_conv.c:2834-2882) and vc_copylineY416toV210 (:3004-3031).  Shared by the converters of pixfmt_ext.hip
// and by matrix2's fused v210 path (pixel_filter.hip).
#pragma once

#include <stdint.h>

namespace ug {

// the 10-bit samples of a group, in place (not yet shifted to 16 bits)
__device__ __forceinline__ void v210_unpack(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&Y)[6], uint32_t (&U)[3], uint32_t (&V)[3])
{
        Y[0] = (w0 >> 10) & 0x3ff, Y[1] = w1 & 0x3ff, Y[2] = (w1 >> 20) & 0x3ff, Y[3] = (w2 >> 10) & 0x3ff, Y[4] = w3 & 0x3ff, Y[5] = (w3 >> 20) & 0x3ff;
        U[0] = w0 & 0x3ff, U[1] = (w1 >> 10) & 0x3ff, U[2] = (w2 >> 20) & 0x3ff;
        V[0] = (w0 >> 20) & 0x3ff, V[1] = w2 & 0x3ff, V[2] = (w3 >> 10) & 0x3ff;
}

// six Y416 pixels s[4 * i + {0, 1, 2}] = U, Y, V (alpha unused) -> the group's four words: chroma of a pair averaged, then the top 10 bits
__device__ __forceinline__ void y416_pack_v210(const uint16_t (&s)[24], uint32_t (&d)[4])
{
        uint32_t u[3], v[3], Y[6];
#pragma unroll
        for (int i = 0; i < 3; i++) {
                u[i] = (uint16_t) ((s[8 * i] + s[8 * i + 4]) / 2), v[i] = (uint16_t) ((s[8 * i + 2] + s[8 * i + 6]) / 2);
                Y[2 * i] = s[8 * i + 1], Y[2 * i + 1] = s[8 * i + 5];
        }
        d[0] = u[0] >> 6U | Y[0] >> 6U << 10U | v[0] >> 6U << 20U;
        d[1] = Y[1] >> 6U | u[1] >> 6U << 10U | Y[2] >> 6U << 20U;
        d[2] = v[1] >> 6U | Y[3] >> 6U << 10U | u[2] >> 6U << 20U;
        d[3] = Y[4] >> 6U | v[2] >> 6U << 10U | Y[5] >> 6U << 20U;
}

} // namespace ug
