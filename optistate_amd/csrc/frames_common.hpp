// frames_common.hpp -- what the frame kernels (frames_kernels.hip: ingest, frames_augment.hip: augmentation) share: Pillow's
// coefficient arithmetic for one output index of a resampled axis, the multiply-high index split and the bounded 16-byte load.
#pragma once
#include "launch.hpp"

#include <math.h>

namespace osfr {

constexpr int PB = 22;            // Pillow's PRECISION_BITS = 32 - 8 - 2

// idx / d for a d fixed per launch: m = magic_of(d), exact while idx * d < 2^32
__device__ __forceinline__ uint32_t div_magic(uint32_t idx, int d, uint32_t m) { return d == 1 ? idx : __umulhi(idx, m); }
static inline uint32_t magic_of(int d) { return d <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d); }

// 16 bytes at p (16-byte aligned); bytes outside [lo, hi) are not read and come back as zero
__device__ __forceinline__ uint4 load16(const uint8_t *p, const uint8_t *lo, const uint8_t *hi)
{
    const uintptr_t a = (uintptr_t)p, l = (uintptr_t)lo, h = (uintptr_t)hi;
    if (a >= l && a + 16 <= h) return *(const uint4 *)p;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; b++)
        if (a + b >= l && a + b < h) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// triangle weight of source index xmin + x for an output index centred at `center`
__host__ __device__ inline double axis_weight(int x, int xmin, double center, double ss)
{
#pragma clang fp contract(off)
    double v = (x + xmin - center + 0.5) * ss;
    if (v < 0.0) v = -v;
    return v < 1.0 ? 1.0 - v : 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter and ONE output index xx of an axis in -> S, operation
// for operation, in IEEE double without contraction (the bits of these coefficients are the bits of the result): first source
// index, tap count, and the taps in PB-bit fixed point at coef[0], coef[stride], ...  An axis that already has the output length
// passes through: one tap of 2^PB at xx, out = (2^21 + 2^22 p) >> 22 = p.  Up to 2 ceil(max(in / S, 1)) + 1 taps (3 when in <= S).
// The host builds the ingest's tables with it, a workgroup of the augmentation kernel the two tables of its image's crop.
__host__ __device__ inline void axis_entry(int in, int S, int xx, int &lo, int &cnt, int32_t *coef, int stride)
{
#pragma clang fp contract(off)
    if (in == S) { lo = xx; cnt = 1; coef[0] = 1 << PB; return; }
    const double scale = (double)in / (double)S;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    const double ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; x++) ww += axis_weight(x, xmin, center, ss);
    for (int x = 0; x < n; x++) {
        const double w = axis_weight(x, xmin, center, ss);
        const double k = ww != 0.0 ? w / ww : w;
        coef[x * stride] = (int)(0.5 + k * (double)(1 << PB));
    }
    lo = xmin; cnt = n;
}

}  // namespace osfr
