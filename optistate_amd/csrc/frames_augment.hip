// frames_augment.hip -- the random augmentations of the auto-encoder's training transform between Grayscale and ToTensor
// (transformer/autoencoder_training.py:45-52): RandomRotation -> RandomVerticalFlip -> RandomHorizontalFlip -> RandomPerspective ->
// RandomApply([RandomResizedCrop]) -> ToTensor on an S x S uint8 gray image (what os_frames_ingest_u8 writes), bit for bit as Pillow
// computes them with nearest-neighbour rotation and perspective, a bilinear crop-resize and fill 0.  The parameters are explicit:
// one record of 20 doubles per image (layout in include/optistate_hip.h), drawn on the host (optistate_amd/augment.py).
//
// The image is defined from output to input.  out = resize(Q[top : top + h, left : left + w]) with the crop flag, else Q;
// Q[y][x] = F[ys][xs] with (xs, ys) the perspective map of (x, y) in float64; F[y][x] = V[y][S - 1 - x]; V[y][x] = R[S - 1 - y][x];
// R[y][x] = G[yi][xi] with (xi, yi) the rotation in Pillow's 16.16 fixed point.  The three nearest-neighbour stages are index maps,
// nothing is rounded between them: they compose into ONE gather from G per pixel of Q and no intermediate image exists.  A +-10
// degree rotation under a distortion-0.5 perspective reaches anywhere in G, so G is not tiled: the whole image is staged in LDS.
//
// frames_augment_kernel: one workgroup of 1,024 threads = one image.
//   stage    G goes from global memory into LDS plane 0 by 16-byte loads (S a multiple of 16 and a 16-byte aligned image: every piece
//            lies inside one row; otherwise pieces at the address aligned down, bounded by the caller's buffer, scattered by byte).
//   no crop  (the flag is uniform over the workgroup) thread = output pixel, consecutive lanes = consecutive pixels of a row: the
//            composed gather reads one byte of plane 0, the division and the coalesced float store follow.  One read of G, one write.
//   crop     the gather fills plane 1 with the crop Q[top : top + h, left : left + w] only; meanwhile 2 S threads build the two
//            coefficient tables of THIS image's crop in LDS with axis_entry (frames_common.hpp: Pillow's precompute_coeffs in double
//            on the device; in <= S, so at most three taps): [lo | cnt | 3 taps][S] per axis, tap-major.  Horizontal pass plane 1 ->
//            plane 0 (G is dead by then), the h rows of the crop only, rounded to uint8; vertical pass plane 0 -> division -> store.
// LDS: both planes have a pitch of P = 16 ceil(S / 16) + 4 bytes, an odd number of dwords.  The gather's reads are irregular: with
// an odd dword pitch a wave whose 64 source pixels run along a rotated line changes bank with every row it crosses (a pitch of 64
// dwords would keep a steep line in one bank).  Both passes run lane = column: the horizontal pass reads up to 3 consecutive bytes at
// lo(x), which grows by 0 or 1 per column, the vertical pass reads its taps P bytes apart down a column -- in either a wave's 64
// lanes read a run of at most 64 consecutive bytes of one row per tap, 16 dwords in 16 different banks, four lanes per dword (a
// broadcast); a wave that straddles two rows (S not a multiple of 64) reads two such runs, which can meet in a bank (2-way).
// 2 S P + 40 S bytes: 111,104 at S = 224, 143,360 at the limit S = 256.
#include "frames_common.hpp"

#include <stdlib.h>

namespace osfr {

constexpr int ANT = 1024;
constexpr int AUG_SMAX = 256;          // two planes of S (16 ceil(S / 16) + 4) bytes and the tables within 160 KB of LDS
constexpr int AUG_REC = 20;            // doubles per record
constexpr int AUG_ROTATE = 1, AUG_VFLIP = 2, AUG_HFLIP = 4, AUG_PERSPECTIVE = 8, AUG_CROP = 16;

struct AugmentArgs {
    const uint8_t *gray;               // [N][S][S]
    const double *params;              // [N][20]
    float *out;                        // [N][S][S]
    size_t total_bytes;                // N S S
    int S, P;
    uint32_t s_magic;                  // idx / S for idx < 2^16
    int lds_q, lds_tab;                // byte offsets of plane 1 and of the tables
};

struct AugmentMap {
    int flags;
    uint32_t A[6];                     // rotation in 16.16 fixed point; the arithmetic wraps like Pillow's int
    double c[8];                       // perspective
};

// Pillow's FIX: floor(v 65536 + 0.5) as an int
__device__ __forceinline__ uint32_t fix16(double v)
{
#pragma clang fp contract(off)
    return (uint32_t)(int)floor(v * 65536.0 + 0.5);
}

// Q[y][x] (before the crop) as one read of G: perspective, horizontal flip, vertical flip, rotation, each only with its flag
__device__ __forceinline__ uint32_t gather(const uint8_t *g, int P, int S, const AugmentMap &m, int x, int y)
{
#pragma clang fp contract(off)
    if (m.flags & AUG_PERSPECTIVE) {
        const double xin = x + 0.5, yin = y + 0.5;
        const double den = m.c[6] * xin + m.c[7] * yin + 1.0;
        const double xs = (m.c[0] * xin + m.c[1] * yin + m.c[2]) / den;
        const double ys = (m.c[3] * xin + m.c[4] * yin + m.c[5]) / den;
        // Pillow: a coordinate < 0 becomes -1, anything else truncates; outside [0, S) is the fill (a NaN is outside as well)
        if (!(xs >= 0.0 && xs < (double)S && ys >= 0.0 && ys < (double)S)) return 0u;
        x = (int)xs; y = (int)ys;
    }
    if (m.flags & AUG_HFLIP) x = S - 1 - x;
    if (m.flags & AUG_VFLIP) y = S - 1 - y;
    if (m.flags & AUG_ROTATE) {
        const int xi = (int)(m.A[2] + (uint32_t)y * m.A[1] + (uint32_t)x * m.A[0]) >> 16;
        const int yi = (int)(m.A[5] + (uint32_t)y * m.A[4] + (uint32_t)x * m.A[3]) >> 16;
        if ((uint32_t)xi >= (uint32_t)S || (uint32_t)yi >= (uint32_t)S) return 0u;
        x = xi; y = yi;
    }
    return g[y * P + x];
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(ANT) void frames_augment_kernel(const AugmentArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    uint8_t *g = lds;                                    // plane 0 [S][P]: G, then the horizontal pass of the crop
    uint8_t *q = lds + a.lds_q;                          // plane 1 [h][P]: the crop of Q
    int32_t *tx = (int32_t *)(lds + a.lds_tab);          // [lo | cnt | tap 0 | tap 1 | tap 2][S]
    const int S = a.S, P = a.P, SS = S * S, tid = threadIdx.x;
    int32_t *ty = tx + 5 * S;
    const size_t n = blockIdx.x;
    const double *rec = a.params + n * AUG_REC;
    const uint8_t *img = a.gray + n * (size_t)SS;
    float *out = a.out + n * (size_t)SS;

    // ---- stage: G -> plane 0 ----
    const int mis = (int)((uintptr_t)img & 15);
    if (mis == 0 && (S & 15) == 0) {
        for (int k = tid; k < (SS >> 4); k += ANT) {
            const uint4 v = *(const uint4 *)(img + 16 * k);
            const int row = (int)div_magic((uint32_t)(16 * k), S, a.s_magic), col = 16 * k - row * S;
            uint32_t *d = (uint32_t *)(g + row * P + col);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        const uint8_t *buf_end = a.gray + a.total_bytes;
        for (int k = tid; k < ((mis + SS + 15) >> 4); k += ANT) {
            const uint4 v = load16(img - mis + 16 * k, a.gray, buf_end);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const int f = 16 * k - mis + b;          // byte of the image
                if (f >= 0 && f < SS) {
                    const int row = (int)div_magic((uint32_t)f, S, a.s_magic);
                    g[row * P + f - row * S] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
                }
            }
        }
    }

    AugmentMap m;
    m.flags = (int)rec[14];
    m.A[0] = fix16(rec[0]); m.A[1] = fix16(rec[1]); m.A[3] = fix16(rec[3]); m.A[4] = fix16(rec[4]);
    m.A[2] = fix16(rec[2] + rec[0] * 0.5 + rec[1] * 0.5);
    m.A[5] = fix16(rec[5] + rec[3] * 0.5 + rec[4] * 0.5);
#pragma unroll
    for (int i = 0; i < 8; i++) m.c[i] = rec[6 + i];
    __syncthreads();

    if (!(m.flags & AUG_CROP)) {
        for (int idx = tid; idx < SS; idx += ANT) {
            const int y = (int)div_magic((uint32_t)idx, S, a.s_magic), x = idx - y * S;
            out[idx] = __fdiv_rn((float)gather(g, P, S, m, x, y), 255.0f);
        }
        return;
    }

    // ---- crop: the box, clamped into the image (a record outside it is not reported) ----
    const int top = clampi((int)rec[15], 0, S - 1), left = clampi((int)rec[16], 0, S - 1);
    const int h = clampi((int)rec[17], 1, S - top), w = clampi((int)rec[18], 1, S - left);
    if (tid < S) {
        int lo, cnt;
        axis_entry(w, S, tid, lo, cnt, tx + 2 * S + tid, S);
        tx[tid] = lo; tx[S + tid] = cnt;
    } else if (tid >= AUG_SMAX && tid < AUG_SMAX + S) {
        const int yy = tid - AUG_SMAX;
        int lo, cnt;
        axis_entry(h, S, yy, lo, cnt, ty + 2 * S + yy, S);
        ty[yy] = lo; ty[S + yy] = cnt;
    }
    for (int idx = tid; idx < h * S; idx += ANT) {
        const int r = (int)div_magic((uint32_t)idx, S, a.s_magic), x = idx - r * S;
        if (x < w) q[r * P + x] = (uint8_t)gather(g, P, S, m, left + x, top + r);
    }
    __syncthreads();
    // ---- horizontal pass: plane 1 -> plane 0, rows of the crop ----
    for (int idx = tid; idx < h * S; idx += ANT) {
        const int r = (int)div_magic((uint32_t)idx, S, a.s_magic), x = idx - r * S;
        const int cnt = tx[S + x];
        const uint8_t *p = q + r * P + tx[x];
        uint32_t acc = 1u << (PB - 1);
        for (int t = 0; t < cnt; t++) acc = __umul24((uint32_t)tx[(2 + t) * S + x], (uint32_t)p[t]) + acc;
        g[r * P + x] = (uint8_t)min(acc >> PB, 255u);
    }
    __syncthreads();
    // ---- vertical pass, division ----
    for (int idx = tid; idx < SS; idx += ANT) {
        const int y = (int)div_magic((uint32_t)idx, S, a.s_magic), x = idx - y * S;
        const int cnt = ty[S + y];
        const uint8_t *p = g + ty[y] * P + x;
        uint32_t acc = 1u << (PB - 1);
        for (int t = 0; t < cnt; t++) acc = __umul24((uint32_t)ty[(2 + t) * S + y], (uint32_t)p[t * P]) + acc;
        out[idx] = __fdiv_rn((float)min(acc >> PB, 255u), 255.0f);
    }
}

}  // namespace osfr

extern "C" int os_frames_augment(os_ctx *ctx, int32_t N, const uint8_t *gray, int32_t S, const double *params, float *out, void *stream)
{
    using namespace osfr;
    OS_CHECK_CTX(ctx);
    if (N < 1 || S < 1 || !gray || !params || !out)
        return os_fail(ctx, -2, "os_frames_augment: bad argument (N >= 1, S >= 1, non-null pointers)");
    if (S > AUG_SMAX) {
        snprintf(ctx->err, sizeof(ctx->err), "os_frames_augment: S = %d: the image, its crop and the crop's tables live in the LDS of one "
                 "workgroup, which holds S <= %d", S, AUG_SMAX);
        return -4;
    }
    if (((uintptr_t)params & 7) || ((uintptr_t)out & 3))
        return os_fail(ctx, -2, "os_frames_augment: params must be 8-byte aligned, out 4-byte aligned");
    OS_HIP(ctx, hipSetDevice(ctx->device));
    AugmentArgs a;
    a.gray = gray; a.params = params; a.out = out; a.total_bytes = (size_t)N * S * S;
    a.S = S; a.P = (S + 15) / 16 * 16 + 4; a.s_magic = magic_of(S);
    a.lds_q = S * a.P; a.lds_tab = 2 * S * a.P;
    const size_t lds_bytes = (size_t)a.lds_tab + (size_t)10 * S * sizeof(int32_t);
    static bool attr_set[64];          // per device of the process: more than 64 KB of dynamic LDS needs the attribute once
    if (ctx->device < 0 || ctx->device >= 64 || !attr_set[ctx->device]) {
        OS_HIP(ctx, hipFuncSetAttribute((const void *)frames_augment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        2 * AUG_SMAX * (AUG_SMAX + 4) + 10 * AUG_SMAX * (int)sizeof(int32_t)));
        if (ctx->device >= 0 && ctx->device < 64) attr_set[ctx->device] = true;
    }
    hipStream_t s = (hipStream_t)stream;
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_MISC, s, "frames_augment_kernel");
    hipLaunchKernelGGL(frames_augment_kernel, dim3((unsigned)N), dim3(ANT), lds_bytes, s, a);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}
