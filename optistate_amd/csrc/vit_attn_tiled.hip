// vit_attn_tiled.hip -- key-tiled exact-fp32 attention of the ViT auto-encoder for the shapes that the whole-head kernels cannot
// hold: head dimension 64, and any token count.  Forward with softmax statistics, and the backward as two kernels.  All products
// run on v_mfma_f32_32x32x2_f32 with fp32 operands; no atomics: every sum has one owner and a fixed order, the same inputs
// give the same bits.
//
// Common plan.  A workgroup is four waves (256 threads) and serves one (image, head) and one BLOCK of four 32-row tiles of the
// side it owns; wave w owns tile 4 blockIdx.y + w of that side for the whole kernel and keeps its operands and accumulators in
// registers.  The 32-row tiles of the OTHER side are walked in ascending order; they pass through LDS, shared by the four
// waves: two matrices [32][HD + 1] floats (pitch HD + 1: a fragment read `row li, column 2q + lh` puts the 32 rows of a wave
// half on 32 different banks, and `row a, column li` is contiguous), double buffered.  The next tile is loaded from global memory
// with 16-byte loads into registers BEFORE the products of the current one and written to the other buffer behind them: one
// barrier per walked tile.  Rows past L are staged as zeros.
//   LDS bytes:  forward / dQ   2 buffers x (K + V) x 32 x (HD + 1) x 4        = 16,896 (HD 32)   33,280 (HD 64)
//               dK dV          2 buffers x (Q + dO) x 32 x (HD + 1) x 4 + 512 = 17,408 (HD 32)   33,792 (HD 64)
//                              (512: log-sum-exp and delta of the staged queries, 2 buffers x 2 x 32 floats)
//   Registers per lane (HD 32 / 64), at two workgroups per CU (256 available):
//               forward        Q fragments 16 / 32, S 16, O^T accumulators 16 / 32, staging 8 / 16
//               dQ             Q and dO fragments 32 / 64, S and dP 32, dQ^T accumulators 16 / 32, staging 8 / 16
//               dK dV          K and V fragments 32 / 64, S and dP 32, dK^T and dV^T accumulators 32 / 64, staging 10 / 18
//
// Fragment conventions (as in vit_kernels.hip): lane = (li, lh) = (lane & 31, lane >> 5); mfma(a, b, C) adds A[row li][k lh] *
// B[k lh][column li]; in C a lane owns column li and register e is row a_e + 4 lh with a_e = (e & 3) + 8 (e >> 2).
//
// attention_tiled_fwd_kernel: the wave owns 32 QUERIES.  Per key tile: S^T = K Q^T (A = K rows from LDS, B = the wave's Q
//   fragments, pre-scaled by log2(e) / sqrt(HD)): a lane owns ONE query and its 16 registers run over keys.  Online softmax in
//   the lane: tile maximum (in-lane, one exchange between the wave halves), m' = max(m, tile), the O^T accumulators and the
//   running sum are scaled by exp2(m - m'), P^T = exp2(S^T - m') stays in the registers and is the B operand of O^T += V^T P^T
//   (k-pair e = keys a_e, a_e + 4 of the tile, the V^T fragments fetched in that order).  Keys past L are set to -3e38 before the
//   maximum: their weight is exp2(-3e38 - m') = 0 exactly.  Output O = O^T / sum and, if asked for, lse2 = m + log2(sum) per
//   (image, head, query): the log-sum-exp of the scaled logits in units of log 2, the form the backward's exp2 takes directly.
// attention_tiled_dq_kernel: the wave owns 32 queries again; per key tile S^T = K Q^T and dP^T = V dO^T in the same layout,
//   P^T = exp2(S^T - lse2), dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T from the registers.  delta = rowsum(dO o O) of the
//   wave's queries is formed here (each wave half holds half of the head's columns, one exchange) and written out for the
//   other kernel.
// attention_tiled_dkv_kernel: the wave owns 32 KEYS (K and V fragments in registers) and walks the query tiles (Q, dO, lse2,
//   delta through LDS).  S = Q K^T and dP = dO V^T with the query rows as A: a lane owns one key, its registers run over
//   queries.  P and dS are rebuilt as above (a padded query has Q = dO = 0, lse2 = delta = 0: P = 1, and everything it adds is
//   P . 0 = 0 or dS = 1 . (0 - 0) = 0), dV^T += dO^T P and dK^T += Q^T dS take them from the registers; the accumulators live
//   across the query loop and are stored once.
// dQ by recomputation (S and dP are formed in both backward kernels: seven tile products per (query tile, key tile) pair at head
// dimension 32 instead of five) rather than per-key-block partial dQ tiles: DESIGN.md section 4.8.1.
#include "vit_host.hpp"

#include <math.h>

namespace osv {

typedef float f32x16a __attribute__((ext_vector_type(16)));
constexpr int AT_NW = 4;                                      // waves per workgroup = tiles of the owned side per block

// lanes 32-63 of a <-> lanes 0-31 of b, as halves_swap32 of vit_kernels.hip (a = b = v on entry: afterwards a holds the low
// half's value in both halves, b the high half's)
__device__ __forceinline__ void at_halves_swap(float &a, float &b)
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}

// one 32-row tile of two row-major matrices on its way from global memory to LDS: 256 threads, HD / 4 16-byte pieces per row
template <int HD>
struct TileRegs { float4 a[HD / 32], b[HD / 32]; };

template <int HD>
__device__ __forceinline__ void at_load(TileRegs<HD> &t, const float *A, size_t lda, const float *B, size_t ldb, int row0, int L)
{
#pragma unroll
    for (int i = 0; i < HD / 32; i++) {
        const int p = threadIdx.x + 256 * i, r = row0 + p / (HD / 4), c4 = (p % (HD / 4)) * 4;
        t.a[i] = t.b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < L) {
            t.a[i] = *reinterpret_cast<const float4 *>(A + (size_t)r * lda + c4);
            t.b[i] = *reinterpret_cast<const float4 *>(B + (size_t)r * ldb + c4);
        }
    }
}

template <int HD>
__device__ __forceinline__ void at_store(const TileRegs<HD> &t, float *As, float *Bs)
{
#pragma unroll
    for (int i = 0; i < HD / 32; i++) {
        const int p = threadIdx.x + 256 * i, o = (p / (HD / 4)) * (HD + 1) + (p % (HD / 4)) * 4;
        As[o] = t.a[i].x; As[o + 1] = t.a[i].y; As[o + 2] = t.a[i].z; As[o + 3] = t.a[i].w;
        Bs[o] = t.b[i].x; Bs[o + 1] = t.b[i].y; Bs[o + 2] = t.b[i].z; Bs[o + 3] = t.b[i].w;
    }
}

template <int HD>
__global__ __launch_bounds__(256, 2) void attention_tiled_fwd_kernel(int L, int D, int heads, const float *QKV, float *O, float *LSE)
{
    constexpr int P = HD + 1, TILE = 32 * P, NJ = HD / 32;
    __shared__ __attribute__((aligned(16))) float sm[2][2][TILE];          // [buffer][K | V]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads, NT = (L + 31) / 32;
    const float *base = QKV + (size_t)n * L * 3 * D + h * HD;
    const int r0 = 32 * ((int)blockIdx.y * AT_NW + wave);
    const bool act = r0 < L;                                               // wave-uniform; an idle wave stages and keeps the barriers
    const float sl2 = rsqrtf((float)HD) * 1.44269504088896341f;
    float qa[HD / 2];
    {
        const int qrow = r0 + li < L ? r0 + li : L - 1;
#pragma unroll
        for (int q = 0; q < HD / 2; q++) qa[q] = base[(size_t)qrow * 3 * D + 2 * q + lh] * sl2;
    }
    f32x16a acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
    float m = -3.0e38f, den = 0.f;                                         // den: this wave half's share of the running sum
    TileRegs<HD> t;
    at_load<HD>(t, base + D, (size_t)3 * D, base + 2 * D, (size_t)3 * D, 0, L);
    at_store<HD>(t, sm[0][0], sm[0][1]);
    __syncthreads();
    for (int jt = 0; jt < NT; jt++) {
        if (jt + 1 < NT) at_load<HD>(t, base + D, (size_t)3 * D, base + 2 * D, (size_t)3 * D, 32 * (jt + 1), L);
        if (act) {
            const float *Kb = sm[jt & 1][0], *Vb = sm[jt & 1][1];
            f32x16a S;
#pragma unroll
            for (int e = 0; e < 16; e++) S[e] = 0.f;
#pragma unroll
            for (int q = 0; q < HD / 2; q++) S = __builtin_amdgcn_mfma_f32_32x32x2f32(Kb[li * P + 2 * q + lh], qa[q], S, 0, 0, 0);
            if (32 * jt + 32 > L) {                                        // the ragged tile: register index = key
#pragma unroll
                for (int e = 0; e < 16; e++)
                    if (32 * jt + (e & 3) + 8 * (e >> 2) + 4 * lh >= L) S[e] = -3.0e38f;
            }
            float mt = S[0];
#pragma unroll
            for (int e = 1; e < 16; e++) mt = fmaxf(mt, S[e]);
            {
                float ma = mt, mb = mt;
                at_halves_swap(ma, mb);
                mt = fmaxf(ma, mb);
            }
            const float mn = fmaxf(m, mt), corr = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 16; e++) { S[e] = __builtin_amdgcn_exp2f(S[e] - mn); ps += S[e]; }
            den = den * corr + ps;
#pragma unroll
            for (int j = 0; j < NJ; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[j][e] *= corr;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int key = (e & 3) + 8 * (e >> 2) + 4 * lh;
#pragma unroll
                for (int j = 0; j < NJ; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vb[key * P + 32 * j + li], S[e], acc[j], 0, 0, 0);
            }
        }
        if (jt + 1 < NT) at_store<HD>(t, sm[(jt + 1) & 1][0], sm[(jt + 1) & 1][1]);     // last read before the previous barrier
        __syncthreads();
    }
    if (!act) return;
    {
        float da = den, db = den;
        at_halves_swap(da, db);
        den = da + db;
    }
    if (r0 + li < L) {
        // lane = query r0 + li, registers = head columns a_e + 4 lh (+ 32 j): four 16-byte stores per accumulator
        const float inv = 1.0f / den;
        float *op = O + ((size_t)n * L + r0 + li) * D + h * HD + 4 * lh;
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                *reinterpret_cast<float4 *>(op + 32 * j + 8 * g) =
                    make_float4(acc[j][4 * g] * inv, acc[j][4 * g + 1] * inv, acc[j][4 * g + 2] * inv, acc[j][4 * g + 3] * inv);
        if (LSE && lh == 0) LSE[((size_t)n * heads + h) * L + r0 + li] = m + log2f(den);
    }
}

template <int HD>
__global__ __launch_bounds__(256, 2) void attention_tiled_dq_kernel(int L, int D, int heads, const float *QKV, const float *O, const float *dO,
                                                                    const float *LSE, float *delta, float *dQKV)
{
    constexpr int P = HD + 1, TILE = 32 * P, NJ = HD / 32;
    __shared__ __attribute__((aligned(16))) float sm[2][2][TILE];          // [buffer][K | V]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads, NT = (L + 31) / 32;
    const float *base = QKV + (size_t)n * L * 3 * D + h * HD;
    const int r0 = 32 * ((int)blockIdx.y * AT_NW + wave);
    const bool act = r0 < L;
    const float scale = rsqrtf((float)HD), sl2 = scale * 1.44269504088896341f;
    const int qrow = r0 + li < L ? r0 + li : L - 1;
    float qa[HD / 2], ga[HD / 2], dl = 0.f;
    {
        const float *gp = dO + ((size_t)n * L + qrow) * D + h * HD, *op = O + ((size_t)n * L + qrow) * D + h * HD;
#pragma unroll
        for (int q = 0; q < HD / 2; q++) {
            qa[q] = base[(size_t)qrow * 3 * D + 2 * q + lh] * sl2;
            ga[q] = gp[2 * q + lh];
            dl += ga[q] * op[2 * q + lh];
        }
        float da = dl, db = dl;
        at_halves_swap(da, db);
        dl = da + db;
    }
    const float lse = LSE[((size_t)n * heads + h) * L + qrow];
    if (act && lh == 0 && r0 + li < L) delta[((size_t)n * heads + h) * L + r0 + li] = dl;
    f32x16a acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
    TileRegs<HD> t;
    at_load<HD>(t, base + D, (size_t)3 * D, base + 2 * D, (size_t)3 * D, 0, L);
    at_store<HD>(t, sm[0][0], sm[0][1]);
    __syncthreads();
    for (int jt = 0; jt < NT; jt++) {
        if (jt + 1 < NT) at_load<HD>(t, base + D, (size_t)3 * D, base + 2 * D, (size_t)3 * D, 32 * (jt + 1), L);
        if (act) {
            const float *Kb = sm[jt & 1][0], *Vb = sm[jt & 1][1];
            f32x16a S, dP;
#pragma unroll
            for (int e = 0; e < 16; e++) { S[e] = 0.f; dP[e] = 0.f; }
#pragma unroll
            for (int q = 0; q < HD / 2; q++) {
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(Kb[li * P + 2 * q + lh], qa[q], S, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(Vb[li * P + 2 * q + lh], ga[q], dP, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int key = (e & 3) + 8 * (e >> 2) + 4 * lh;
                const float p = 32 * jt + key < L ? __builtin_amdgcn_exp2f(S[e] - lse) : 0.f;
                const float ds = p * (dP[e] - dl);                         // dS^T (of the scaled scores)
#pragma unroll
                for (int j = 0; j < NJ; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kb[key * P + 32 * j + li], ds, acc[j], 0, 0, 0);
            }
        }
        if (jt + 1 < NT) at_store<HD>(t, sm[(jt + 1) & 1][0], sm[(jt + 1) & 1][1]);
        __syncthreads();
    }
    if (act && r0 + li < L) {
        float *qp = dQKV + ((size_t)n * L + r0 + li) * 3 * D + h * HD + 4 * lh;
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                *reinterpret_cast<float4 *>(qp + 32 * j + 8 * g) =
                    make_float4(acc[j][4 * g] * scale, acc[j][4 * g + 1] * scale, acc[j][4 * g + 2] * scale, acc[j][4 * g + 3] * scale);
    }
}

template <int HD>
__global__ __launch_bounds__(256, 2) void attention_tiled_dkv_kernel(int L, int D, int heads, const float *QKV, const float *dO, const float *LSE,
                                                                     const float *delta, float *dQKV)
{
    constexpr int P = HD + 1, TILE = 32 * P, NJ = HD / 32;
    __shared__ __attribute__((aligned(16))) float sm[2][2][TILE];          // [buffer][Q | dO]
    __shared__ float st[2][2][32];                                         // [buffer][lse2 | delta] of the staged queries
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads, NT = (L + 31) / 32;
    const float *base = QKV + (size_t)n * L * 3 * D + h * HD;
    const float *gbase = dO + (size_t)n * L * D + h * HD;
    const float *stat = (threadIdx.x < 32 ? LSE : delta) + ((size_t)n * heads + h) * L;      // threads 0-31: lse2, 32-63: delta
    const int key0 = 32 * ((int)blockIdx.y * AT_NW + wave);
    const bool act = key0 < L, masked = key0 + li >= L;                    // masked: this lane's key is padding
    const float scale = rsqrtf((float)HD), sl2 = scale * 1.44269504088896341f;
    float kf[HD / 2], vf[HD / 2];
    {
        const int krow = key0 + li < L ? key0 + li : L - 1;
#pragma unroll
        for (int q = 0; q < HD / 2; q++) {
            kf[q] = base[(size_t)krow * 3 * D + D + 2 * q + lh];
            vf[q] = base[(size_t)krow * 3 * D + 2 * D + 2 * q + lh];
        }
    }
    f32x16a accK[NJ], accV[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) { accK[j][e] = 0.f; accV[j][e] = 0.f; }
    TileRegs<HD> t;
    float sv = 0.f;
    at_load<HD>(t, base, (size_t)3 * D, gbase, (size_t)D, 0, L);
    if (threadIdx.x < 64) sv = (int)(threadIdx.x & 31) < L ? stat[threadIdx.x & 31] : 0.f;
    at_store<HD>(t, sm[0][0], sm[0][1]);
    if (threadIdx.x < 64) st[0][threadIdx.x >> 5][threadIdx.x & 31] = sv;
    __syncthreads();
    for (int qt = 0; qt < NT; qt++) {
        if (qt + 1 < NT) {
            at_load<HD>(t, base, (size_t)3 * D, gbase, (size_t)D, 32 * (qt + 1), L);
            if (threadIdx.x < 64) { const int r = 32 * (qt + 1) + (threadIdx.x & 31); sv = r < L ? stat[r] : 0.f; }
        }
        if (act) {
            const float *Qb = sm[qt & 1][0], *Gb = sm[qt & 1][1], *lb = st[qt & 1][0], *db = st[qt & 1][1];
            f32x16a S, dP;
#pragma unroll
            for (int e = 0; e < 16; e++) { S[e] = 0.f; dP[e] = 0.f; }
#pragma unroll
            for (int q = 0; q < HD / 2; q++) {
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(Qb[li * P + 2 * q + lh], kf[q], S, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(Gb[li * P + 2 * q + lh], vf[q], dP, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int qr = (e & 3) + 8 * (e >> 2) + 4 * lh;
                const float p = masked ? 0.f : __builtin_amdgcn_exp2f(S[e] * sl2 - lb[qr]);
                const float ds = p * (dP[e] - db[qr]);                     // dS (of the scaled scores)
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    accV[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gb[qr * P + 32 * j + li], p, accV[j], 0, 0, 0);
                    accK[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qb[qr * P + 32 * j + li], ds, accK[j], 0, 0, 0);
                }
            }
        }
        if (qt + 1 < NT) {
            at_store<HD>(t, sm[(qt + 1) & 1][0], sm[(qt + 1) & 1][1]);
            if (threadIdx.x < 64) st[(qt + 1) & 1][threadIdx.x >> 5][threadIdx.x & 31] = sv;
        }
        __syncthreads();
    }
    if (act && !masked) {
        // lane = key, registers = head columns a_e + 4 lh (+ 32 j)
        float *kp = dQKV + ((size_t)n * L + key0 + li) * 3 * D + D + h * HD + 4 * lh, *vp = kp + D;
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                *reinterpret_cast<float4 *>(kp + 32 * j + 8 * g) =
                    make_float4(accK[j][4 * g] * scale, accK[j][4 * g + 1] * scale, accK[j][4 * g + 2] * scale, accK[j][4 * g + 3] * scale);
                *reinterpret_cast<float4 *>(vp + 32 * j + 8 * g) = make_float4(accV[j][4 * g], accV[j][4 * g + 1], accV[j][4 * g + 2], accV[j][4 * g + 3]);
            }
    }
}

}  // namespace osv

using namespace osv;

int os_vit_launch_attention_tiled(os_ctx *ctx, const VitDims &d, int N, const float *QKV, float *O, float *lse, hipStream_t s, const char *name)
{
    const int L = ntok(d), hd = d.dim / d.heads;
    if (hd != 32 && hd != 64) return os_fail(ctx, -4, "os_vit: the tiled attention kernels need a head dimension of 32 or 64");
    const dim3 grid((unsigned)(N * d.heads), (unsigned)(((L + 31) / 32 + AT_NW - 1) / AT_NW));
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_ATTN, s, name);
    if (hd == 32) hipLaunchKernelGGL(attention_tiled_fwd_kernel<32>, grid, dim3(256), 0, s, L, d.dim, d.heads, QKV, O, lse);
    else hipLaunchKernelGGL(attention_tiled_fwd_kernel<64>, grid, dim3(256), 0, s, L, d.dim, d.heads, QKV, O, lse);
    os_prof_end(ctx, slot, s);
    return 0;
}

int os_vit_launch_attention_tiled_bwd(os_ctx *ctx, const VitDims &d, int N, const float *QKV, const float *O, const float *dO, const float *lse,
                                      float *delta, float *dQKV, hipStream_t s)
{
    const int L = ntok(d), hd = d.dim / d.heads;
    if (hd != 32 && hd != 64) return os_fail(ctx, -4, "os_vit: the tiled attention kernels need a head dimension of 32 or 64");
    const dim3 grid((unsigned)(N * d.heads), (unsigned)(((L + 31) / 32 + AT_NW - 1) / AT_NW));
    int slot = os_prof_begin(ctx, OS_PHASE_VIT_ATTN, s, "attention_tiled_dq_kernel");
    if (hd == 32) hipLaunchKernelGGL(attention_tiled_dq_kernel<32>, grid, dim3(256), 0, s, L, d.dim, d.heads, QKV, O, dO, lse, delta, dQKV);
    else hipLaunchKernelGGL(attention_tiled_dq_kernel<64>, grid, dim3(256), 0, s, L, d.dim, d.heads, QKV, O, dO, lse, delta, dQKV);
    os_prof_end(ctx, slot, s);
    slot = os_prof_begin(ctx, OS_PHASE_VIT_ATTN, s, "attention_tiled_dkv_kernel");
    if (hd == 32) hipLaunchKernelGGL(attention_tiled_dkv_kernel<32>, grid, dim3(256), 0, s, L, d.dim, d.heads, QKV, dO, lse, delta, dQKV);
    else hipLaunchKernelGGL(attention_tiled_dkv_kernel<64>, grid, dim3(256), 0, s, L, d.dim, d.heads, QKV, dO, lse, delta, dQKV);
    os_prof_end(ctx, slot, s);
    return 0;
}
