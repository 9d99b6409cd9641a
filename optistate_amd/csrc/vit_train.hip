// vit_train.hip -- training step of the ViT auto-encoder (transformer/autoencoder_training.py:103-114): the forward with its
// activations kept in a caller-owned workspace, and the backward pass to the flat gradient vectors of encoder and decoder.
//
// Forward: the unfused launches of the inference path (layernorm_kernel, vit_gemm_kernel, the attention kernels,
// dec_seed_kernel, dec_pred_kernel) pointed at workspace slices, so that per block its input, qkv, the attention output, the
// residual stream behind the attention, the fc1 pre-activation and its GELU survive.  LayerNorm outputs and row statistics
// are recomputed in the backward.
//
// Backward, the kernels of this file:
//   attention_bwd_kernel   one workgroup per (image, head): Q, K, V and dO of the head in LDS, wave w owns key tile w and keeps
//                          its dK^T / dV^T tiles in accumulators across the query tiles (details at the kernel): head dimension 32
//                          and at most 224 tokens; every other stack runs the key-tiled kernels of vit_attn_tiled.hip, forward
//                          (with softmax statistics kept in the workspace) and backward
//   vit_dw_kernel          dW[n][k] = sum_m dY[m][n] X[m][k] and the bias gradient from the same pass, per M-slice partials
//   reduce_parts_kernel    the partials summed in a fixed order: gradients are bit-reproducible
//   ln_bwd_kernel          LayerNorm backward + the residual add of the incoming gradient; dgamma / dbeta as per-workgroup partials
//   vit_pack_wt_kernel     W^T in B-fragment order: dX = dY . W runs on vit_gemm_kernel (EPI 7); skipped for a matrix whose
//                          resident transposed pack is current (vit_optim.hip writes those in the optimiser step)
//   gelu_bwd_kernel, loss_grad_kernel, enc_head_bwd_kernel, dec_seed_bwd_kernel, outer_sum_kernel, fill_kernel: the two ends
// All fp32, products on v_mfma_f32_32x32x2_f32; no atomics anywhere.
#include "vit_host.hpp"

#include <math.h>

namespace osv {

typedef float f32x16t __attribute__((ext_vector_type(16)));

__global__ void fill_kernel(float *p, size_t n, float v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// dst = W^T in vit_pack_w_kernel's order: W is [K][N] (the forward's [out][in] with K = out, N = in), and
// dst[(c * K/2 + q) * 64 + lane] = W[2q + (lane >> 5)][c*32 + (lane & 31)]
__global__ void vit_pack_wt_kernel(int N, int K, const float *W, float *dst)
{
    const size_t total = (size_t)N * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = i & 63;
        const size_t cq = i >> 6;
        const int q = cq % (K / 2), c = cq / (K / 2);
        dst[i] = W[(size_t)(2 * q + (lane >> 5)) * N + c * 32 + (lane & 31)];
    }
}

// out[i] = sum over s < S of part[s * stride + i], s ascending
__global__ void reduce_parts_kernel(int S, size_t n, size_t stride, const float *part, float *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < S; k++) s += part[(size_t)k * stride + i];
    out[i] = s;
}

// out[r * cols + c] = sum over n of A[n * sa + r] * B[n * sb + c], n ascending (decoder_embed.weight: N terms)
__global__ void outer_sum_kernel(int N, int rows, int cols, const float *A, size_t sa, const float *B, size_t sb, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i % cols;
    float s = 0.f;
    for (int n = 0; n < N; n++) s += A[(size_t)n * sa + r] * B[(size_t)n * sb + c];
    out[i] = s;
}

// d loss / d pred in TOKEN rows [N * L][NP] (row 0 of every image zero), read straight from the images in patch order:
// 2 (pred - target) dloss / count
__global__ void loss_grad_kernel(uint32_t M, int L, int G, int P, int NP, const float *images, const float *pred, const float *dloss,
                                 float inv_count, float *dpred)
{
    const float sc = 2.0f * dloss[0] * inv_count;
    const int W = G * P;
    const size_t total = (size_t)M * NP;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(i / NP), n = row / L, t = row % L;
        const int col = (int)(i % NP);
        float v = 0.f;
        if (t) {
            const uint32_t p = t - 1, gy = p / G, gx = p % G;
            v = sc * (pred[((size_t)n * (L - 1) + p) * NP + col] - images[((size_t)n * W + gy * P + col / P) * W + gx * P + col % P]);
        }
        dpred[i] = v;
    }
}

// dG[i] *= gelu'(H[i]) with the forward's erf (Abramowitz-Stegun 7.1.26 on the hardware exp2 / rcp): Phi(h) + h phi(h)
__global__ void gelu_bwd_kernel(size_t n, const float *H, float *dG)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = H[i], z = fabsf(v) * 0.70710678118654752f;
        const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
        const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
        const float ex = __builtin_amdgcn_exp2f(-1.44269504088896341f * z * z);           // exp(-h^2 / 2)
        dG[i] *= 0.5f * (1.0f + copysignf(fmaf(-poly, ex, 1.0f), v)) + v * ex * 0.39894228040143268f;
    }
}

__device__ __forceinline__ float wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LayerNorm backward over rows of D <= 256 (statistics recomputed as layernorm_kernel forms them): dX = dres + dLN(dY), in place
// over dres when they are the same buffer.  A workgroup owns LNB_ROWS rows, a wave every fourth of them; the waves' dgamma /
// dbeta sums meet in LDS in a fixed order and go to part[blockIdx.x][2 D].
constexpr int LNB_ROWS = 64;
__global__ __launch_bounds__(256) void ln_bwd_kernel(size_t M, int D, const float *X, const float *dY, const float *gamma, const float *dres,
                                                     float *dX, float *part)
{
    __shared__ float red[4][2][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float g[4], dg[4], db[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int c = lane + 64 * j; g[j] = c < D ? gamma[c] : 0.f; dg[j] = 0.f; db[j] = 0.f; }
    const float invD = 1.0f / D;
    for (int r = wave; r < LNB_ROWS; r += 4) {
        const size_t row = (size_t)blockIdx.x * LNB_ROWS + r;
        if (row >= M) break;
        float x[4], dy[4], s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = lane + 64 * j;
            x[j] = c < D ? X[row * D + c] : 0.f;
            dy[j] = c < D ? dY[row * D + c] : 0.f;
            s += x[j];
        }
        const float mean = wave_sum(s) * invD;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) { const int c = lane + 64 * j; x[j] = c < D ? x[j] - mean : 0.f; q += x[j] * x[j]; }
        const float rstd = rsqrtf(wave_sum(q) * invD + 1e-5f);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            x[j] *= rstd;                                   // xhat
            dg[j] += dy[j] * x[j]; db[j] += dy[j];
            dy[j] *= g[j];
            s1 += dy[j]; s2 += dy[j] * x[j];
        }
        s1 = wave_sum(s1) * invD; s2 = wave_sum(s2) * invD;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = lane + 64 * j;
            if (c < D) dX[row * D + c] = rstd * (dy[j] - s1 - x[j] * s2) + (dres ? dres[row * D + c] : 0.f);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) { red[wave][0][lane + 64 * j] = dg[j]; red[wave][1][lane + 64 * j] = db[j]; }
    __syncthreads();
    if ((int)threadIdx.x < D) {
        const int t = threadIdx.x;
        float *o = part + (size_t)blockIdx.x * 2 * D;
        o[t] = ((red[0][0][t] + red[1][0][t]) + red[2][0][t]) + red[3][0][t];
        o[D + t] = ((red[0][1][t] + red[1][1][t]) + red[2][1][t]) + red[3][1][t];
    }
}

// latent = sigmoid(LN(X[n][0])): the gradient of token row 0 (the other rows get none from the head: dX is cleared before) and
// the sample's dgamma / dbeta terms in part[n][2 D].  One wave per image.
__global__ __launch_bounds__(256) void enc_head_bwd_kernel(int N, int L, int D, const float *X, const float *w, const float *lat,
                                                           const float *dlat, float *dX, float *part)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float *xr = X + (size_t)n * L * D;
    const float invD = 1.0f / D;
    float x[4], dz[4], s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = lane + 64 * j;
        x[j] = c < D ? xr[c] : 0.f;
        const float y = c < D ? lat[(size_t)n * D + c] : 0.f;
        dz[j] = c < D ? dlat[(size_t)n * D + c] * y * (1.0f - y) : 0.f;
        s += x[j];
    }
    const float mean = wave_sum(s) * invD;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) { const int c = lane + 64 * j; x[j] = c < D ? x[j] - mean : 0.f; q += x[j] * x[j]; }
    const float rstd = rsqrtf(wave_sum(q) * invD + 1e-5f);
    float s1 = 0.f, s2 = 0.f, gy[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = lane + 64 * j;
        x[j] *= rstd;
        gy[j] = c < D ? dz[j] * w[c] : 0.f;
        s1 += gy[j]; s2 += gy[j] * x[j];
    }
    s1 = wave_sum(s1) * invD; s2 = wave_sum(s2) * invD;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = lane + 64 * j;
        if (c >= D) continue;
        dX[(size_t)n * L * D + c] = rstd * (gy[j] - s1 - x[j] * s2);
        part[(size_t)n * 2 * D + c] = dz[j] * x[j];
        part[(size_t)n * 2 * D + D + c] = dz[j];
    }
}

// The decoder's token matrix backwards, one workgroup per image: part[n][Dd] = sum of dX over the image's noise rows 1 .. L - 1
// (decoder_noise_token), dlat[n][k] = sum_c dX[n][0][c] We[c][k] (decoder_embed to the latent).
__global__ __launch_bounds__(256) void dec_seed_bwd_kernel(int L, int Dd, int De, const float *We, const float *dX, float *part, float *dlat)
{
    __shared__ float r0[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const float *x = dX + (size_t)n * L * Dd;
    if (t < Dd) {
        r0[t] = x[t];
        float s = 0.f;
        for (int r = 1; r < L; r++) s += x[(size_t)r * Dd + t];
        part[(size_t)n * Dd + t] = s;
    }
    __syncthreads();
    for (int k = t; k < De; k += 256) {
        float s = 0.f;
        for (int c = 0; c < Dd; c++) s += r0[c] * We[(size_t)c * De + k];
        dlat[(size_t)n * De + k] = s;
    }
}

// ---- vit_dw_kernel: dW[n][k] = sum_m dY[m][n] X[m][k] -----------------------------------------------------------------------
// Both operands are row-major over the reduced index m, which is exactly the fragment order of v_mfma_f32_32x32x2_f32 with
// A = dY^T and B = X: a lane's A / B element of k-pair q is column (chunk + li) of row 2q + lh.  Workgroup = 4 waves = a
// 128 (n) x 128 (k) output tile over ONE slice of rows_per_slice rows; wave w owns the 32 n of chunk w against all four
// 32-k chunks (64 accumulator registers).  Slabs of 32 rows of both operands are staged through LDS with 16-byte loads
// (pitch 160 floats: the two wave halves read rows 2q and 2q + 1 from different bank halves), so every dY element is loaded
// once per workgroup and used against 128 k.  The output is small (at most 512 x 128 per matrix at the reference's widths),
// so the parallelism comes from the slices: each writes its own partial part[slice][N K + N] (the bias gradient = column sums
// of dY ride along in the k-tile 0 workgroups) and reduce_parts_kernel adds the slices in ascending order.
// SRC 1: X rows are image patches read in place (row = (frame, gy, gx), column = P py + px), as vit_gemm_kernel<1, .> does.
struct DwArgs {
    uint32_t M;
    int N, K;                   // multiples of 32 / 128
    const float *dY; int ldy;
    int skipL;                  // > 0: dY lives in token rows, row m of X pairs with dY row m + m / (skipL - 1) + 1 (patch rows only)
    const float *X; int ldx;    // SRC 0
    const float *img; int img_size, grid, patch;   // SRC 1
    float *part;
    int rows_per_slice;         // a multiple of 32
};
constexpr int DW_SLAB = 32, DW_PITCH = 160;

template <int SRC>
__global__ __launch_bounds__(256) void vit_dw_kernel(const DwArgs a)
{
    __shared__ __attribute__((aligned(16))) float Ys[DW_SLAB * DW_PITCH], Xs[DW_SLAB * DW_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int ntk = a.K / 128, n0 = ((int)blockIdx.x / ntk) * 128, kt = (int)blockIdx.x % ntk, k0 = kt * 128;
    const uint32_t mbeg = blockIdx.y * (uint32_t)a.rows_per_slice;
    const uint32_t mend = mbeg + a.rows_per_slice < a.M ? mbeg + a.rows_per_slice : a.M;
    const bool cok = n0 + 32 * wave < a.N;
    f32x16t acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
    float bsum = 0.f;
    const int G = a.grid, P = a.patch;
    for (uint32_t m0 = mbeg; m0 < mend; m0 += DW_SLAB) {
        if (m0 != mbeg) __syncthreads();                                   // the previous slab has been consumed
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = threadIdx.x + 256 * i, r = p >> 5, c4 = (p & 31) * 4;
            const uint32_t m = m0 + r;
            float4 y = make_float4(0.f, 0.f, 0.f, 0.f), x = y;             // rows past the slice add nothing
            if (m < mend) {
                const uint32_t yrow = a.skipL ? m + m / (uint32_t)(a.skipL - 1) + 1 : m;
                if (n0 + c4 < a.N) y = *reinterpret_cast<const float4 *>(a.dY + (size_t)yrow * a.ldy + n0 + c4);
                if (SRC == 0) x = *reinterpret_cast<const float4 *>(a.X + (size_t)m * a.ldx + k0 + c4);
                else {
                    const int k = k0 + c4;
                    const uint32_t fn = m / (uint32_t)(G * G), pp = m % (uint32_t)(G * G), gy = pp / G, gx = pp % G;
                    x = *reinterpret_cast<const float4 *>(a.img + ((size_t)fn * a.img_size + gy * P + k / P) * a.img_size + gx * P + k % P);
                }
            }
            *reinterpret_cast<float4 *>(&Ys[r * DW_PITCH + c4]) = y;
            *reinterpret_cast<float4 *>(&Xs[r * DW_PITCH + c4]) = x;
        }
        __syncthreads();
        if (kt == 0 && threadIdx.x < 128) {
#pragma unroll 8
            for (int r = 0; r < DW_SLAB; r++) bsum += Ys[r * DW_PITCH + threadIdx.x];
        }
        if (cok) {
#pragma unroll
            for (int q = 0; q < DW_SLAB / 2; q++) {
                const float af = Ys[(2 * q + lh) * DW_PITCH + 32 * wave + li];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, Xs[(2 * q + lh) * DW_PITCH + 32 * j + li], acc[j], 0, 0, 0);
            }
        }
    }
    float *o = a.part + (size_t)blockIdx.y * ((size_t)a.N * a.K + a.N);
    if (cok) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int e = 0; e < 16; e++)
                o[(size_t)(n0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * lh) * a.K + k0 + 32 * j + li] = acc[j][e];
    }
    if (kt == 0 && threadIdx.x < 128 && n0 + (int)threadIdx.x < a.N) o[(size_t)a.N * a.K + n0 + threadIdx.x] = bsum;
}

// ---- attention_bwd_kernel ------------------------------------------------------------------------------------------------
// One workgroup (eight waves) per (image, head), head dimension 32, L <= 224 tokens = NT <= 7 tiles of 32.  LDS: Q, K, V, dO of
// the head as [32 NT][33] each (rows past L zero: a padded query has dO = 0 and so adds nothing, a padded key is masked), one
// 32 x 33 transposition tile per wave, the waves' softmax statistics and delta = rowsum(dO o O): 155,008 bytes at NT = 7.
// Wave w owns KEY tile w for the whole kernel (waves >= NT only stage, sum and keep the barriers).  Over the query tiles:
//   S = Q K^T and dP = dO V^T for (query tile, key tile w), both with A = the query-side rows, B = the key-side rows: in the
//   accumulator layout a lane then owns ONE key (column li) and its 16 registers run over the queries (e & 3) + 8 (e >> 2) + 4 lh.
//   The row maximum / sum of a query is a reduction over the 32 lanes of a wave half per register, then over the waves through
//   LDS (two barriers); P = exp2(S' - max) / sum, dS = P o (dP - delta).  Masked keys give P = dS = 0 exactly.
//   dV^T += dO^T P and dK^T += Q^T dS take P / dS straight from those registers as B operands (k-pair e = queries a_e, a_e + 4 with
//   a_e = (e & 3) + 8 (e >> 2): a sum does not care about the order) with the A fragments fetched from LDS in that order; the
//   two 32 x 32 accumulators live across the query loop and are stored once, lane = key, four 16-byte stores.
//   dQ needs the sum over keys, i.e. over lanes: the wave transposes its dS tile through its LDS tile, forms its key tile's share
//   dS K (A = dS rows from the tile, B = K rows), writes it back to the tile, and after a barrier all threads add the NT shares
//   in ascending order and store the dQ rows.  No atomics: the same inputs give the same bits.
constexpr int AB_P = 33, AB_TILE = 32 * AB_P;

__device__ __forceinline__ float half_reduce_max(float v)
{
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float half_reduce_sum(float v)
{
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(512, 1) void attention_bwd_kernel(int L, int D, int heads, const float *QKV, const float *O, const float *dO,
                                                               float *dQKV)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int NT = (L + 31) / 32, Lp = NT * 32;
    float *Qs = sm, *Ks = Qs + Lp * AB_P, *Vs = Ks + Lp * AB_P, *Gs = Vs + Lp * AB_P;      // Gs = dO
    float *T = Gs + Lp * AB_P, *wmax = T + 8 * AB_TILE, *wsum = wmax + 256, *delta = wsum + 256;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads;
    const float *base = QKV + (size_t)n * L * 3 * D + h * 32;
    const size_t obase = (size_t)n * L * D + h * 32;
    {
        const int c4 = (threadIdx.x & 7) * 4;                              // eight threads per 32-wide head row
        for (int l = threadIdx.x >> 3; l < Lp; l += 64) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f), k = q, v = q, g = q, o = q;
            if (l < L) {
                q = *reinterpret_cast<const float4 *>(base + (size_t)l * 3 * D + c4);
                k = *reinterpret_cast<const float4 *>(base + (size_t)l * 3 * D + D + c4);
                v = *reinterpret_cast<const float4 *>(base + (size_t)l * 3 * D + 2 * D + c4);
                g = *reinterpret_cast<const float4 *>(dO + obase + (size_t)l * D + c4);
                o = *reinterpret_cast<const float4 *>(O + obase + (size_t)l * D + c4);
            }
            float *qd = Qs + l * AB_P + c4, *kd = Ks + l * AB_P + c4, *vd = Vs + l * AB_P + c4, *gd = Gs + l * AB_P + c4;
            qd[0] = q.x; qd[1] = q.y; qd[2] = q.z; qd[3] = q.w;
            kd[0] = k.x; kd[1] = k.y; kd[2] = k.z; kd[3] = k.w;
            vd[0] = v.x; vd[1] = v.y; vd[2] = v.z; vd[3] = v.w;
            gd[0] = g.x; gd[1] = g.y; gd[2] = g.z; gd[3] = g.w;
            float dl = (g.x * o.x + g.y * o.y) + (g.z * o.z + g.w * o.w);
            dl += __shfl_xor(dl, 1, 64); dl += __shfl_xor(dl, 2, 64); dl += __shfl_xor(dl, 4, 64);
            if ((threadIdx.x & 7) == 0) delta[l] = dl;
        }
    }
    __syncthreads();
    const float scale = rsqrtf(32.0f), sl2 = scale * 1.44269504088896341f;
    const bool act = wave < NT;                                            // wave-uniform
    const int key0 = 32 * wave;
    float *Tw = T + wave * AB_TILE;
    f32x16t accK, accV;
#pragma unroll
    for (int e = 0; e < 16; e++) { accK[e] = 0.f; accV[e] = 0.f; }
    for (int qt = 0; qt < NT; qt++) {
        const int r0 = 32 * qt;
        f32x16t S, dP;
        if (act) {
#pragma unroll
            for (int e = 0; e < 16; e++) { S[e] = 0.f; dP[e] = 0.f; }
#pragma unroll
            for (int q = 0; q < 16; q++) {
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[(r0 + li) * AB_P + 2 * q + lh], Ks[(key0 + li) * AB_P + 2 * q + lh], S, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[(r0 + li) * AB_P + 2 * q + lh], Vs[(key0 + li) * AB_P + 2 * q + lh], dP, 0, 0, 0);
            }
            const bool masked = key0 + li >= L;                            // this lane's key is padding
#pragma unroll
            for (int e = 0; e < 16; e++) {
                S[e] = masked ? -3.0e38f : S[e] * sl2;
                const float m = half_reduce_max(S[e]);
                if (li == 0) wmax[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh] = m;
            }
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int qr = (e & 3) + 8 * (e >> 2) + 4 * lh;
                float m = wmax[qr];
                for (int w = 1; w < NT; w++) m = fmaxf(m, wmax[w * 32 + qr]);
                S[e] = __builtin_amdgcn_exp2f(S[e] - m);
                const float t = half_reduce_sum(S[e]);
                if (li == 0) wsum[wave * 32 + qr] = t;
            }
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int qr = (e & 3) + 8 * (e >> 2) + 4 * lh;
                float den = wsum[qr];
                for (int w = 1; w < NT; w++) den += wsum[w * 32 + qr];
                S[e] = S[e] / den;                                         // P
                dP[e] = S[e] * (dP[e] - delta[r0 + qr]);                   // dS (of the scaled scores)
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int qrow = r0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                accV = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[qrow * AB_P + li], S[e], accV, 0, 0, 0);
                accK = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[qrow * AB_P + li], dP[e], accK, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; e++) Tw[((e & 3) + 8 * (e >> 2) + 4 * lh) * AB_P + li] = dP[e];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // the wave's own tile: program order is enough
            __builtin_amdgcn_wave_barrier();
            f32x16t dq;
#pragma unroll
            for (int e = 0; e < 16; e++) dq[e] = 0.f;
#pragma unroll
            for (int q = 0; q < 16; q++)
                dq = __builtin_amdgcn_mfma_f32_32x32x2f32(Tw[li * AB_P + 2 * q + lh], Ks[(key0 + 2 * q + lh) * AB_P + li], dq, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; e++) Tw[((e & 3) + 8 * (e >> 2) + 4 * lh) * AB_P + li] = dq[e];      // [query][dim]
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 1024; idx += 512) {
            const int q = idx >> 5, c = idx & 31;
            if (r0 + q >= L) continue;
            float s = T[q * AB_P + c];
            for (int w = 1; w < NT; w++) s += T[w * AB_TILE + q * AB_P + c];
            dQKV[((size_t)n * L + r0 + q) * 3 * D + h * 32 + c] = s * scale;
        }
        // (the next iteration's first write to T / wsum lies behind its first barrier, its write to wmax behind this sum's reads
        // of T only: wmax was last read before the second barrier above)
    }
    if (act && key0 + li < L) {
        float *kp = dQKV + ((size_t)n * L + key0 + li) * 3 * D + D + h * 32 + 4 * lh, *vp = kp + D;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            *reinterpret_cast<float4 *>(kp + 8 * g) = make_float4(accK[4 * g] * scale, accK[4 * g + 1] * scale, accK[4 * g + 2] * scale, accK[4 * g + 3] * scale);
            *reinterpret_cast<float4 *>(vp + 8 * g) = make_float4(accV[4 * g], accV[4 * g + 1], accV[4 * g + 2], accV[4 * g + 3]);
        }
    }
}

}  // namespace osv

using namespace osv;

namespace {

// flat offsets of a block's twelve tensors (include/optistate_hip.h), and its length
struct BlockOff { size_t ln1, qkvw, qkvb, projw, projb, ln2, fc1w, fc1b, fc2w, fc2b, total; };
BlockOff block_off(const VitDims &d)
{
    const size_t D = d.dim, Mh = d.mlp;
    BlockOff o;
    o.ln1 = 0; o.qkvw = 2 * D; o.qkvb = o.qkvw + 3 * D * D; o.projw = o.qkvb + 3 * D; o.projb = o.projw + D * D;
    o.ln2 = o.projb + D; o.fc1w = o.ln2 + 2 * D; o.fc1b = o.fc1w + Mh * D; o.fc2w = o.fc1b + Mh; o.fc2b = o.fc2w + D * Mh;
    o.total = o.fc2b + D;
    return o;
}

// workspace slices of one block (floats): its input, qkv, attention output, the residual stream behind the attention, the fc1
// pre-activation and its GELU; the block's output is the next block's input
struct BlockWs { size_t xin, qkv, ao, xmid, h, g, total; };
BlockWs block_ws(const VitDims &d, size_t M)
{
    const size_t D = d.dim, Mh = d.mlp;
    BlockWs o;
    o.xin = 0; o.qkv = M * D; o.ao = o.qkv + M * 3 * D; o.xmid = o.ao + M * D; o.h = o.xmid + M * D; o.g = o.h + M * Mh;
    o.total = o.g + M * Mh;
    return o;
}

// a stack whose attention runs on the key-tiled kernels (vit_attn_tiled.hip): whatever the whole-head backward cannot hold, and
// every stack under OS_VIT_ATT_TILED=1
bool att_tiled(const os_ctx *ctx, const VitDims &d)
{
    return d.dim / d.heads != 32 || ntok(d) > 224 || ctx->tune_vit_att_tiled;
}

// the whole workspace: encoder blocks | encoder output X | latent | decoder blocks | decoder output X | pred, then per block of a
// stack on the tiled kernels its softmax statistics [N][heads][L] (encoder, decoder)
struct TrainWs { size_t enc, lat, dec, pred, lse_enc, lse_dec, total; };
TrainWs train_ws(const os_ctx *ctx, const VitDims &e, const VitDims &dd, int N)
{
    const size_t M = (size_t)N * ntok(e);
    TrainWs o;
    o.enc = 0;
    o.lat = o.enc + e.depth * block_ws(e, M).total + M * e.dim;
    o.dec = o.lat + (size_t)N * e.dim;
    o.pred = o.dec + dd.depth * block_ws(dd, M).total + M * dd.dim;
    o.lse_enc = o.pred + (size_t)N * (ntok(dd) - 1) * dd.patch * dd.patch;
    o.lse_dec = o.lse_enc + (att_tiled(ctx, e) ? e.depth * M * e.heads : 0);
    o.total = o.lse_dec + (att_tiled(ctx, dd) ? dd.depth * M * dd.heads : 0);
    return o;
}

size_t max2(size_t a, size_t b) { return a > b ? a : b; }

int rows_per_slice(size_t M)
{
    const size_t r = (M + 63) / 64;                       // at most 64 slices
    return (int)max2(256, (r + 31) / 32 * 32);
}

// the loaded encoder / decoder pair if the training step supports it at N images (0), or the error code with its message
int train_state(os_ctx *ctx, int N, os_vit_state **out)
{
    os_vit_state *v = (os_vit_state *)ctx->vit;
    if (!v || !v->w || !v->dec) return os_fail(ctx, -5, "os_vit training: call os_vit_load and os_vit_load_decoder first");
    const VitDims &e = v->d, &dd = v->dec->d;
    const int he = e.dim / e.heads, hdd = dd.dim / dd.heads;
    if ((he != 32 && he != 64) || (hdd != 32 && hdd != 64) || e.img != dd.img || e.patch != dd.patch || v->dec->latent_dim != e.dim)
        return os_fail(ctx, -4, "os_vit training: needs head dimension 32 or 64 in encoder and decoder and one image geometry");
    const size_t bigw = max2(max2(3 * e.dim, e.mlp), max2(3 * dd.dim, dd.mlp));
    if (N <= 0 || (uint64_t)N * ntok(e) * bigw * 4 >= (1ull << 32)) return os_fail(ctx, -2, "os_vit training: N must be positive and N * tokens * width below 2^30");
    *out = v;
    return 0;
}

void fill(os_ctx *ctx, float *p, size_t n, hipStream_t s)
{
    const int slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "fill_kernel");
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 1023) / 1024 < 1024 ? (n + 1023) / 1024 : 1024)), dim3(256), 0, s, p, n, 0.f);
    os_prof_end(ctx, slot, s);
}

void reduce_parts(os_ctx *ctx, int S, size_t n, size_t stride, const float *part, float *out, hipStream_t s)
{
    const int slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "reduce_parts_kernel");
    hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S, n, stride, part, out);
    os_prof_end(ctx, slot, s);
}

// scratch of one backward call
struct Bwd {
    os_ctx *ctx; os_vit_state *v; hipStream_t s;
    size_t M;
    float *dX, *dT, *dBig, *Yn, *wt, *part;
    float *delta;               // [N][heads][L] of the block in flight (stacks on the tiled attention kernels)
};

// grad[W | b] of a linear layer y = x W^T + b from dY [M][N] and X [M][K] (img: X are the image patches, dY in token rows)
void weight_grad(const Bwd &b, int N, int K, const float *dY, int ldy, const float *X, const float *img, const VitDims *pd, float *grad)
{
    DwArgs a;
    a.M = (uint32_t)b.M; a.N = N; a.K = K; a.dY = dY; a.ldy = ldy; a.skipL = 0; a.X = X; a.ldx = K; a.img = nullptr;
    a.img_size = a.grid = a.patch = 0; a.part = b.part; a.rows_per_slice = rows_per_slice(b.M);
    if (img) { a.img = img; a.img_size = pd->img; a.grid = grid_of(*pd); a.patch = pd->patch; a.skipL = ntok(*pd); a.M = (uint32_t)(b.M / ntok(*pd) * (ntok(*pd) - 1)); }
    const int slices = (int)((a.M + a.rows_per_slice - 1) / a.rows_per_slice);
    const dim3 grid((unsigned)((N + 127) / 128 * (K / 128)), (unsigned)slices);
    const int slot = os_prof_begin(b.ctx, OS_PHASE_TRAIN_DW, b.s, "vit_dw_kernel");
    if (img) hipLaunchKernelGGL(vit_dw_kernel<1>, grid, dim3(256), 0, b.s, a);
    else hipLaunchKernelGGL(vit_dw_kernel<0>, grid, dim3(256), 0, b.s, a);
    os_prof_end(b.ctx, slot, b.s);
    const size_t n = (size_t)N * K + N;
    reduce_parts(b.ctx, slices, n, n, b.part, grad, b.s);
}

// dXin [M][Kin] = dY [M][Nout] . W  (W [Nout][Kin] flat); with the pre-activations H of a GELU in front: * gelu'(H).
// Wt: W's resident transposed pack (vit_adamw_pack_kernel keeps it current), or null: packed here into b.wt -- the same floats.
int input_grad(const Bwd &b, int Nout, int Kin, const float *W, const float *Wt, const float *dY, float *dXin, const float *H)
{
    int slot;
    if (!Wt) {
        slot = os_prof_begin(b.ctx, OS_PHASE_TRAIN_MISC, b.s, "vit_pack_wt_kernel");
        hipLaunchKernelGGL(vit_pack_wt_kernel, dim3(256), dim3(256), 0, b.s, Kin, Nout, W, b.wt);
        os_prof_end(b.ctx, slot, b.s);
        Wt = b.wt;
    }
    GemmArgs g;
    g.M = b.M; g.N = Kin; g.K = Nout; g.lda = Nout; g.A = dY; g.img = nullptr; g.img_size = g.grid = g.patch = 0; g.Wp = Wt;
    g.bias = nullptr; g.C = dXin; g.pos = nullptr; g.L = 0; g.R = nullptr; g.C2 = nullptr;
    if (int rc = os_vit_launch_gemm(b.ctx, 0, 7, g, b.s, "vit_gemm_kernel<dX>")) return rc;
    if (H) {
        slot = os_prof_begin(b.ctx, OS_PHASE_TRAIN_MISC, b.s, "gelu_bwd_kernel");
        hipLaunchKernelGGL(gelu_bwd_kernel, dim3(2048), dim3(256), 0, b.s, b.M * Kin, H, dXin);
        os_prof_end(b.ctx, slot, b.s);
    }
    return 0;
}

// dX = dres + LayerNorm backward of dY at input X; grad[gamma | beta]
void ln_grad(const Bwd &b, int D, const float *X, const float *dY, const float *gamma, const float *dres, float *dX, float *grad)
{
    const int nblk = (int)((b.M + LNB_ROWS - 1) / LNB_ROWS);
    const int slot = os_prof_begin(b.ctx, OS_PHASE_TRAIN_MISC, b.s, "ln_bwd_kernel");
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(nblk), dim3(256), 0, b.s, b.M, D, X, dY, gamma, dres, dX, b.part);
    os_prof_end(b.ctx, slot, b.s);
    reduce_parts(b.ctx, nblk, (size_t)2 * D, (size_t)2 * D, b.part, grad, b.s);
}

// forward of the blocks of d with the activations kept: ws at block 0's slices, w / wp as os_vit_run_blocks takes them; lse: block
// 0's softmax statistics for a stack on the tiled attention kernels, else null
int blocks_forward(os_ctx *ctx, os_vit_state *v, const VitDims &d, const float *w, const float *wp, float *ws, float *lse, float *Y, int N,
                   hipStream_t s)
{
    const int D = d.dim, Mh = d.mlp;
    const size_t M = (size_t)N * ntok(d);
    const BlockOff o = block_off(d);
    const BlockWs k = block_ws(d, M);
    GemmArgs g;
    g.img = nullptr; g.img_size = g.grid = g.patch = 0; g.pos = nullptr; g.L = 0; g.M = M;
    for (int blk = 0; blk < d.depth; blk++, w += o.total, ws += k.total) {
        float *xin = ws + k.xin, *xout = ws + k.total + k.xin;
        os_vit_launch_layernorm(ctx, M, D, xin, w + o.ln1, w + o.ln1 + D, Y, s);
        g.A = Y; g.lda = D; g.N = 3 * D; g.K = D; g.Wp = wp; g.bias = w + o.qkvb; g.C = ws + k.qkv; g.R = nullptr; g.C2 = nullptr;
        if (int rc = os_vit_launch_gemm(ctx, 0, 0, g, s, "vit_gemm_kernel<+bias>")) return rc;
        wp += (size_t)3 * D * D;
        if (lse) {
            if (int rc = os_vit_launch_attention_tiled(ctx, d, N, ws + k.qkv, ws + k.ao, lse + (size_t)blk * M * d.heads, s, "attention_tiled_fwd_kernel<lse>")) return rc;
        } else if (int rc = os_vit_launch_attention(ctx, v, d, N, ws + k.qkv, w + o.qkvb, ws + k.ao, s)) return rc;
        g.A = ws + k.ao; g.N = D; g.Wp = wp; g.bias = w + o.projb; g.C = ws + k.xmid; g.R = xin;
        if (int rc = os_vit_launch_gemm(ctx, 0, 4, g, s, "vit_gemm_kernel<+bias,+residual to>")) return rc;
        wp += (size_t)D * D;
        os_vit_launch_layernorm(ctx, M, D, ws + k.xmid, w + o.ln2, w + o.ln2 + D, Y, s);
        g.A = Y; g.N = Mh; g.Wp = wp; g.bias = w + o.fc1b; g.C = ws + k.h; g.R = nullptr; g.C2 = ws + k.g;
        if (int rc = os_vit_launch_gemm(ctx, 0, 5, g, s, "vit_gemm_kernel<+bias,gelu beside>")) return rc;
        wp += (size_t)Mh * D;
        g.A = ws + k.g; g.lda = Mh; g.N = D; g.K = Mh; g.Wp = wp; g.bias = w + o.fc2b; g.C = xout; g.R = ws + k.xmid; g.C2 = nullptr;
        if (int rc = os_vit_launch_gemm(ctx, 0, 4, g, s, "vit_gemm_kernel<+bias,+residual to>")) return rc;
        wp += (size_t)D * Mh;
        OS_HIP(ctx, hipGetLastError());
    }
    return 0;
}

// backward of the blocks of d, last to first: b.dX holds the gradient of the last block's output on entry and of block 0's input
// on return.  w / ws / grad at block 0; wtr: the stack's resident transposed packs (per block qkv, proj, fc1, fc2) or null; lse:
// block 0's softmax statistics as blocks_forward left them (tiled attention kernels), or null (attention_bwd_kernel).
int blocks_backward(const Bwd &b, const VitDims &d, const float *w, const float *wtr, const float *ws, const float *lse, float *grad, int N)
{
    const int D = d.dim, Mh = d.mlp;
    const BlockOff o = block_off(d);
    const BlockWs k = block_ws(d, b.M);
    os_vit_state *v = b.v;
    if (!lse && !v->att_bwd_attr_set) {
        OS_HIP(b.ctx, hipFuncSetAttribute((const void *)attention_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        v->att_bwd_attr_set = true;
    }
    const int L = ntok(d), Lp = (L + 31) / 32 * 32;
    const size_t alds = ((size_t)4 * Lp * AB_P + 8 * AB_TILE + 512 + Lp) * sizeof(float);
    for (int blk = d.depth - 1; blk >= 0; blk--) {
        const float *wb = w + blk * o.total, *a = ws + blk * k.total;
        float *gb = grad + blk * o.total;
        const size_t DD = (size_t)D * D, MD = (size_t)Mh * D;
        const float *tq = wtr ? wtr + blk * (4 * DD + 2 * MD) : nullptr, *tp = wtr ? tq + 3 * DD : nullptr;
        const float *t1 = wtr ? tp + DD : nullptr, *t2 = wtr ? t1 + MD : nullptr;
        // x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
        weight_grad(b, D, Mh, b.dX, D, a + k.g, nullptr, nullptr, gb + o.fc2w);
        if (int rc = input_grad(b, D, Mh, wb + o.fc2w, t2, b.dX, b.dBig, a + k.h)) return rc;
        os_vit_launch_layernorm(b.ctx, b.M, D, a + k.xmid, wb + o.ln2, wb + o.ln2 + D, b.Yn, b.s);
        weight_grad(b, Mh, D, b.dBig, Mh, b.Yn, nullptr, nullptr, gb + o.fc1w);
        if (int rc = input_grad(b, Mh, D, wb + o.fc1w, t1, b.dBig, b.dT, nullptr)) return rc;
        ln_grad(b, D, a + k.xmid, b.dT, wb + o.ln2, b.dX, b.dX, gb + o.ln2);
        // x_mid = x_in + proj(attention(qkv(LN1(x_in))))
        weight_grad(b, D, D, b.dX, D, a + k.ao, nullptr, nullptr, gb + o.projw);
        if (int rc = input_grad(b, D, D, wb + o.projw, tp, b.dX, b.dT, nullptr)) return rc;
        if (lse) {
            if (int rc = os_vit_launch_attention_tiled_bwd(b.ctx, d, N, a + k.qkv, a + k.ao, b.dT, lse + (size_t)blk * b.M * d.heads, b.delta, b.dBig, b.s))
                return rc;
        } else {
            const int slot = os_prof_begin(b.ctx, OS_PHASE_VIT_ATTN, b.s, "attention_bwd_kernel");
            hipLaunchKernelGGL(attention_bwd_kernel, dim3(N * d.heads), dim3(512), alds, b.s, L, D, d.heads, a + k.qkv, a + k.ao, b.dT, b.dBig);
            os_prof_end(b.ctx, slot, b.s);
        }
        os_vit_launch_layernorm(b.ctx, b.M, D, a + k.xin, wb + o.ln1, wb + o.ln1 + D, b.Yn, b.s);
        weight_grad(b, 3 * D, D, b.dBig, 3 * D, b.Yn, nullptr, nullptr, gb + o.qkvw);
        if (int rc = input_grad(b, 3 * D, D, wb + o.qkvw, tq, b.dBig, b.dT, nullptr)) return rc;
        ln_grad(b, D, a + k.xin, b.dT, wb + o.ln1, b.dX, b.dX, gb + o.ln1);
        OS_HIP(b.ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

size_t os_vit_train_ws_floats(os_ctx *ctx, int32_t N)
{
    if (!ctx || ctx->magic != OS_MAGIC) return 0;
    os_vit_state *v;
    return train_state(ctx, N, &v) ? 0 : train_ws(ctx, v->d, v->dec->d, N).total;
}

int os_vit_forward_train(os_ctx *ctx, int32_t N, const float *images, float *ws, float *pred, float *loss, void *stream)
{
    OS_CHECK_CTX(ctx);
    if (!images || !ws || !loss) return os_fail(ctx, -2, "os_vit_forward_train: null pointer");
    os_vit_state *v;
    if (int rc = train_state(ctx, N, &v)) return rc;
    OS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    os_vit_dec_state *q = v->dec;
    const VitDims &e = v->d, &dd = q->d;
    const int D = e.dim, Dd = dd.dim, L = ntok(e), PP = e.patch * e.patch;
    const size_t M = (size_t)N * L;
    if (os_ensure_scratch(ctx, &v->buf, &v->buf_floats, M * max2(D, Dd))) return -10;
    float *Y = v->buf;
    const TrainWs t = train_ws(ctx, e, dd, N);
    // encoder: patch embedding + position table, cls rows, blocks, sigmoid(LN(cls row))
    const float *w = v->w, *patch_b = w + (size_t)D * PP, *cls = patch_b + D, *pos = cls + D;
    w = pos + (size_t)L * D;
    GemmArgs g;
    g.img = images; g.img_size = e.img; g.grid = grid_of(e); g.patch = e.patch; g.pos = pos; g.L = L; g.A = nullptr; g.lda = 0;
    g.M = (size_t)N * (L - 1); g.N = D; g.K = PP; g.Wp = v->wp; g.bias = patch_b; g.C = ws + t.enc; g.R = nullptr; g.C2 = nullptr;
    if (int rc = os_vit_launch_gemm(ctx, 1, 3, g, s, "vit_gemm_kernel<patch,+pos>")) return rc;
    os_vit_launch_cls_row(ctx, N, L, D, cls, pos, ws + t.enc, s);
    if (int rc = blocks_forward(ctx, v, e, w, v->wp + (size_t)D * PP, ws + t.enc, att_tiled(ctx, e) ? ws + t.lse_enc : nullptr, Y, N, s)) return rc;
    w += e.depth * block_off(e).total;
    os_vit_launch_cls_head(ctx, N, L, D, ws + t.enc + e.depth * block_ws(e, M).total, w, w + D, ws + t.lat, s);
    // decoder: token matrix, blocks, decoder_norm + decoder_pred + loss
    if (int rc = os_vit_dec_seed(ctx, q, N, ws + t.lat, ws + t.dec, s)) return rc;
    w = q->w + (size_t)Dd * D + 2 * Dd + (size_t)L * Dd;
    if (int rc = blocks_forward(ctx, v, dd, w, q->wp, ws + t.dec, att_tiled(ctx, dd) ? ws + t.lse_dec : nullptr, Y, N, s)) return rc;
    w += dd.depth * block_off(dd).total;
    if (int rc = os_vit_dec_tail(ctx, q, N, w, ws + t.dec + dd.depth * block_ws(dd, M).total, images, ws + t.pred, nullptr, loss, s)) return rc;
    if (pred) OS_HIP(ctx, hipMemcpyAsync(pred, ws + t.pred, (t.lse_enc - t.pred) * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

int os_vit_backward(os_ctx *ctx, int32_t N, const float *images, const float *ws, const float *dloss, float *grad_enc, float *grad_dec,
                    void *stream)
{
    OS_CHECK_CTX(ctx);
    if (!images || !ws || !dloss || !grad_enc || !grad_dec) return os_fail(ctx, -2, "os_vit_backward: null pointer");
    os_vit_state *v;
    if (int rc = train_state(ctx, N, &v)) return rc;
    OS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    os_vit_dec_state *q = v->dec;
    const VitDims &e = v->d, &dd = q->d;
    const int D = e.dim, Dd = dd.dim, L = ntok(e), PP = e.patch * e.patch, NP = dd.patch * dd.patch;
    const size_t M = (size_t)N * L, Dm = max2(D, Dd), bigw = max2(max2(3 * D, e.mlp), max2(3 * Dd, dd.mlp));
    const TrainWs t = train_ws(ctx, e, dd, N);
    // scratch: dX | dT | Yn [M][Dm], dBig [M][bigw], dpred [M][NP] (token rows), the transposed pack of one matrix, the partials of
    // one reduction, dlatent, delta = rowsum(dO o O) of one block's attention (stacks on the tiled kernels)
    const size_t wt_floats = max2(max2((size_t)NP * Dd, max2(3 * (size_t)D * D, (size_t)e.mlp * D)), max2(3 * (size_t)Dd * Dd, (size_t)dd.mlp * Dd));
    const int slices = (int)((M + rows_per_slice(M) - 1) / rows_per_slice(M));
    const size_t nk = max2(max2((size_t)D * PP + D, wt_floats + bigw), (size_t)NP * Dd + NP);
    const size_t part_floats = max2(max2((size_t)slices * nk, ((M + LNB_ROWS - 1) / LNB_ROWS) * 2 * Dm), (size_t)N * 2 * Dm);
    const size_t delta_floats = M * max2(att_tiled(ctx, e) ? e.heads : 0, att_tiled(ctx, dd) ? dd.heads : 0);
    const size_t need = 3 * M * Dm + M * bigw + M * NP + wt_floats + part_floats + (size_t)N * D + delta_floats;
    if (os_ensure_scratch(ctx, &v->tbuf, &v->tbuf_floats, need)) return -10;
    Bwd b;
    b.ctx = ctx; b.v = v; b.s = s; b.M = M;
    b.dX = v->tbuf; b.dT = b.dX + M * Dm; b.Yn = b.dT + M * Dm; b.dBig = b.Yn + M * Dm;
    float *dpred = b.dBig + M * bigw;
    b.wt = dpred + M * NP; b.part = b.wt + wt_floats;
    float *dlat = b.part + part_floats;
    b.delta = dlat + (size_t)N * D;
    // ---- decoder ----
    const float *wd = q->w;
    const size_t o_be = (size_t)Dd * D, o_noise = o_be + Dd, o_dpos = o_noise + Dd, o_dblk = o_dpos + (size_t)L * Dd;
    const size_t o_dnorm = o_dblk + dd.depth * block_off(dd).total, o_pred = o_dnorm + 2 * Dd;
    const float *xd_out = ws + t.dec + dd.depth * block_ws(dd, M).total;
    int slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "loss_grad_kernel");
    hipLaunchKernelGGL(loss_grad_kernel, dim3(1024), dim3(256), 0, s, (uint32_t)M, L, grid_of(dd), dd.patch, NP, images, ws + t.pred, dloss,
                       (float)(1.0 / ((double)N * (L - 1) * NP)), dpred);
    os_prof_end(ctx, slot, s);
    os_vit_launch_layernorm(ctx, M, Dd, xd_out, wd + o_dnorm, wd + o_dnorm + Dd, b.Yn, s);
    weight_grad(b, NP, Dd, dpred, NP, b.Yn, nullptr, nullptr, grad_dec + o_pred);
    const float *wtd = q->wpt_valid ? q->wpt : nullptr, *wte = v->wpt_valid ? v->wpt : nullptr;
    const float *wtpred = wtd ? wtd + (size_t)dd.depth * (4 * (size_t)Dd * Dd + 2 * (size_t)dd.mlp * Dd) : nullptr;
    if (int rc = input_grad(b, NP, Dd, wd + o_pred, wtpred, dpred, b.dT, nullptr)) return rc;
    ln_grad(b, Dd, xd_out, b.dT, wd + o_dnorm, nullptr, b.dX, grad_dec + o_dnorm);
    if (int rc = blocks_backward(b, dd, wd + o_dblk, wtd, ws + t.dec, att_tiled(ctx, dd) ? ws + t.lse_dec : nullptr, grad_dec + o_dblk, N)) return rc;
    // the token matrix: decoder_embed (row 0 of every image), the noise token (the other rows), no gradient for the position table
    slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "dec_seed_bwd_kernel");
    hipLaunchKernelGGL(dec_seed_bwd_kernel, dim3(N), dim3(256), 0, s, L, Dd, D, wd, b.dX, b.part, dlat);
    os_prof_end(ctx, slot, s);
    reduce_parts(ctx, N, Dd, Dd, b.part, grad_dec + o_noise, s);
    reduce_parts(ctx, N, Dd, (size_t)L * Dd, b.dX, grad_dec + o_be, s);
    slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "outer_sum_kernel");
    hipLaunchKernelGGL(outer_sum_kernel, dim3((Dd * D + 255) / 256), dim3(256), 0, s, N, Dd, D, b.dX, (size_t)L * Dd, ws + t.lat, (size_t)D, grad_dec);
    os_prof_end(ctx, slot, s);
    fill(ctx, grad_dec + o_dpos, (size_t)L * Dd, s);
    // ---- encoder ----
    const float *we = v->w;
    const size_t o_pb = (size_t)D * PP, o_cls = o_pb + D, o_pos = o_cls + D, o_blk = o_pos + (size_t)L * D;
    const size_t o_norm = o_blk + e.depth * block_off(e).total;
    const float *xe_out = ws + t.enc + e.depth * block_ws(e, M).total;
    fill(ctx, b.dX, M * D, s);
    slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "enc_head_bwd_kernel");
    hipLaunchKernelGGL(enc_head_bwd_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, L, D, xe_out, we + o_norm, ws + t.lat, dlat, b.dX, b.part);
    os_prof_end(ctx, slot, s);
    reduce_parts(ctx, N, (size_t)2 * D, (size_t)2 * D, b.part, grad_enc + o_norm, s);
    if (int rc = blocks_backward(b, e, we + o_blk, wte, ws + t.enc, att_tiled(ctx, e) ? ws + t.lse_enc : nullptr, grad_enc + o_blk, N)) return rc;
    reduce_parts(ctx, N, D, (size_t)L * D, b.dX, grad_enc + o_cls, s);
    weight_grad(b, D, PP, b.dX, D, nullptr, images, &e, grad_enc);
    fill(ctx, grad_enc + o_pos, (size_t)L * D, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
