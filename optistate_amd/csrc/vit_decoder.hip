// vit_decoder.hip -- decoder half of the reference's ViT auto-encoder (transformer/transformer_model.py:137-175): latent ->
// decoder_embed -> [embedded latent | num_patches noise tokens] + fixed position table -> decoder blocks -> decoder_norm ->
// decoder_pred -> patch rows, their un-patchified image and the MSE against the input frames.
//
// The blocks are the encoder's (os_vit_run_blocks, vit_kernels.hip).  What is the decoder's own:
//   dec_seed_kernel         the token matrix: one matvec row per image, the other rows are the same table for every image
//   dec_pred_kernel         the tail as ONE kernel over the PATCH rows only: rows staged by LDS-DMA, decoder_norm on the staged
//                           tile, fp32-MFMA product with the packed decoder_pred, and an epilogue that writes the reference's
//                           pred layout, the un-patchified image and a per-workgroup float64 partial of the squared error
//                           against the input pixels.  The normalised rows never reach memory, the cls row is never computed,
//                           and there is no separate loss pass.
//   dec_loss_finish_kernel  the partials summed in a fixed order (no atomics: the same inputs give the same bits)
//   recon_loss_kernel       the same partials for a pred that is already in memory (forward_loss on its own)
#include "vit_host.hpp"

#include <math.h>

namespace osv {

typedef float f32x16d __attribute__((ext_vector_type(16)));

constexpr int DEC_MAX_LATENT = 1024;       // latent floats staged per image in dec_seed_kernel

// X[n][0] = W_embed . latent[n] + b_embed + dpos[0]; X[n][r] = noise + dpos[r] for r >= 1.  One workgroup per image: a wave per
// output column of the matvec (lanes over the latent, coalesced rows of W_embed), then 16-byte copies of the shared rows.
__global__ __launch_bounds__(256) void dec_seed_kernel(int L, int Dd, int De, const float *We, const float *be, const float *noise,
                                                       const float *dpos, const float *latent, float *X)
{
    __shared__ float lat[DEC_MAX_LATENT];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < De; k += 256) lat[k] = latent[(size_t)n * De + k];
    __syncthreads();
    float *x = X + (size_t)n * L * Dd;
    for (int c = wave; c < Dd; c += 4) {
        float s = 0.f;
        for (int k = lane; k < De; k += 64) s += We[(size_t)c * De + k] * lat[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) x[c] = s + be[c] + dpos[c];
    }
    const int n4 = (L - 1) * (Dd / 4);
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 p = *reinterpret_cast<const float4 *>(dpos + Dd + 4 * i);
        const float4 t = *reinterpret_cast<const float4 *>(noise + (4 * i) % Dd);
        *reinterpret_cast<float4 *>(x + Dd + 4 * i) = make_float4(p.x + t.x, p.y + t.y, p.z + t.z, p.w + t.w);
    }
}

struct PredArgs {
    uint32_t M;                 // N * (L - 1) patch rows
    int L, G, P, NP;            // tokens per image, patches per image side, patch side, P * P
    const float *X;             // [N * L][DD] residual stream behind the last block
    const float *lnw, *lnb;     // decoder_norm
    const float *Wp, *bias;     // decoder_pred packed by vit_pack_w_kernel (N = NP, K = DD), bias [NP]
    const float *images;        // [N][G P][G P] or null (no loss)
    float *pred;                // [N][L - 1][NP] or null
    float *recon;               // [N][G P][G P] or null
    double *partials;           // [gridDim.x] or null
};

constexpr int DP_BM = 64;       // patch rows per workgroup

__device__ __forceinline__ void dec_lds_dma16(const float *g, float *l) { __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0); }
template <int CTRL>
__device__ __forceinline__ float dec_dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// sum of a double over the workgroup's four waves in a fixed order -> thread 0
__device__ __forceinline__ double dec_block_sum(double v, double *wsum)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// Workgroup = 4 waves = 64 patch rows x all NP columns.  Tile row m is token row n L + 1 + p (n = m / (L - 1), p = m % (L - 1)):
// the gather happens in the DMA's source address, the tile is dense.  Rows are DD floats = DD / 4 16-byte slots, slot s of row r
// stored at slot s ^ (r & 7) (vit_gemm_kernel's swizzle: the fragment read of 32 rows at one column is 4-way conflicted, not
// 32-way).  LayerNorm: four threads per row over the stored tile, in place.  Product: wave w owns the 32-column chunks w, w + 4, ..
// for both 32-row blocks (32 accumulator registers), A fragments from LDS and W fragments from L2 through an 8-deep ring.
// Epilogue: in the accumulator layout a lane owns ONE column (chunk * 32 + li = pixel (py, px) of the patch) and 32 rows in
// ascending order, so the pixel address of its next row is the previous one + P per patch step + (P - 1) W at the end of a
// patch row (a frame boundary needs nothing more: G P = H) -- one division per lane and chunk, none per element.
template <int DD>
__global__ __launch_bounds__(256, DD == 128 ? 2 : 1) void dec_pred_kernel(const PredArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[DP_BM * DD];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const uint32_t row0 = blockIdx.x * DP_BM, np = (uint32_t)(a.L - 1);
    constexpr int SPR = DD / 4, RPI = 256 / SPR, NIT = DP_BM / RPI;      // slots per row, rows per DMA round, rounds
    {
        const int r_lo = threadIdx.x / SPR, slot = threadIdx.x % SPR;
        const uint32_t last_tok = a.M - 1 + (a.M - 1) / np + 1;
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int r = r_lo + RPI * i;
            const uint32_t m = row0 + r;
            uint32_t tok = m + m / np + 1;
            if (tok > last_tok) tok = last_tok;                           // rows past M: a valid row, never stored
            dec_lds_dma16(a.X + (size_t)tok * DD + 4 * (slot ^ (r & 7)), &As[(wave * 64 + 256 * i) * 4]);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    {
        // decoder_norm in place (two passes: mean, centred second moment; eps 1e-5)
        constexpr int SPQ = SPR / 4;
        const int row = threadIdx.x >> 2, qd = threadIdx.x & 3;
        float *rp = As + row * DD + qd * SPQ * 4;
        float4 v4[SPQ];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < SPQ; j++) { v4[j] = *reinterpret_cast<const float4 *>(rp + 4 * j); sum += (v4[j].x + v4[j].y) + (v4[j].z + v4[j].w); }
        sum += dec_dpp<0xB1>(sum); sum += dec_dpp<0x4E>(sum);
        const float mean = sum * (1.0f / DD);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < SPQ; j++) {
            v4[j].x -= mean; v4[j].y -= mean; v4[j].z -= mean; v4[j].w -= mean;
            q += (v4[j].x * v4[j].x + v4[j].y * v4[j].y) + (v4[j].z * v4[j].z + v4[j].w * v4[j].w);
        }
        q += dec_dpp<0xB1>(q); q += dec_dpp<0x4E>(q);
        const float rstd = rsqrtf(q * (1.0f / DD) + 1e-5f);
#pragma unroll
        for (int j = 0; j < SPQ; j++) {
            const int col = 4 * ((qd * SPQ + j) ^ (row & 7));
            const float4 w4 = *reinterpret_cast<const float4 *>(a.lnw + col), b4 = *reinterpret_cast<const float4 *>(a.lnb + col);
            float4 o;
            o.x = v4[j].x * rstd * w4.x + b4.x; o.y = v4[j].y * rstd * w4.y + b4.y;
            o.z = v4[j].z * rstd * w4.z + b4.z; o.w = v4[j].w * rstd * w4.w + b4.w;
            *reinterpret_cast<float4 *>(rp + 4 * j) = o;
        }
    }
    __syncthreads();
    int lo8[8];
#pragma unroll
    for (int j = 0; j < 8; j++) lo8[j] = li * DD + ((j ^ (li & 7)) << 2) + lh;
#define DEC_AFRAG(q, rb) As[lo8[((q) >> 1) & 7] + (rb) * 32 * DD + (((q) >> 1) >> 3) * 32 + ((q) & 1) * 2]
    const int nch = a.NP / 32, W = a.G * a.P;
    // (frame, patch) of the lane's first row
    const uint32_t m_first = row0 + 4 * lh, n_first = m_first / np, p_first = m_first % np;
    const uint32_t gx_first = p_first % (uint32_t)a.G, gy_first = p_first / (uint32_t)a.G;
    const size_t base_first = ((size_t)n_first * W + gy_first * a.P) * W + gx_first * a.P;
    double sq = 0.0;
    for (int c = wave; c < nch; c += 4) {
        constexpr int D8 = 8;
        f32x16d acc[2];
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[rb][e] = 0.f;
        const float *wq = a.Wp + (size_t)c * (DD / 2) * 64 + lane;
        float wbf[D8], abf[D8][2];
#pragma unroll
        for (int d = 0; d < D8; d++) {
            wbf[d] = wq[d * 64];
#pragma unroll
            for (int rb = 0; rb < 2; rb++) abf[d][rb] = DEC_AFRAG(d, rb);
        }
#pragma unroll
        for (int q = 0; q < DD / 2; q++) {
            const int d = q & (D8 - 1);
#pragma unroll
            for (int rb = 0; rb < 2; rb++) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(abf[d][rb], wbf[d], acc[rb], 0, 0, 0);
            if (q + D8 < DD / 2) {
                wbf[d] = wq[(q + D8) * 64];
#pragma unroll
                for (int rb = 0; rb < 2; rb++) abf[d][rb] = DEC_AFRAG(q + D8, rb);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const int col = c * 32 + li;
        const float bv = a.bias[col];
        const int pix = (col / a.P) * W + col % a.P;
        uint32_t gx = gx_first;
        size_t base = base_first;
        int prev = 0;
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int off = rb * 32 + (e & 3) + 8 * (e >> 2);
                for (int st = prev; st < off; st++) {
                    gx++; base += a.P;
                    if (gx == (uint32_t)a.G) { gx = 0; base += (size_t)(a.P - 1) * W; }
                }
                prev = off;
                const uint32_t m = m_first + off;
                if (m >= a.M) continue;
                const float v = acc[rb][e] + bv;
                if (a.pred) a.pred[(size_t)m * a.NP + col] = v;
                if (a.recon) a.recon[base + pix] = v;
                if (a.partials) { const float dlt = v - a.images[base + pix]; sq += (double)dlt * (double)dlt; }
            }
    }
#undef DEC_AFRAG
    if (a.partials) {
        __syncthreads();                                                  // every wave is done with the tile: its first bytes carry the sums
        const double t = dec_block_sum(sq, reinterpret_cast<double *>(As));
        if (threadIdx.x == 0) a.partials[blockIdx.x] = t;
    }
}

// squared error of pred [M][NP] against the pixels it stands for: a workgroup walks rows blockIdx.x, + gridDim.x, ..
__global__ __launch_bounds__(256) void recon_loss_kernel(uint32_t M, int L, int G, int P, int NP, const float *images, const float *pred,
                                                         double *partials)
{
    __shared__ double wsum[4];
    const uint32_t np = (uint32_t)(L - 1);
    const int W = G * P;
    double sq = 0.0;
    for (uint32_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint32_t n = m / np, p = m % np, gy = p / (uint32_t)G, gx = p % (uint32_t)G;
        const float *ib = images + ((size_t)n * W + gy * P) * W + gx * P, *pb = pred + (size_t)m * NP;
        for (int col = threadIdx.x; col < NP; col += 256) {
            const float dlt = pb[col] - ib[(col / P) * W + col % P];
            sq += (double)dlt * (double)dlt;
        }
    }
    const double t = dec_block_sum(sq, wsum);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// loss = (sum of the partials, in a fixed order) / count
__global__ __launch_bounds__(256) void dec_loss_finish_kernel(int n, const double *partials, double inv_count, float *loss)
{
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(sm[0] * inv_count);
}

}  // namespace osv

using namespace osv;

static size_t dec_block_floats(const VitDims &d)
{
    const size_t D = d.dim, Mh = d.mlp;
    return 2 * D + 3 * D * D + 3 * D + D * D + D + 2 * D + Mh * D + Mh + D * Mh + D;
}

static const char *dec_check_dims(const os_vit_dims *d, int latent_dim)
{
    if (d->embed_dim <= 0 || d->num_heads <= 0 || d->patch_size <= 0 || d->depth <= 0) return "os_vit_load_decoder: dimensions must be positive";
    if (d->embed_dim > 256 || d->embed_dim % d->num_heads || d->img_size % d->patch_size || d->in_chans != 1)
        return "os_vit_load_decoder: unsupported dimensions (decoder_embed_dim <= 256, one channel)";
    const int hd = d->embed_dim / d->num_heads;
    if (hd != 32 && hd != 64) return "os_vit_load_decoder: head dimension must be 32 or 64";
    if (d->embed_dim % 128 || d->mlp_hidden % 128) return "os_vit_load_decoder: decoder_embed_dim and mlp_hidden must be multiples of 128";
    if ((d->patch_size * d->patch_size * d->in_chans) % 32) return "os_vit_load_decoder: patch_size^2 * in_chans must be a multiple of 32";
    if (latent_dim <= 0 || latent_dim > DEC_MAX_LATENT) return "os_vit_load_decoder: latent_dim must be in 1 .. 1024";
    return nullptr;
}

void os_vit_decoder_destroy(os_vit_state *v)
{
    os_vit_dec_state *q = v->dec;
    if (!q) return;
    if (q->wp) (void)hipFree(q->wp);
    if (q->wpt) (void)hipFree(q->wpt);
    if (q->part) (void)hipFree(q->part);
    free(q);
    v->dec = nullptr;
}

// the decoder's loss partials -> *loss on stream s
static int dec_finish_loss(os_ctx *ctx, int nparts, const double *partials, double count, float *loss, hipStream_t s)
{
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_MISC, s, "dec_loss_finish_kernel");
    hipLaunchKernelGGL(dec_loss_finish_kernel, dim3(1), dim3(256), 0, s, nparts, partials, 1.0 / count, loss);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}

int os_vit_dec_seed(os_ctx *ctx, const os_vit_dec_state *q, int N, const float *latent, float *X, hipStream_t s)
{
    const int D = q->d.dim, L = ntok(q->d), De = q->latent_dim;
    const float *We = q->w, *be = We + (size_t)D * De, *noise = be + D, *dpos = noise + D;
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_MISC, s, "dec_seed_kernel");
    hipLaunchKernelGGL(dec_seed_kernel, dim3(N), dim3(256), 0, s, L, D, De, We, be, noise, dpos, latent, X);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}

// decoder_norm (flat cursor w) + decoder_pred over the patch rows of X, with the loss when asked for
int os_vit_dec_tail(os_ctx *ctx, os_vit_dec_state *q, int N, const float *w, const float *X, const float *images, float *pred,
                    float *recon, float *loss, hipStream_t s)
{
    const VitDims &d = q->d;
    const int D = d.dim, L = ntok(d), NP = d.patch * d.patch, Mh = d.mlp;
    const uint32_t Mp = (uint32_t)N * (L - 1);
    const int ntiles = (int)((Mp + DP_BM - 1) / DP_BM);
    if (loss && os_ensure_scratch(ctx, &q->part, &q->part_floats, (size_t)2 * ntiles)) return -10;
    PredArgs a;
    a.M = Mp; a.L = L; a.G = grid_of(d); a.P = d.patch; a.NP = NP; a.X = X;
    a.lnw = w; a.lnb = w + D; a.bias = w + 2 * D + (size_t)NP * D;
    a.Wp = q->wp + (size_t)d.depth * (3 * D * D + D * D + 2 * (size_t)Mh * D);
    a.images = loss ? images : nullptr; a.pred = pred; a.recon = recon; a.partials = loss ? (double *)q->part : nullptr;
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_GEMM, s, "dec_pred_kernel");
    if (D == 128) hipLaunchKernelGGL(dec_pred_kernel<128>, dim3(ntiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dec_pred_kernel<256>, dim3(ntiles), dim3(256), 0, s, a);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    if (loss) return dec_finish_loss(ctx, ntiles, a.partials, (double)Mp * NP, loss, s);
    return 0;
}

extern "C" {

size_t os_vit_decoder_param_count(const os_vit_dims *dec, int32_t latent_dim)
{
    const VitDims d{dec->img_size, dec->patch_size, dec->embed_dim, dec->depth, dec->num_heads, dec->mlp_hidden};
    const size_t D = d.dim, L = ntok(d), NP = (size_t)d.patch * d.patch * dec->in_chans;
    return D * latent_dim + D + D + L * D + (size_t)d.depth * dec_block_floats(d) + 2 * D + NP * D + NP;
}

int os_vit_load_decoder(os_ctx *ctx, const os_vit_dims *dec, int32_t latent_dim, const float *w_flat)
{
    OS_CHECK_CTX(ctx);
    if (!dec || !w_flat) return os_fail(ctx, -2, "os_vit_load_decoder: null pointer");
    if (const char *why = dec_check_dims(dec, latent_dim)) return os_fail(ctx, -4, why);
    OS_HIP(ctx, hipSetDevice(ctx->device));
    os_vit_state *v = os_vit_state_get(ctx);
    if (!v) return -13;
    os_vit_dec_state *q = v->dec;
    if (!q) {
        q = (os_vit_dec_state *)calloc(1, sizeof(os_vit_dec_state));
        if (!q) return os_fail(ctx, -13, "os_vit_load_decoder: out of memory");
        v->dec = q;
    }
    q->d = VitDims{dec->img_size, dec->patch_size, dec->embed_dim, dec->depth, dec->num_heads, dec->mlp_hidden};
    q->latent_dim = latent_dim;
    q->w = w_flat;
    q->wpt_valid = false;
    const size_t D = q->d.dim, L = ntok(q->d), Mh = q->d.mlp, NP = (size_t)q->d.patch * q->d.patch;
    const size_t total = (size_t)q->d.depth * (3 * D * D + D * D + 2 * Mh * D) + NP * D;
    if (os_ensure_scratch(ctx, &q->wp, &q->wp_floats, total)) return -10;
    const float *w = w_flat + D * latent_dim + D + D + L * D;
    float *o = q->wp;
    for (int blk = 0; blk < q->d.depth; blk++) {
        w += 2 * D;
        os_vit_pack_w((int)(3 * D), (int)D, w, o, 0); o += 3 * D * D; w += 3 * D * D + 3 * D;
        os_vit_pack_w((int)D, (int)D, w, o, 0); o += D * D; w += D * D + D;
        w += 2 * D;
        os_vit_pack_w((int)Mh, (int)D, w, o, 0); o += Mh * D; w += Mh * D + Mh;
        os_vit_pack_w((int)D, (int)Mh, w, o, 0); o += D * Mh; w += D * Mh + D;
    }
    w += 2 * D;
    os_vit_pack_w((int)NP, (int)D, w, o, 0);
    OS_HIP(ctx, hipGetLastError());
    OS_HIP(ctx, hipStreamSynchronize(0));
    return 0;
}

int os_vit_decode(os_ctx *ctx, int32_t N, const float *latent, const float *images, float *pred, float *recon, float *loss, void *stream)
{
    OS_CHECK_CTX(ctx);
    os_vit_state *v = (os_vit_state *)ctx->vit;
    os_vit_dec_state *q = v ? v->dec : nullptr;
    if (!q) return os_fail(ctx, -5, "os_vit_decode: call os_vit_load_decoder first");
    if (N <= 0 || !latent) return os_fail(ctx, -2, "os_vit_decode: bad argument");
    if (loss && !images) return os_fail(ctx, -2, "os_vit_decode: the loss needs the images");
    const VitDims &d = q->d;
    const int D = d.dim, L = ntok(d), Mh = d.mlp, De = q->latent_dim;
    if ((uint64_t)N * L >= (1ull << 31)) return os_fail(ctx, -2, "os_vit_decode: too many token rows for one call");
    OS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t M = (size_t)N * L;
    const size_t bigw = (size_t)(3 * D > Mh ? 3 * D : Mh);
    if (os_ensure_scratch(ctx, &v->buf, &v->buf_floats, M * D * 2 + M * bigw)) return -10;
    float *X = v->buf, *Y = X + M * D, *big = Y + M * D;
    if (int rc = os_vit_dec_seed(ctx, q, N, latent, X, s)) return rc;
    const float *w = q->w + (size_t)D * De + 2 * D + (size_t)L * D;
    if (int rc = os_vit_run_blocks(ctx, v, d, w, q->wp, X, Y, big, N, s, &w)) return rc;
    if (!pred && !recon && !loss) return 0;
    return os_vit_dec_tail(ctx, q, N, w, X, images, pred, recon, loss, s);
}

int os_vit_recon_loss(os_ctx *ctx, int32_t N, const float *images, const float *pred, float *loss, void *stream)
{
    OS_CHECK_CTX(ctx);
    os_vit_state *v = (os_vit_state *)ctx->vit;
    os_vit_dec_state *q = v ? v->dec : nullptr;
    if (!q) return os_fail(ctx, -5, "os_vit_recon_loss: call os_vit_load_decoder first");
    if (N <= 0 || !images || !pred || !loss) return os_fail(ctx, -2, "os_vit_recon_loss: bad argument");
    const VitDims &d = q->d;
    const int L = ntok(d), NP = d.patch * d.patch;
    if ((uint64_t)N * L >= (1ull << 31)) return os_fail(ctx, -2, "os_vit_recon_loss: too many token rows for one call");
    OS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t Mp = (uint32_t)N * (L - 1);
    const int nwg = Mp < 2048u ? (int)Mp : 2048;
    if (os_ensure_scratch(ctx, &q->part, &q->part_floats, (size_t)2 * nwg)) return -10;
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_MISC, s, "recon_loss_kernel");
    hipLaunchKernelGGL(recon_loss_kernel, dim3(nwg), dim3(256), 0, s, Mp, L, grid_of(d), d.patch, NP, images, pred, (double *)q->part);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return dec_finish_loss(ctx, nwg, (const double *)q->part, (double)Mp * NP, loss, s);
}

}  // extern "C"
