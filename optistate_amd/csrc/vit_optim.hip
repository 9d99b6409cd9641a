// vit_optim.hip -- the optimiser step of the ViT auto-encoder (transformer/autoencoder_training.py:96,113: torch.optim.AdamW over
// timm's two decay groups) as ONE launch that also keeps every packed copy of the weights current.
//
// The GEMMs of forward and backward do not read the flat weight vectors: vit_gemm_kernel streams W in B-fragment order
// (vit_pack_w_kernel), and the input-gradient GEMMs stream W^T in the same order (vit_pack_wt_kernel).  An optimiser that updates
// only the flat vectors leaves about fifty re-pack launches per step behind it.  vit_adamw_pack_kernel updates a tile of a matrix in
// registers and writes the new values three times: back to the flat vector, into the forward pack and into the transposed pack.
//
// Work table: one entry per workgroup, built on the host from the two VitDims and kept on the device (it holds offsets only, so it
// survives a reload of the same model).
//   matrix tile   32 rows x 128 columns of a [N][K] matrix that the GEMMs read packed.  256 threads read w, g, m, v as 16-byte row
//                 segments (a row of the tile = 32 lanes = 512 contiguous bytes), update, store w, m, v the same way and park the new
//                 w in LDS as T[32][OPT_PITCH].  Behind one barrier the tile is read out twice, every wave instruction filling one
//                 whole 256-byte run of the destination:
//                   forward     wp[(c K/2 + q) 64 + lane]    = W[32 c + (lane & 31)][2 q + (lane >> 5)]: c = row0 / 32 and the 64 q of
//                               the tile's columns are consecutive -- one 16 KB run; wave w writes q = w, w + 4, ...
//                   transposed  wpt[(c' N/2 + q') 64 + lane] = W[2 q' + (lane >> 5)][32 c' + (lane & 31)]: four c' (wave w takes
//                               c' = k0 / 32 + w) times the 16 q' of the tile's rows -- four 4 KB runs
//                 OPT_PITCH = 132 floats: a multiple of four, so the 16-byte stores into T stay aligned, and = 4 mod 64, so over the
//                 64 four-byte banks the forward read-out (lane -> row lane & 31, the wave halves one column apart) puts rows r and
//                 r + 16 on one bank and nothing else, and the transposed read-out (lane -> column, the wave halves one row = 4 banks
//                 apart) overlaps only the two halves: both 2-way.  A pitch = 32 mod 64 would free the transposed read-out and make
//                 the forward one 32-way; an odd pitch would cost the 16-byte stores.
//   flat span     at most 4,096 contiguous elements that nothing reads packed: biases, LayerNorm affines, cls_token,
//                 decoder_noise_token and decoder_embed.weight (dec_seed_kernel and its backward read it flat).  Neighbouring
//                 tensors with the same decay flag share spans.
// The position tables have no entry: their weights, m and v are neither read nor written, whatever the gradient vectors hold there.
// Scalar fp32 only (build.py compiles this file without the packed-fp32 VALU forms); division and square root are the correctly
// rounded ones.  No atomics: the step is a pure function of its inputs.
#include "vit_host.hpp"

#include <math.h>
#include <string.h>

#include <vector>

namespace osv {

constexpr int OPT_ROWS = 32, OPT_COLS = 128, OPT_PITCH = 132, OPT_SPAN = 4096;
constexpr uint32_t OPT_DEC = 1, OPT_DECAY = 2, OPT_TILE = 4, OPT_WPT = 8;

struct OptEntry {
    uint32_t flags;             // OPT_DEC: the decoder's vectors; OPT_DECAY; OPT_TILE: matrix tile, else flat span; OPT_WPT: has a transposed pack
    uint32_t off;               // flat offset of the tensor (tile) / of the span
    uint32_t n;                 // tile: N (rows of the matrix); span: its length, a multiple of 4
    uint32_t K, row0, k0;       // tile
    uint32_t wp_off, wpt_off;   // tile: the matrix's offset in the forward / transposed pack buffer
};

struct OptArgs {
    float *w0, *w1;             // 0: encoder, 1: decoder
    const float *g0, *g1;
    float *m0, *m1, *v0, *v1;
    float *wp0, *wp1, *wpt0, *wpt1;
    const OptEntry *table;
    float decay;                // 1 - lr * weight_decay
    float b1, omb1, b2, omb2;   // beta, 1 - beta
    float step_size;            // lr / (1 - beta1^t)
    float inv_sqrt_bc2;         // 1 / sqrt(1 - beta2^t)
    float eps;
};

__device__ __forceinline__ float adamw1(float w, float g, float &m, float &v, const OptArgs &a, float decay)
{
    w *= decay;
    m = a.b1 * m + a.omb1 * g;
    v = a.b2 * v + a.omb2 * g * g;
    return w - a.step_size * (m / (sqrtf(v) * a.inv_sqrt_bc2 + a.eps));
}

// w, m, v at element i .. i + 3 of their vectors (16-byte aligned) updated in place; returns the new w
__device__ __forceinline__ float4 adamw4(float *w, const float *g, float *m, float *v, size_t i, const OptArgs &a, float decay)
{
    float4 wv = *reinterpret_cast<const float4 *>(w + i), mv = *reinterpret_cast<const float4 *>(m + i);
    float4 vv = *reinterpret_cast<const float4 *>(v + i);
    const float4 gv = *reinterpret_cast<const float4 *>(g + i);
    wv.x = adamw1(wv.x, gv.x, mv.x, vv.x, a, decay);
    wv.y = adamw1(wv.y, gv.y, mv.y, vv.y, a, decay);
    wv.z = adamw1(wv.z, gv.z, mv.z, vv.z, a, decay);
    wv.w = adamw1(wv.w, gv.w, mv.w, vv.w, a, decay);
    *reinterpret_cast<float4 *>(w + i) = wv;
    *reinterpret_cast<float4 *>(m + i) = mv;
    *reinterpret_cast<float4 *>(v + i) = vv;
    return wv;
}

__global__ __launch_bounds__(256) void vit_adamw_pack_kernel(const OptArgs a)
{
    __shared__ __attribute__((aligned(16))) float T[OPT_ROWS * OPT_PITCH];
    const OptEntry e = a.table[blockIdx.x];
    const bool dec = e.flags & OPT_DEC;
    float *w = dec ? a.w1 : a.w0, *m = dec ? a.m1 : a.m0, *v = dec ? a.v1 : a.v0;
    const float *g = dec ? a.g1 : a.g0;
    const float decay = (e.flags & OPT_DECAY) ? a.decay : 1.0f;
    if (!(e.flags & OPT_TILE)) {
#pragma unroll
        for (int i = 0; i < OPT_SPAN / 1024; i++) {
            const uint32_t p = (threadIdx.x + 256 * i) * 4;
            if (p < e.n) adamw4(w, g, m, v, (size_t)e.off + p, a, decay);
        }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const size_t base = (size_t)e.off + (size_t)e.row0 * e.K + e.k0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int p = threadIdx.x + 256 * i, r = p >> 5, c4 = (p & 31) * 4;
        *reinterpret_cast<float4 *>(&T[r * OPT_PITCH + c4]) = adamw4(w, g, m, v, base + (size_t)r * e.K + c4, a, decay);
    }
    __syncthreads();
    float *wp = (dec ? a.wp1 : a.wp0) + e.wp_off + ((size_t)(e.row0 / 32) * (e.K / 2) + e.k0 / 2) * 64;
#pragma unroll 4
    for (int q = wave; q < OPT_COLS / 2; q += 4) wp[q * 64 + lane] = T[li * OPT_PITCH + 2 * q + lh];
    if (e.flags & OPT_WPT) {
        float *wpt = (dec ? a.wpt1 : a.wpt0) + e.wpt_off + ((size_t)(e.k0 / 32 + wave) * (e.n / 2) + e.row0 / 2) * 64;
#pragma unroll 4
        for (int q = 0; q < OPT_ROWS / 2; q++) wpt[q * 64 + lane] = T[(2 * q + lh) * OPT_PITCH + 32 * wave + li];
    }
}

}  // namespace osv

using namespace osv;

namespace {

// The table of one vector, appended to t.  Tensors are visited in flat order; neighbouring flat tensors with one decay flag merge.
struct TableBuilder {
    std::vector<OptEntry> &t;
    uint32_t which;             // 0 | OPT_DEC
    size_t off = 0, wp = 0, wpt = 0;
    size_t span_off = 0, span_len = 0;
    uint32_t span_decay = 0;

    void flush()
    {
        for (size_t o = 0; o < span_len; o += OPT_SPAN) {
            OptEntry e{};
            e.flags = which | span_decay;
            e.off = (uint32_t)(span_off + o);
            e.n = (uint32_t)(span_len - o < OPT_SPAN ? span_len - o : OPT_SPAN);
            t.push_back(e);
        }
        span_len = 0;
    }
    void flat(size_t n, bool decay)
    {
        const uint32_t f = decay ? OPT_DECAY : 0;
        if (span_len && f != span_decay) flush();
        if (!span_len) { span_off = off; span_decay = f; }
        span_len += n;
        off += n;
    }
    void skip(size_t n) { flush(); off += n; }
    // a packed [N][K] matrix, always decayed; its forward pack is the next one in wp, its transposed pack (if any) the next in wpt
    void matrix(size_t N, size_t K, bool transposed)
    {
        flush();
        for (size_t r = 0; r < N; r += OPT_ROWS)
            for (size_t k = 0; k < K; k += OPT_COLS) {
                OptEntry e{};
                e.flags = which | OPT_DECAY | OPT_TILE | (transposed ? OPT_WPT : 0);
                e.off = (uint32_t)off; e.n = (uint32_t)N; e.K = (uint32_t)K; e.row0 = (uint32_t)r; e.k0 = (uint32_t)k;
                e.wp_off = (uint32_t)wp; e.wpt_off = (uint32_t)wpt;
                t.push_back(e);
            }
        off += N * K; wp += N * K;
        if (transposed) wpt += N * K;
    }
    void blocks(const VitDims &d)
    {
        const size_t D = d.dim, Mh = d.mlp;
        for (int b = 0; b < d.depth; b++) {
            flat(2 * D, false);                              // norm1
            matrix(3 * D, D, true); flat(3 * D, false);      // attn.qkv
            matrix(D, D, true); flat(D, false);              // attn.proj
            flat(2 * D, false);                              // norm2
            matrix(Mh, D, true); flat(Mh, false);            // mlp.fc1
            matrix(D, Mh, true); flat(D, false);             // mlp.fc2
        }
    }
};

size_t stack_pack_floats(const VitDims &d) { return (size_t)d.depth * (4 * (size_t)d.dim * d.dim + 2 * (size_t)d.mlp * d.dim); }

bool same_dims(const VitDims &a, const VitDims &b) { return memcmp(&a, &b, sizeof(VitDims)) == 0; }

// the work table for the loaded pair, on the device; rebuilt only when the dimensions changed (behind a device synchronise)
int ensure_table(os_ctx *ctx, os_vit_state *v)
{
    os_vit_dec_state *q = v->dec;
    const VitDims &e = v->d, &dd = q->d;
    if (v->opt_table && v->opt_entries && same_dims(v->opt_enc, e) && same_dims(v->opt_dec, dd) && v->opt_latent == q->latent_dim) return 0;
    std::vector<OptEntry> t;
    const size_t D = e.dim, PP = (size_t)e.patch * e.patch, L = ntok(e), Dd = dd.dim, NP = (size_t)dd.patch * dd.patch;
    TableBuilder be{t, 0};
    be.matrix(D, PP, false);                                 // patch_embed.proj.weight: only dW reaches it in the backward
    be.flat(D, false);                                       // patch_embed.proj.bias
    be.flat(D, true);                                        // cls_token (1, 1, D): decayed
    be.skip(L * D);                                          // pos_embed: fixed
    be.blocks(e);
    be.flat(2 * D, false);                                   // norm
    be.flush();
    TableBuilder bd{t, OPT_DEC};
    bd.flat(Dd * (size_t)q->latent_dim, true);               // decoder_embed.weight: read flat
    bd.flat(Dd, false);                                      // decoder_embed.bias
    bd.flat(Dd, true);                                       // decoder_noise_token
    bd.skip(L * Dd);                                         // decoder_pos_embed: fixed
    bd.blocks(dd);
    bd.flat(2 * Dd, false);                                  // decoder_norm
    bd.matrix(NP, Dd, true); bd.flat(NP, false);             // decoder_pred
    bd.flush();
    // what the kernel will address lies inside the buffers of this load (the tiling needs N % 32 == 0 and K % 128 == 0)
    const size_t wpt_e = stack_pack_floats(e), wpt_d = stack_pack_floats(dd) + NP * Dd;
    bool ok = be.wp <= v->wp_floats && bd.wp <= q->wp_floats && be.wpt == wpt_e && bd.wpt == wpt_d && be.off < (1ull << 32) && bd.off < (1ull << 32);
    for (const OptEntry &x : t)
        if (x.flags & OPT_TILE) ok = ok && x.n % OPT_ROWS == 0 && x.K % OPT_COLS == 0;
        else ok = ok && x.n % 4 == 0 && x.off % 4 == 0 && x.n <= OPT_SPAN;
    if (!ok) return os_fail(ctx, -4, "os_vit_adamw_step: the loaded dimensions do not tile (rows % 32, columns % 128)");
    if (os_ensure_scratch(ctx, &v->wpt, &v->wpt_floats, wpt_e)) return -10;
    if (os_ensure_scratch(ctx, &q->wpt, &q->wpt_floats, wpt_d)) return -10;
    if (v->opt_cap < t.size()) {
        if (v->opt_table) OS_HIP(ctx, hipFree(v->opt_table));
        v->opt_table = nullptr; v->opt_cap = 0; v->opt_entries = 0;
        OS_HIP(ctx, hipMalloc(&v->opt_table, t.size() * sizeof(OptEntry)));
        v->opt_cap = t.size();
    }
    OS_HIP(ctx, hipDeviceSynchronize());                     // a step of the previous dimensions may still be reading the table
    OS_HIP(ctx, hipMemcpy(v->opt_table, t.data(), t.size() * sizeof(OptEntry), hipMemcpyHostToDevice));
    v->opt_entries = t.size();
    v->opt_enc = e; v->opt_dec = dd; v->opt_latent = q->latent_dim;
    return 0;
}

}  // namespace

extern "C" {

int os_vit_adamw_step(os_ctx *ctx, float *w_enc, float *w_dec, const float *g_enc, const float *g_dec, float *m_enc, float *v_enc,
                      float *m_dec, float *v_dec, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                      void *stream)
{
    OS_CHECK_CTX(ctx);
    if (!w_enc || !w_dec || !g_enc || !g_dec || !m_enc || !v_enc || !m_dec || !v_dec) return os_fail(ctx, -2, "os_vit_adamw_step: null pointer");
    if (step < 1) return os_fail(ctx, -2, "os_vit_adamw_step: step counts from 1");
    const void *ptrs[] = {w_enc, w_dec, g_enc, g_dec, m_enc, v_enc, m_dec, v_dec};
    for (const void *p : ptrs)
        if ((uintptr_t)p % 16) return os_fail(ctx, -2, "os_vit_adamw_step: every vector must be 16-byte aligned");
    os_vit_state *v = (os_vit_state *)ctx->vit;
    if (!v || !v->w || !v->dec) return os_fail(ctx, -5, "os_vit_adamw_step: call os_vit_load and os_vit_load_decoder first");
    if (w_enc != v->w || w_dec != v->dec->w)
        return os_fail(ctx, -5, "os_vit_adamw_step: w_enc / w_dec are not the vectors the context has loaded (the step rewrites their packed copies)");
    OS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_table(ctx, v)) return rc;
    os_vit_dec_state *q = v->dec;
    OptArgs a;
    a.w0 = w_enc; a.w1 = w_dec; a.g0 = g_enc; a.g1 = g_dec; a.m0 = m_enc; a.m1 = m_dec; a.v0 = v_enc; a.v1 = v_dec;
    a.wp0 = v->wp; a.wp1 = q->wp; a.wpt0 = v->wpt; a.wpt1 = q->wpt;
    a.table = (const OptEntry *)v->opt_table;
    a.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    a.b1 = beta1; a.omb1 = (float)(1.0 - (double)beta1); a.b2 = beta2; a.omb2 = (float)(1.0 - (double)beta2);
    a.step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)));
    a.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    a.eps = eps;
    hipStream_t s = (hipStream_t)stream;
    const int slot = os_prof_begin(ctx, OS_PHASE_TRAIN_MISC, s, "vit_adamw_pack_kernel");
    hipLaunchKernelGGL(vit_adamw_pack_kernel, dim3((unsigned)v->opt_entries), dim3(256), 0, s, a);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    v->wpt_valid = true; q->wpt_valid = true;                // stream-ordered: a backward behind this launch reads what it wrote
    return 0;
}

}  // extern "C"
