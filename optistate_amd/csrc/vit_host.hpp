// vit_host.hpp -- host-side state and entry points that the ViT encoder (vit_kernels.hip), decoder (vit_decoder.hip) and training
// step (vit_train.hip, vit_optim.hip) share.
#pragma once
#include "launch.hpp"

namespace osv {

struct VitDims { int img, patch, dim, depth, heads, mlp; };

__host__ __device__ inline int grid_of(const VitDims &d) { return d.img / d.patch; }
__host__ __device__ inline int ntok(const VitDims &d) { return grid_of(d) * grid_of(d) + 1; }

// arguments of vit_gemm_kernel (vit_kernels.hip, where SRC and EPI are described)
struct GemmArgs {
    size_t M;
    int N, K, lda;
    const float *A;            // SRC 0
    const float *img;          // SRC 1: [frames][img][img]
    int img_size, grid, patch; // SRC 1
    const float *Wp;           // packed weights
    const float *bias;         // [N] (not EPI 7)
    float *C;                  // EPI 0/1/4/5/7: [M][N]; EPI 2/3: the token matrix X
    const float *pos;          // EPI 3: [L][N]
    int L;                     // EPI 3
    const float *R;            // EPI 4: residual [M][N] read beside C
    float *C2;                 // EPI 5: gelu(C) [M][N]
};

}  // namespace osv

struct os_vit_dec_state {
    osv::VitDims d;          // dim / depth / heads / mlp are the decoder's
    int latent_dim;
    const float *w;          // caller-owned flat weights
    float *wp; size_t wp_floats;       // per block qkv, proj, fc1, fc2, then decoder_pred, in B-fragment order
    float *part; size_t part_floats;   // float64 loss partials
    float *wpt; size_t wpt_floats;     // the same matrices transposed (vit_pack_wt_kernel's order), written by vit_adamw_pack_kernel
    bool wpt_valid;                    // wpt holds the transposes of w's current values (cleared by every load)
};

struct os_vit_state {
    osv::VitDims d;
    const float *w;          // caller-owned flat weights (null until os_vit_load)
    float *wp; size_t wp_floats;       // every projection matrix re-packed into B-fragment order (vit_pack_w_kernel)
    float *buf; size_t buf_floats;     // X | Y | big of the call in flight (encoder and decoder take turns on the stream)
    bool att_attr_set, mlp_attr_set, att_bwd_attr_set;
    os_vit_dec_state *dec;   // created by os_vit_load_decoder
    float *tbuf; size_t tbuf_floats;   // os_vit_backward's scratch (vit_train.hip)
    float *wpt; size_t wpt_floats;     // per block qkv, proj, fc1, fc2 transposed (the patch embedding's transpose is never read)
    bool wpt_valid;                    // as in os_vit_dec_state
    void *opt_table; size_t opt_entries, opt_cap;   // vit_adamw_pack_kernel's work table on the device (vit_optim.hip)
    osv::VitDims opt_enc, opt_dec; int opt_latent;  // the dimensions it was built for
};

// the context's ViT state, created empty on first use (null: out of memory, message set)
os_vit_state *os_vit_state_get(os_ctx *ctx);
// W [N][K] -> B-fragment order (vit_pack_w_kernel) on stream s
void os_vit_pack_w(int N, int K, const float *W, float *dst, hipStream_t s);
// The transformer blocks of d over the token matrix X [N * ntok(d)][d.dim] in place.  w: flat cursor at block 0's norm1.weight,
// wp: packed cursor at block 0's qkv matrix; *w_end receives the flat cursor behind the last block.  Y [M][dim] and
// big [M][max(3 dim, mlp)] are scratch.
int os_vit_run_blocks(os_ctx *ctx, os_vit_state *v, const osv::VitDims &d, const float *w, const float *wp, float *X, float *Y,
                      float *big, int N, hipStream_t s, const float **w_end);
void os_vit_decoder_destroy(os_vit_state *v);

// ---- single launches of the forward kernels, for callers outside their translation unit (the training forward) ----
void os_vit_launch_layernorm(os_ctx *ctx, size_t M, int D, const float *X, const float *w, const float *b, float *Y, hipStream_t s);
// vit_gemm_kernel<src, epi>: (0, 0), (0, 4), (0, 5), (0, 7) and (1, 3)
int os_vit_launch_gemm(os_ctx *ctx, int src, int epi, const osv::GemmArgs &g, hipStream_t s, const char *name);
// attention of every (image, head): QKV [N * L][3 dim] -> O [N * L][dim]
int os_vit_launch_attention(os_ctx *ctx, os_vit_state *v, const osv::VitDims &d, int N, const float *QKV, const float *qkvb, float *O,
                            hipStream_t s);
// the key-tiled kernels (vit_attn_tiled.hip): head dimension 32 or 64, any token count.  lse [N][heads][L]: the log-sum-exp of the
// scaled logits in units of log 2 (null: not written); delta [N][heads][L]: scratch that the backward fills and reads.  dQKV in
// the layout of QKV.
int os_vit_launch_attention_tiled(os_ctx *ctx, const osv::VitDims &d, int N, const float *QKV, float *O, float *lse, hipStream_t s,
                                  const char *name);
int os_vit_launch_attention_tiled_bwd(os_ctx *ctx, const osv::VitDims &d, int N, const float *QKV, const float *O, const float *dO,
                                      const float *lse, float *delta, float *dQKV, hipStream_t s);
void os_vit_launch_cls_row(os_ctx *ctx, int N, int L, int D, const float *cls, const float *pos, float *X, hipStream_t s);
void os_vit_launch_cls_head(os_ctx *ctx, int N, int L, int D, const float *X, const float *w, const float *b, float *latent, hipStream_t s);
// the decoder's two ends (vit_decoder.hip): latent -> token matrix X; X behind the last block -> pred / recon / loss
int os_vit_dec_seed(os_ctx *ctx, const os_vit_dec_state *q, int N, const float *latent, float *X, hipStream_t s);
int os_vit_dec_tail(os_ctx *ctx, os_vit_dec_state *q, int N, const float *w_norm, const float *X, const float *images, float *pred,
                    float *recon, float *loss, hipStream_t s);
