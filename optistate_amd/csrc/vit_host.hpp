// vit_host.hpp -- host-side state and entry points that the ViT encoder (vit_kernels.hip) and decoder (vit_decoder.hip) share.
#pragma once
#include "launch.hpp"

namespace osv {

struct VitDims { int img, patch, dim, depth, heads, mlp; };

__host__ __device__ inline int grid_of(const VitDims &d) { return d.img / d.patch; }
__host__ __device__ inline int ntok(const VitDims &d) { return grid_of(d) * grid_of(d) + 1; }

}  // namespace osv

struct os_vit_dec_state;     // vit_decoder.hip

struct os_vit_state {
    osv::VitDims d;
    const float *w;          // caller-owned flat weights (null until os_vit_load)
    float *wp; size_t wp_floats;       // every projection matrix re-packed into B-fragment order (vit_pack_w_kernel)
    float *buf; size_t buf_floats;     // X | Y | big of the call in flight (encoder and decoder take turns on the stream)
    bool att_attr_set, mlp_attr_set;
    os_vit_dec_state *dec;   // created by os_vit_load_decoder
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
