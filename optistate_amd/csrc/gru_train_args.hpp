// gru_train_args.hpp -- argument blocks of the GRU backward kernels shared by gru_train_kernels.hip (hidden sizes up to 128:
// resident / LDS-tile kernels) and gru_stream_kernels.hip (hidden sizes 160 .. 256: weight-streaming kernels).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ost {

struct SweepArgs {
    int B, T, K, H;
    int need_dx;                 // write dx (layer > 0 or caller wants d(input))
    const float *sv_r, *sv_z, *sv_n, *sv_g, *sv_h;   // [T][B][H]
    const float *dy;             // [T][B][H] gradient w.r.t. this layer's outputs, or null
    const float *dy_last;        // [B][H] gradient w.r.t. h_T only (top layer), or null
    const float *wihT, *whhT;    // transposed-packed weights
    float *dg4;                  // [T][B][4H]: da_r | da_z | da_n | da_n * r  (W_ih's products read sections 0-2, W_hh's 0, 1, 3)
    float *dx;                   // [T][B][K]
    // bwd_sweep_stack_kernel only (null otherwise): progress counters of the layer above (its dx is this layer's dy) and of this
    // workgroup; a counter holds the number of steps published, T - t after step t
    const uint32_t *flag_prev;
    uint32_t *flag_mine;
    int32_t *err = nullptr;      // the context's error word (launch.hpp): bit 0 = a bounded wait expired
    int32_t *err_local = nullptr;    // its twin in device memory
    uint32_t max_polls = 1u << 22;
    int drop_from = -1;          // tests (OS_STACK_DBG_DROP): stop publishing once T - 1 - t reaches this count of steps done
};

struct DwArgs {
    int H3, K;                // gate units, input width
    size_t r_begin, r_end;    // rows of dG to reduce (row r of dG pairs with row r - x_row_shift of X)
    size_t x_row_shift;
    size_t x_valid_from;      // dw2_kernel, dw_stream_kernel: rows below this pair with X = 0 (h_{-1}): they only count for the bias sum
                              // (dw2_kernel: a multiple of 32)
    int rows_per_slice;
    const float *dG;          // [rows][ldg]: gate unit j sits in column j (+ nshift for the n gate, j >= 2 H3 / 3)
    int ldg, nshift;          // the sweep's four-section array: ldg = 4H; nshift = 0 for W_ih (da_n), H for W_hh (da_n * r)
    const float *X;           // [rows][K], or (B, T, K) batch_first when x_btf (row r = t*B + b lives at (b*T + t)*K)
    int x_btf, B, T;
    float *dW;                // [H3][K]
    float *db;                // [H3] or null
};

}  // namespace ost
