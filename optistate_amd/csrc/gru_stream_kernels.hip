// gru_stream_kernels.hip -- GRU layers with hidden sizes 160, 192, 224 and 256 on gfx950: weight-STREAMING kernels.
//
// Every other GRU kernel of the library keeps a wavefront's weight slice in registers and stops at H = 128: at H = 256 one
// 32-unit chunk's slice is 96 x (K + H) floats, eight of them do not fit a compute unit's register file.  Here the weights stay
// in global memory (about 1.5 MB per layer at K = H = 256: every workgroup reads the same image, so it lives in L2 / MALL) and are
// read as MFMA B operands in every time step; what is resident is the A side.  Exact fp32 on v_mfma_f32_32x32x2_f32 like the
// rest of the GRU path.  No workgroup ever waits for another: no progress counters, no spin loops, no atomics -- a plain launch
// per layer, and gradients that do not depend on the order workgroups retire in.
//
//   gru_stream_layer_kernel<RBW>  forward (inference and training): 8 waves, one per 32-unit chunk (run-time chunk count 5 .. 8),
//                                 a tile of 32 RBW rows; [x_t | h_{t-1}] k-major in LDS, r / z / n / gh_n accumulators in registers;
//                                 the fragment image of os_gru_load as it is (a chunk's W_ih and W_hh fragments are contiguous)
//   bwd_sweep_stream_kernel       backward sweep: 8 waves, wave c owns hidden chunk c -- its slice of dh lives in the MFMA
//                                 accumulator for the whole launch, only the 4H-wide gate-derivative tile is in LDS (131 KB at 256)
//   dw_stream_kernel              weight gradients: 128 x 128 tiles of dW per workgroup over a slice of rows, plain stores into
//                                 per-slice partial images, summed in slice order by dw_stream_reduce_kernel
#include "launch.hpp"

#include "gru_common.hpp"
#include "kf_device.hpp"        // buffer addressing helpers
#include "gru_device.hpp"       // gru_cell_pair
#include "gru_train_args.hpp"   // SweepArgs, DwArgs

namespace osg {

using osk::buf_load;
using osk::make_rsrc;
using osk::rsrc_t;

constexpr int STREAM_NT = 512;          // threads per workgroup of the layer and sweep kernels (eight waves)
constexpr int STREAM_KMAX = 256;        // widest input (and hidden state) the LDS tile holds
constexpr int STREAM_D = 4;             // k-pairs of weight / A fragments in flight per wave

// One part of the gate GEMM: KP k-pairs of this wave's chunk, starting at k-pair wq0 of its fragment stream (768 bytes per k-pair:
// gates r, z, n x 64 lanes).  ap: this lane's A element of k-pair 0, row block 0 in the k-major LDS tile (pitch BMS floats per k).
// GN: accumulator of the n gate (2: gi_n of the input part, 3: gh_n of the recurrent part).  Software pipeline STREAM_D k-pairs
// deep: the fragments of k-pair q + D are requested right behind the MFMAs of k-pair q, so D x 3 x RBW MFMAs cover an L2 round
// trip.  The steady-state loop has no conditional (a guarded request makes hipcc's wait-count pass drain the whole queue).
template <int RBW, int GN>
__device__ __forceinline__ void stream_part(f32x16 (*acc)[4], rsrc_t w, uint32_t wl, uint32_t wq0, const float *ap, int BMS, int KP)
{
    constexpr int D = STREAM_D;
    float wb[D][3], ab[D][RBW];
    auto request = [&](int j, int q) {
        const uint32_t so = __builtin_amdgcn_readfirstlane((wq0 + (uint32_t)q) * 768u);
#pragma unroll
        for (int g = 0; g < 3; g++) wb[j][g] = buf_load(w, wl, so + (uint32_t)g * 256u);
#pragma unroll
        for (int rb = 0; rb < RBW; rb++) ab[j][rb] = ap[2 * q * BMS + rb * 32];
    };
    auto fire = [&](int j) {
#pragma unroll
        for (int rb = 0; rb < RBW; rb++) {
            const float av = ab[j][rb];
            acc[rb][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wb[j][0], acc[rb][0], 0, 0, 0);
            acc[rb][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wb[j][1], acc[rb][1], 0, 0, 0);
            acc[rb][GN] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wb[j][2], acc[rb][GN], 0, 0, 0);
        }
    };
    int q0 = 0;
    if (KP >= 2 * D) {
#pragma unroll
        for (int j = 0; j < D; j++) {
            request(j, j);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; q0 + 2 * D <= KP; q0 += D) {
#pragma unroll
            for (int j = 0; j < D; j++) {
                fire(j);
                request(j, q0 + j + D);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; j++)
            if (j < KP) request(j, j);
    }
    // tail: the last D .. 2 D - 1 k-pairs, requests guarded
    for (; q0 < KP; q0 += D) {
#pragma unroll
        for (int j = 0; j < D; j++) {
            const int q = q0 + j;
            if (q < KP) {
                fire(j);
                if (q + D < KP) request(j, q + D);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// RBW = 32-row blocks per workgroup (BM = 32 RBW rows): every weight fragment a wave loads feeds 3 RBW MFMAs, so the L2 read
// rate per MFMA halves from RBW = 1 to 2 (K = H = 256: 1.5 MB per step and workgroup either way).
// LDS: A [2 KPx + H][BM + 1], k-major: rows 0 .. 2 KPx - 1 hold x_t (the pad row of an odd K is zero, like its weights), the rest
// h_{t-1}.  Lane li of an A fragment reads row li of one k: consecutive words; the cell update writes unit li of one row: pitch
// BM + 1, odd.  133 KB at K = H = 256, RBW = 2.  Single-buffered, two barriers per step:
//   SoA write-back of h_{t-1} | loads of x_{t+1} into registers | MFMAs | cell update (h_t kept in the accumulator registers,
//   saved activations stored) | barrier: every wave is done reading the tile | h_t and x_{t+1} into the tile | barrier
template <int RBW>
__global__ __launch_bounds__(STREAM_NT, 1) void gru_stream_layer_kernel(const LayerArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float As[];
    constexpr int BM = 32 * RBW, BMS = BM + 1, XPT = STREAM_KMAX * BM / STREAM_NT;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const int H = a.H, K = a.K, NCH = H >> 5, KP2 = 2 * a.KPx;
    const int tile_row0 = blockIdx.x * BM;
    const size_t B = (size_t)a.B;
    float *xS = As, *hS = As + KP2 * BMS;
    for (int i = threadIdx.x; i < H * BMS; i += STREAM_NT) hS[i] = 0.f;      // h0 = 0 (gru/gru_model.py:27)

    const bool work = wave < NCH;                    // H = 160 .. 224: the last waves only help with staging and write-back
    const int chunk = work ? wave : 0;
    const float *wc = a.w + (size_t)chunk * chunk_floats(a.KPx, a.KPh);
    const rsrc_t rw = make_rsrc(wc, (uint32_t)(a.KPx + a.KPh) * 768u);
    const uint32_t wl = (uint32_t)lane * 4u;
    const float *bias = wc + (size_t)(a.KPx + a.KPh) * 192;
    constexpr float LOG2E = 1.44269504088896341f;
    const float nb_r = -LOG2E * bias[li], nb_z = -LOG2E * bias[32 + li], nb_n = 2.0f * LOG2E * bias[64 + li], b_hn = bias[96 + li];

    // x tile of a step through registers: thread = (row xrow, inputs xk0 + j KSTEP) -- coalesced rows of the SoA stream.  One
    // per-lane offset for all of a thread's loads, the input in a wave-uniform offset; what must read zero (rows past the batch,
    // the pad row of an odd K) gets an offset no descriptor covers.
    auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
    constexpr int KSTEP = STREAM_NT / BM;
    const int xk0 = threadIdx.x / BM, xrow = threadIdx.x % BM;
    const uint32_t rowB = (uint32_t)a.B * 4u;
    const uint32_t xv0 = tile_row0 + xrow < a.B ? ((uint32_t)xk0 * (uint32_t)a.B + (uint32_t)(tile_row0 + xrow)) * 4u : 0x80000000u;
    float xst[XPT];
    auto x_load = [&](int t) {
        const rsrc_t rx = make_rsrc(a.xs + (size_t)t * K * B, (uint32_t)K * rowB);
#pragma unroll
        for (int j = 0; j < XPT; j++)
            xst[j] = buf_load(rx, xk0 + j * KSTEP < K ? xv0 : 0x80000000u, __builtin_amdgcn_readfirstlane((uint32_t)(j * KSTEP) * rowB));
    };
    auto x_store = [&]() {
#pragma unroll
        for (int j = 0; j < XPT; j++)
            if (xk0 + j * KSTEP < KP2) xS[(xk0 + j * KSTEP) * BMS + xrow] = xst[j];
    };
    // cooperative, coalesced write-back of the h tile in SoA ([H][B] block at dst)
    auto write_back = [&](float *dst) {
        for (int i = threadIdx.x; i < BM * H; i += STREAM_NT) {
            const int row = i % BM, k = i / BM, g = tile_row0 + row;
            if (g < a.B) dst[(size_t)k * B + g] = hS[k * BMS + row];
        }
    };
    x_load(0);
    x_store();
    __syncthreads();

    for (int t = 0; t < a.T; t++) {
        if (t > 0 && a.seq_out) write_back(a.seq_out + (size_t)(t - 1) * H * B);
        if (t + 1 < a.T) x_load(t + 1);
        f32x16 acc[RBW][4];
        if (work) {
#pragma unroll
            for (int rb = 0; rb < RBW; rb++)
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[rb][g][e] = 0.f;
            // ---- gates = [x_t | h_{t-1}] . [W_ih | W_hh]^T: one fragment stream, one A tile ----
            stream_part<RBW, 2>(acc, rw, wl, 0u, xS + lh * BMS + li, BMS, a.KPx);
            stream_part<RBW, 3>(acc, rw, wl, (uint32_t)a.KPx, hS + lh * BMS + li, BMS, a.KPh);

            // ---- cell update on the accumulator layout: col = lane & 31 (hidden unit), row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) ----
            rsrc_t rs_r, rs_z, rs_n, rs_g, rs_h;
            if (a.sv_r) {
                const size_t so_t = (size_t)t * B * H;
                const uint32_t sbytes = (uint32_t)a.B * (uint32_t)H * 4u;
                rs_r = make_rsrc(a.sv_r + so_t, sbytes); rs_z = make_rsrc(a.sv_z + so_t, sbytes); rs_n = make_rsrc(a.sv_n + so_t, sbytes);
                rs_g = make_rsrc(a.sv_g + so_t, sbytes); rs_h = make_rsrc(a.sv_h + so_t, sbytes);
            }
            // Element (rb, e) sits rc = 32 rb + (e & 3) + 8 (e >> 2) rows below the lane's first one: an immediate for the LDS
            // accesses, a wave-uniform offset for the stores.  The per-lane bases pass through opaque() once per step: left visible
            // as loop invariants, hipcc hoists every element's address out of the T loop and spills them.
            const int gr = opaque(tile_row0 + 4 * lh), unit = opaque(chunk * 32 + li);
            const uint32_t svo = ((uint32_t)gr * (uint32_t)H + (uint32_t)unit) * 4u;
            const float *hp0 = hS + unit * BMS + 4 * lh;
#pragma unroll
            for (int rb = 0; rb < RBW; rb++) {
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    const int rc = rb * 32 + (e & 3) + 8 * (e >> 2);                 // element e + 1: the next row
                    const CellPair cp = gru_cell_pair((osk::f2){acc[rb][0][e], acc[rb][0][e + 1]}, (osk::f2){acc[rb][1][e], acc[rb][1][e + 1]},
                                                      (osk::f2){acc[rb][2][e], acc[rb][2][e + 1]}, (osk::f2){acc[rb][3][e], acc[rb][3][e + 1]},
                                                      (osk::f2){hp0[rc], hp0[rc + 1]}, nb_r, nb_z, nb_n, b_hn);
                    acc[rb][0][e] = cp.hn[0]; acc[rb][0][e + 1] = cp.hn[1];         // h_t waits here for the barrier
                    if (a.sv_r) {
                        // write-once streams [B][H] of this step (non-temporal: they must not evict the weights): rows past the
                        // batch are not stored
#pragma unroll
                        for (int p = 0; p < 2; p++) {
                            if (gr + rc + p < a.B) {
                                const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)((rc + p) * H) * 4u);
                                osk::buf_store_nt(rs_r, svo, so, cp.r[p]); osk::buf_store_nt(rs_z, svo, so, cp.z[p]);
                                osk::buf_store_nt(rs_n, svo, so, cp.n[p]); osk::buf_store_nt(rs_g, svo, so, cp.ghn[p]);
                                osk::buf_store_nt(rs_h, svo, so, cp.hn[p]);
                            }
                        }
                    }
                }
            }
        }
        lds_barrier();            // every wave is done with x_t and h_{t-1}
        if (work) {
            float *hp0 = hS + opaque(chunk * 32 + li) * BMS + 4 * lh;
#pragma unroll
            for (int rb = 0; rb < RBW; rb++)
#pragma unroll
                for (int e = 0; e < 16; e++) hp0[rb * 32 + (e & 3) + 8 * (e >> 2)] = acc[rb][0][e];
        }
        if (t + 1 < a.T) x_store();
        lds_barrier();            // h_t and x_{t+1} are in the tile
    }
    if (a.seq_out) write_back(a.seq_out + (size_t)(a.T - 1) * H * B);
    if (a.h_last) write_back(a.h_last);
}

}  // namespace osg

namespace ost {

using osk::buf_load;
using osk::make_rsrc;
using osk::rsrc_t;

// One output chunk of the sweep's matrix phase: acc += dG[32 rows][sections] . W^T chunk over Q = 3H/2 gate-unit pairs, weights
// streamed from the transposed pack (256 bytes per pair), A fragments from the LDS tile.  arow: this lane's element of pair 0
// (row li, column lh).  is_h: the recurrent product reads the r-scaled n section (columns >= 2H shift by H; H is a multiple of the
// 16-pair block, so a block never straddles that boundary).  16 pairs in flight: 16 x 64 MFMA cycles cover an L2 round trip.
__device__ __forceinline__ void sweep_reduce(f32x16 &acc, const float *wp, int Q, const float *arow, bool is_h, int H, int lane)
{
    constexpr int D = 16;
    const rsrc_t rw = make_rsrc(wp, (uint32_t)Q * 256u);
    const uint32_t wl = (uint32_t)lane * 4u;
    float wbf[D], abf[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        wbf[d] = buf_load(rw, wl + (uint32_t)d * 256u, 0u);
        abf[d] = arow[2 * d];
    }
    for (int q0 = 0; q0 + D < Q; q0 += D) {
        const int qn = q0 + D;
        const uint32_t wo = __builtin_amdgcn_readfirstlane((uint32_t)qn * 256u);
        const int sh = __builtin_amdgcn_readfirstlane(2 * qn + ((is_h && qn >= H) ? H : 0));
#pragma unroll
        for (int d = 0; d < D; d++) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(abf[d], wbf[d], acc, 0, 0, 0);
            wbf[d] = buf_load(rw, wl + (uint32_t)d * 256u, wo);
            abf[d] = arow[sh + 2 * d];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int d = 0; d < D; d++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(abf[d], wbf[d], acc, 0, 0, 0);
}

// Backward sweep of one layer, t = T-1 .. 0, for a tile of 32 rows.  Wave c < H/32 owns hidden chunk c: it forms the gate
// derivatives of its 32 units in the MFMA accumulator layout (lane = unit, sixteen rows per lane), so dh_t of the chunk IS the
// accumulator that the recurrent product dh_{t-1} = z dh_t + [da_r | da_z | da_n r] . W_hh of the same wave is started from: dh
// never touches LDS.  LDS holds the gate-derivative tile dG [32][4H + 1] only (da_r | da_z | da_n | da_n r; odd pitch:
// conflict-free A fragments).  The dx chunks (need_dx) are dealt to the waves starting behind the last chunk owner.
// Two barriers per step; the saved activations of step t-1 are requested behind the first one and fly under the MFMAs of step t.
__global__ __launch_bounds__(osg::STREAM_NT, 1) void bwd_sweep_stream_kernel(const SweepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float dG[];
    const int H = a.H, K = a.K, GS = 4 * H + 1, Q = 3 * H / 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    const int row0 = blockIdx.x * 32;
    const size_t B = (size_t)a.B;
    const int nchh = H / 32, nchx = a.need_dx ? (K + 31) / 32 : 0;
    const bool own = wave < nchh;
    const int col = (own ? wave : 0) * 32 + li;              // hidden unit of this lane
    // the lane's sixteen elements: row grow + rc(e), rc(e) = (e & 3) + 8 (e >> 2), of unit col.  Every address of an element is ONE
    // per-lane offset (element 0) plus a wave-uniform offset of rc(e) rows; a row past the batch gets an offset no descriptor
    // covers (reads zero) and its stores are skipped.  The per-lane bases pass through opaque() once per step: left visible as loop
    // invariants, hipcc hoists all ~100 element addresses out of the T loop and spills them.
    const int grow = row0 + 4 * lh;
    auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
    const uint32_t sbytes = (uint32_t)(B * H * 4);
    // pd: dy of the step (the layer above), or dh_T of the top layer at t = T - 1
    float pr[16], pz[16], pn[16], pg[16], ph[16], pd[16];
    auto prefetch = [&](int t) {
        const size_t so = (size_t)t * B * H;
        const rsrc_t rr_ = make_rsrc(a.sv_r + so, sbytes), rz_ = make_rsrc(a.sv_z + so, sbytes), rn_ = make_rsrc(a.sv_n + so, sbytes),
                     rg_ = make_rsrc(a.sv_g + so, sbytes), rh_ = make_rsrc(a.sv_h + (t > 0 ? so - B * H : 0), sbytes),
                     rd_ = make_rsrc(a.dy ? a.dy + so : a.dy_last ? a.dy_last : a.sv_r, sbytes);
        const int gr = opaque(grow);
        const uint32_t vo = ((uint32_t)gr * (uint32_t)H + (uint32_t)opaque(col)) * 4u;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int rc = (e & 3) + 8 * (e >> 2);
            const uint32_t o = gr + rc < a.B ? vo : 0x80000000u, so_e = __builtin_amdgcn_readfirstlane((uint32_t)(rc * H) * 4u);
            pr[e] = osk::buf_load_nt(rr_, o, so_e); pz[e] = osk::buf_load_nt(rz_, o, so_e);
            pn[e] = osk::buf_load_nt(rn_, o, so_e); pg[e] = osk::buf_load_nt(rg_, o, so_e);
            ph[e] = osk::buf_load_nt(rh_, o, so_e); pd[e] = osk::buf_load_nt(rd_, o, so_e);
        }
    };
    f32x16 dh;
#pragma unroll
    for (int e = 0; e < 16; e++) dh[e] = 0.f;
    if (own) prefetch(a.T - 1);

    for (int t = a.T - 1; t >= 0; t--) {
        // ---- gate derivatives of the wave's chunk (VALU), into the LDS tile and out to dg4 [B][4H] of this step ----
        if (own) {
            const rsrc_t rg4 = make_rsrc(a.dg4 + (size_t)t * B * 4 * H, (uint32_t)(B * 4 * H * 4));
            const rsrc_t rdl = make_rsrc(a.dy_last ? a.dy_last : a.sv_r, sbytes);
            const uint32_t gH = (uint32_t)H * 4u;
            const bool last = a.dy_last && t == a.T - 1;
            const int gr = opaque(grow), cl = opaque(col);
            const uint32_t vo = ((uint32_t)gr * (uint32_t)H + (uint32_t)cl) * 4u, vg = ((uint32_t)gr * 4u * (uint32_t)H + (uint32_t)cl) * 4u;
            float *gp0 = dG + (4 * lh) * GS + cl;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int rc = (e & 3) + 8 * (e >> 2);
                const bool ok = gr + rc < a.B;
                const float rr = pr[e], zz = pz[e], nn = pn[e], gg = pg[e], hp = t > 0 ? ph[e] : 0.f;
                float dht = dh[e] + ((a.dy || last) ? pd[e] : 0.f);
                if (a.dy && last) dht += osk::buf_load(rdl, ok ? vo : 0x80000000u, __builtin_amdgcn_readfirstlane((uint32_t)(rc * H) * 4u));
                if (!ok) dht = 0.f;
                const float dn = dht * (1.0f - zz);
                const float dz = dht * (hp - nn);
                const float dan = dn * (1.0f - nn * nn);
                const float danr = dan * rr;
                const float dar = dan * gg * rr * (1.0f - rr);
                const float daz = dz * zz * (1.0f - zz);
                if (ok) {
                    const uint32_t sg = __builtin_amdgcn_readfirstlane((uint32_t)(rc * 4 * H) * 4u);
                    osk::buf_store_nt(rg4, vg, sg, dar); osk::buf_store_nt(rg4, vg, sg + gH, daz);
                    osk::buf_store_nt(rg4, vg, sg + 2 * gH, dan); osk::buf_store_nt(rg4, vg, sg + 3 * gH, danr);
                }
                float *gp = gp0 + rc * GS;
                gp[0] = dar; gp[H] = daz; gp[2 * H] = dan; gp[3 * H] = danr;
                dh[e] = dht * zz;              // the z dh_t part of dh_{t-1}; the matrix part accumulates on top below
            }
        }
        osg::lds_barrier();
        if (own && t > 0) prefetch(t - 1);
        // ---- dh_{t-1} (own chunk) and dx_t (chunks dealt round-robin from the first wave without a chunk of its own) ----
        const float *arow = dG + li * GS + lh;
        if (own) sweep_reduce(dh, a.whhT + (size_t)wave * Q * 64, Q, arow, true, H, lane);
        for (int oc = (wave + 8 - nchh) & 7; oc < nchx; oc += 8) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; e++) acc[e] = 0.f;
            sweep_reduce(acc, a.wihT + (size_t)oc * Q * 64, Q, arow, false, H, lane);
            const rsrc_t rdx = make_rsrc(a.dx + (size_t)t * B * K, (uint32_t)(B * K * 4));
            const int gr = opaque(grow), k = oc * 32 + li;
            const uint32_t vx = ((uint32_t)gr * (uint32_t)K + (uint32_t)k) * 4u;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int rc = (e & 3) + 8 * (e >> 2);
                const float v = acc[e];        // (a copy: __builtin_bit_cast of a vector ELEMENT reads element 0)
                if (k < K && gr + rc < a.B) osk::buf_store(rdx, vx, __builtin_amdgcn_readfirstlane((uint32_t)(rc * K) * 4u), v);
            }
        }
        osg::lds_barrier();            // every wave is done with this step's tile
    }
}

// ---- weight gradients without atomics ----
// dW [H3][K] = dG^T X over the rows of one slice.  Workgroup = 4 waves = 4 consecutive 32-unit gate chunks (blockIdx.x) x 128
// input columns (blockIdx.y) x one slice of rows (blockIdx.z): run-time chunk counts, one instantiation.  The X rows of a 32-row
// tile are staged once per workgroup through LDS (register-staged double buffer: tile i + 1 is in flight during tile i's MFMAs),
// each wave streams its own dG column chunk one tile ahead.  A = dG[r + kk][j0 + li], B = X[r + kk][k0 + li].  The tile is
// STORED: into dW when the launch has one slice, else into the slice's partial image [H3][K] | [H3] (dw_stream_reduce_kernel
// adds the images in slice order).  The bias gradient (column sums of dG) rides along in the workgroups of blockIdx.y = 0.
// Rows below x_valid_from pair with X = 0 (h_{-1}); a batch_first X (layer 0) is read in place.
constexpr int DWS_TR = 32, DWS_KW = 128, DWS_NC = DWS_KW / 32, DWS_NV = DWS_TR * DWS_KW / 256;
__global__ __launch_bounds__(256, 2) void dw_stream_kernel(const DwArgs a, float *part)
{
    __shared__ __attribute__((aligned(16))) float Xs[2][DWS_TR][DWS_KW];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, kk = lane >> 5;
    const int j0 = (blockIdx.x * 4 + wave) * 32;
    const bool jok = j0 < a.H3;
    const int jc = j0 + (3 * j0 >= 2 * a.H3 ? a.nshift : 0);          // column of the chunk in dG
    const size_t r0 = a.r_begin + (size_t)blockIdx.z * a.rows_per_slice;
    size_t r1 = r0 + a.rows_per_slice;
    if (r1 > a.r_end) r1 = a.r_end;
    const int kbase = blockIdx.y * DWS_KW;
    const int ntiles = r1 > r0 ? (int)((r1 - r0 + DWS_TR - 1) / DWS_TR) : 0;
    float *dW = part ? part + (size_t)blockIdx.z * ((size_t)a.H3 * a.K + a.H3) : a.dW;
    float *db = part ? dW + (size_t)a.H3 * a.K : a.db;
    auto xrow_off = [&](size_t rr) -> size_t {
        const uint32_t xr = (uint32_t)(rr - a.x_row_shift);            // row counts are far below 2^32: 32-bit div/mod
        return a.x_btf ? ((size_t)(xr % (uint32_t)a.B) * a.T + xr / (uint32_t)a.B) * (size_t)a.K : (size_t)xr * (size_t)a.K;
    };
    f32x16 acc[DWS_NC];
#pragma unroll
    for (int c = 0; c < DWS_NC; c++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[c][e] = 0.f;
    float stg[DWS_NV], avb[2][DWS_TR / 2], bsum = 0.f;
    auto stage_load = [&](int tile) {
#pragma unroll
        for (int i = 0; i < DWS_NV; i++) {
            const int flat = threadIdx.x + 256 * i, row = flat / DWS_KW, c = flat % DWS_KW;
            const size_t rr = r0 + (size_t)tile * DWS_TR + row;
            const bool ok = tile < ntiles && rr < r1 && rr >= a.x_valid_from && kbase + c < a.K;
            stg[i] = ok ? a.X[xrow_off(rr) + kbase + c] : 0.f;
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < DWS_NV; i++) {
            const int flat = threadIdx.x + 256 * i;
            Xs[buf][flat / DWS_KW][flat % DWS_KW] = stg[i];
        }
    };
    auto dg_load = [&](int tile, float *dst) {
        const size_t rt = r0 + (size_t)tile * DWS_TR;
#pragma unroll
        for (int st = 0; st < DWS_TR / 2; st++) {
            const size_t rr = rt + 2 * st + kk;
            dst[st] = (jok && tile < ntiles && rr < r1) ? __builtin_nontemporal_load(a.dG + rr * a.ldg + jc + li) : 0.f;
        }
    };
    stage_load(0);
    stage_store(0);
    dg_load(0, avb[0]);
    __syncthreads();
    for (int tile = 0; tile < ntiles; tile += 2) {
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int tl = tile + half;                        // ntiles may be odd: the last half-iteration only meets the barrier
            if (tl < ntiles) {
                stage_load(tl + 1);
                dg_load(tl + 1, avb[half ^ 1]);
#pragma unroll
                for (int st = 0; st < DWS_TR / 2; st++) {
                    const float av = avb[half][st];
                    bsum += av;
#pragma unroll
                    for (int c = 0; c < DWS_NC; c++)
                        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Xs[half][2 * st + kk][c * 32 + li], acc[c], 0, 0, 0);
                    if (st & 1) __builtin_amdgcn_sched_barrier(0);      // keep a tile's LDS reads from being hoisted (spills)
                }
                stage_store(half ^ 1);
            }
            __syncthreads();
        }
    }
    if (!jok) return;
#pragma unroll
    for (int c = 0; c < DWS_NC; c++) {
        const int k = kbase + c * 32 + li;
        if (k < a.K) {
#pragma unroll
            for (int e = 0; e < 16; e++) dW[(size_t)(j0 + (e & 3) + 8 * (e >> 2) + 4 * kk) * a.K + k] = acc[c][e];
        }
    }
    if (db && blockIdx.y == 0) {
        bsum += __shfl_xor(bsum, 32, 64);            // the two row parities of the same gate unit
        if (kk == 0) db[j0 + li] = bsum;
    }
}

// dW (and db) = the partial images added in slice order
__global__ __launch_bounds__(256) void dw_stream_reduce_kernel(size_t nw, size_t nb, int nsl, const float *part, float *dW, float *db)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = nw + nb;
    if (i >= stride || (i >= nw && !db)) return;
    float s = part[i];
    for (int sl = 1; sl < nsl; sl++) s += part[(size_t)sl * stride + i];
    if (i < nw) dW[i] = s;
    else db[i - nw] = s;
}

}  // namespace ost

using namespace osg;

// H > 128: the one layer kernel of these widths (inference, the two-kernel fused path, the training forward)
int os_gru_stream_launch_layer(os_ctx *ctx, const LayerArgs &a, hipStream_t s)
{
    if (a.H % 32 || a.H <= 128 || a.H > STREAM_KMAX) return os_fail(ctx, -4, "gru_stream_layer_kernel: hidden_size must be 160, 192, 224 or 256");
    if (a.K > STREAM_KMAX) return os_fail(ctx, -4, "gru_stream_layer_kernel: a layer input wider than 256 does not fit its LDS tile");
    if (a.xs_btf || a.gi) return os_fail(ctx, -4, "gru_stream_layer_kernel: reads the SoA input stream only");
    // (an offset of 2 GiB marks what must read zero: every real offset, plus the wave-uniform part, stays below it)
    if ((size_t)a.K * a.B * 4 >= ((size_t)1 << 31) || (size_t)a.H * a.B * 4 >= ((size_t)1 << 31))
        return os_fail(ctx, -2, "gru_stream_layer_kernel: one time step of the batch reaches 2 GiB, beyond its 32-bit buffer offsets; split the batch");
    if (!ctx->stream_attr_set) {
        OS_HIP(ctx, hipFuncSetAttribute((const void *)gru_stream_layer_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        OS_HIP(ctx, hipFuncSetAttribute((const void *)gru_stream_layer_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        OS_HIP(ctx, hipFuncSetAttribute((const void *)ost::bwd_sweep_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->stream_attr_set = true;
    }
    // 64-row tiles halve the weight bytes per MFMA; the recurrence cannot be split, so rows are the only parallel axis: they are
    // taken once they still put a workgroup on every compute unit (one workgroup per CU: its LDS tile)
    const int rbw = (a.B + 63) / 64 >= ctx->cu_count ? 2 : 1;
    const int BM = 32 * rbw;
    const size_t lds = (size_t)(2 * a.KPx + a.H) * (BM + 1) * sizeof(float);
    const int slot = os_prof_begin(ctx, OS_PHASE_GRU_LAYER, s, rbw == 2 ? "gru_stream_layer_kernel<2>" : "gru_stream_layer_kernel<1>");
    const dim3 grid((a.B + BM - 1) / BM), block(STREAM_NT);
    if (rbw == 2) hipLaunchKernelGGL(gru_stream_layer_kernel<2>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(gru_stream_layer_kernel<1>, grid, block, lds, s, a);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}

int os_gru_stream_launch_sweep(os_ctx *ctx, const ost::SweepArgs &a, hipStream_t s)
{
    if (!ctx->stream_attr_set) {
        OS_HIP(ctx, hipFuncSetAttribute((const void *)gru_stream_layer_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        OS_HIP(ctx, hipFuncSetAttribute((const void *)gru_stream_layer_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        OS_HIP(ctx, hipFuncSetAttribute((const void *)ost::bwd_sweep_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->stream_attr_set = true;
    }
    if ((size_t)a.B * 4 * a.H * 4 >= ((size_t)1 << 31) || (size_t)a.B * a.K * 4 >= ((size_t)1 << 31))
        return os_fail(ctx, -2, "bwd_sweep_stream_kernel: one time step of the batch reaches 2 GiB, beyond its 32-bit buffer offsets; split the batch");
    const size_t lds = (size_t)32 * (4 * a.H + 1) * sizeof(float);      // 131,200 bytes at H = 256
    const int slot = os_prof_begin(ctx, OS_PHASE_TRAIN_SWEEP, s, "bwd_sweep_stream_kernel");
    hipLaunchKernelGGL(ost::bwd_sweep_stream_kernel, dim3((a.B + 31) / 32), dim3(STREAM_NT), lds, s, a);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}

// One weight-gradient product over rows d.r_begin .. d.r_end (d.rows_per_slice is chosen here).  *ws / *ws_cap: the caller's
// scratch for the partial images, grown as needed.
int os_gru_stream_launch_dw(os_ctx *ctx, ost::DwArgs d, float **ws, size_t *ws_cap, hipStream_t s)
{
    const size_t rows = d.r_end - d.r_begin, nw = (size_t)d.H3 * d.K, nb = (size_t)d.H3;
    const unsigned gx = (unsigned)((d.H3 / 32 + 3) / 4), gy = (unsigned)((d.K + ost::DWS_KW - 1) / ost::DWS_KW);
    // slices: enough workgroups for two per compute unit, at least 256 rows each
    const size_t max_sl = (size_t)(2 * ctx->cu_count) / (gx * gy) > 0 ? (size_t)(2 * ctx->cu_count) / (gx * gy) : 1;
    size_t rps = ((rows + max_sl - 1) / max_sl + 31) / 32 * 32;
    rps = ctx->tune_dw_rps > 0 ? (size_t)ctx->tune_dw_rps : rps < 256 ? 256 : rps;
    const unsigned nsl = (unsigned)((rows + rps - 1) / rps);
    d.rows_per_slice = (int)rps;
    float *part = nullptr;
    if (nsl > 1) {
        if (os_ensure_scratch(ctx, ws, ws_cap, (size_t)nsl * (nw + nb))) return -10;
        part = *ws;
    }
    hipLaunchKernelGGL(ost::dw_stream_kernel, dim3(gx, gy, nsl), dim3(256), 0, s, d, part);
    if (part)
        hipLaunchKernelGGL(ost::dw_stream_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, nw, nb, (int)nsl,
                           (const float *)part, d.dW, d.db);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}
