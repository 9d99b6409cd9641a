// frames_kernels.hip -- frame ingest of the ViT chain: Resize((S, S)) -> Grayscale(1) -> ToTensor() of a PIL image after
// convert('RGB') (gru/gru_test.py:49-53,122-124, gru/gru_train.py:137-165, transformer/autoencoder_load.py:32-53,
// transformer/autoencoder_training.py:42-44,67-69), for uint8 frames [N][H][W][C], C = 1 | 3, bit for bit as Pillow computes it.
//
// The transform is integer arithmetic: per axis a table of bilinear (triangle) coefficients in 22-bit fixed point, built on the
// host in double exactly as Pillow's precompute_coeffs does; a horizontal pass over W on every channel, rounded to uint8; a
// vertical pass over H on those bytes, rounded to uint8; ITU-R 601 luma in 16-bit fixed point; a correctly rounded division by 255.
// An axis whose length already is S passes through: its table is the identity (one tap of 2^22 at xx, which the rounding maps to
// the byte itself), so the kernel has no second path.
//
// frames_ingest_kernel<C>: one workgroup of 256 threads = one (image, TH x TW output tile); one launch does both passes, the luma
// and the division, the 8-bit intermediate lives in LDS only.
//   tables  the tile's slices of the two axis tables ([rel | cnt | ks coefficient rows][T], tap-major so that the lanes of a
//           column / row group read consecutive dwords) are copied from the plan (L2) into LDS once per workgroup.
//   stage A the source window of the tile, rows [ymin(first row), ymin(last row) + cnt(last row)) x bytes [xmin(first col) C,
//           (xmin(last col) + cnt(last col)) C), goes from global memory into LDS by 16-byte loads on the address aligned DOWN to
//           16 (W C is arbitrary: a row starts at any byte), four loads in flight per lane.  A 16-byte piece that is not wholly
//           inside the caller's buffer [frames, frames + N H W C) is gathered byte by byte from the bytes that are: nothing outside
//           the buffer is read.  The row keeps its misalignment in LDS (stage B adds it back), the pitch is 16 k + 4 bytes.
//           When the whole window does not fit, stages A and B run over it in chunks of RCP rows (the 8-bit array holds all rows).
//   stage B horizontal pass, one thread per (window row, tile column); consecutive lanes walk DOWN the window rows of one column
//           (then the next column), so they share bounds and coefficients (LDS broadcast) and their byte reads are a pitch apart:
//           the pitch is an odd number of dwords, hence distinct banks up to the rows' differing misalignment (a 2-way conflict
//           where two rows' bytes straddle into the same bank; lanes across the tile columns of one row, the other mapping, would
//           be scale * C bytes apart: 137 dwords over a wave at 640 -> 224, 3 channels, i.e. 2- to 3-way everywhere).  Results go
//           to the 8-bit array [C][TW][RP], rows contiguous: consecutive lanes write consecutive bytes.
//   stage C vertical pass + luma + division, one thread per output pixel, lane = column: the taps are consecutive bytes down the
//           column, the lanes are RP bytes apart (RP / 4 odd: distinct banks), the vertical coefficients are the same for a wave's
//           row (broadcast); the float stores of a wave are whole 256-byte runs at TW = 64.
// The index splits idx -> (row, piece) and idx -> (column, row) divide by plan constants with a multiply-high (host-verified range).
#include "vit_host.hpp"
#include "frames_common.hpp"

#include <stdlib.h>
#include <vector>

extern "C" int os_vit_encode(os_ctx *ctx, int32_t N, const float *images, float *latent, void *stream);

namespace osfr {

constexpr int NT = 256;
constexpr int LDS_HARD = 64 * 1024;   // dynamic LDS without an attribute call; two workgroups per CU at the least

struct IngestArgs {
    const uint8_t *frames;
    float *out;                                       // frames_ingest_kernel
    uint8_t *out_u8;                                  // frames_ingest_u8_kernel: the byte L, before the division
    const int32_t *plan;
    size_t img_bytes, total_bytes;
    int N, S, row_bytes;
    int TH, TW, tw_log2, ntx, nty, ksx, ksy;
    int xwin_off, ywin_off, xblk_off, yblk_off;       // offsets (ints) into plan
    int P, cpr, RCP, RP;                              // raw pitch (bytes), 16-byte pieces per row, rows per chunk, 8-bit array pitch
    uint32_t cpr_magic, rcp_magic;
    int lds_raw, lds_mid;                             // byte offsets into the dynamic LDS block (the tables come first)
};

template <int C, bool U8>
__device__ __forceinline__ void ingest_body(const IngestArgs &a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int32_t *cx = (int32_t *)lds;                        // [2 + ksx][TW]: rel, cnt, coefficients by tap
    int32_t *cy = cx + (2 + a.ksx) * a.TW;               // [2 + ksy][TH]
    uint8_t *raw = lds + a.lds_raw;                      // [RCP][P]
    uint8_t *mid = lds + a.lds_mid;                      // [C][TW][RP]
    const int tid = threadIdx.x;
    const uint32_t tpi = (uint32_t)a.ntx * a.nty;
    const uint32_t n = blockIdx.x / tpi, t = blockIdx.x - n * tpi;
    const int ty = t / a.ntx, tx = t - ty * a.ntx;
    const int xw0 = a.plan[a.xwin_off + 2 * tx], xwn = a.plan[a.xwin_off + 2 * tx + 1];     // window: first pixel, pixels
    const int yw0 = a.plan[a.ywin_off + 2 * ty], ywn = a.plan[a.ywin_off + 2 * ty + 1];     //         first row, rows
    {
        const int nx = (2 + a.ksx) * a.TW, ny = (2 + a.ksy) * a.TH;
        const int32_t *gx = a.plan + a.xblk_off + (size_t)tx * nx, *gy = a.plan + a.yblk_off + (size_t)ty * ny;
        for (int i = tid; i < nx; i += NT) cx[i] = gx[i];
        for (int i = tid; i < ny; i += NT) cy[i] = gy[i];
    }
    const uint8_t *img = a.frames + (size_t)n * a.img_bytes;
    const uint8_t *buf_end = a.frames + a.total_bytes;
    const int bx0 = xw0 * C, len = xwn * C;
    const uint32_t lo0 = (uint32_t)(uintptr_t)img + (uint32_t)bx0;      // only its low four bits matter
    for (int r0 = 0; r0 < ywn; r0 += a.RCP) {
        const int rc = min(a.RCP, ywn - r0);
        // ---- stage A: rows yw0 + r0 .. + rc of the window -> raw ----
        const int items = rc * a.cpr;
        for (int base = tid; base < items; base += 4 * NT) {
            uint4 v[4];
            int dst[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int idx = base + k * NT;
                dst[k] = -1;
                if (idx < items) {
                    const int r = (int)div_magic((uint32_t)idx, a.cpr, a.cpr_magic), ch = idx - r * a.cpr;
                    const uint8_t *g = img + (size_t)(yw0 + r0 + r) * a.row_bytes + bx0;
                    const int mis = (int)((uintptr_t)g & 15);
                    if (ch * 16 < mis + len) {
                        v[k] = load16(g - mis + ch * 16, a.frames, buf_end);
                        dst[k] = r * a.P + ch * 16;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (dst[k] >= 0) {
                    uint32_t *d = (uint32_t *)(raw + dst[k]);
                    d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
                }
        }
        __syncthreads();
        // ---- stage B: horizontal pass of those rows -> mid ----
        const int itemsB = a.RCP * a.TW;
        for (int idx = tid; idx < itemsB; idx += NT) {
            const int col = (int)div_magic((uint32_t)idx, a.RCP, a.rcp_magic), r = idx - col * a.RCP;
            const int cnt = cx[a.TW + col];
            if (r >= rc || cnt == 0) continue;               // cnt 0: a column past the image's right edge
            const int mis = (int)((lo0 + (uint32_t)(yw0 + r0 + r) * (uint32_t)a.row_bytes) & 15u);
            const uint8_t *p = raw + r * a.P + mis + cx[col] * C;
            uint32_t acc[C];
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = 1u << (PB - 1);
            for (int x = 0; x < cnt; x++) {
                const uint32_t k = (uint32_t)cx[(2 + x) * a.TW + col];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] = __umul24(k, (uint32_t)p[x * C + c]) + acc[c];
            }
#pragma unroll
            for (int c = 0; c < C; c++) mid[(c * a.TW + col) * a.RP + r0 + r] = (uint8_t)min(acc[c] >> PB, 255u);
        }
        __syncthreads();
    }
    // ---- stage C: vertical pass, luma, division ----
    const int cstride = a.TW * a.RP;
    for (int idx = tid; idx < a.TH * a.TW; idx += NT) {
        const int yy = idx >> a.tw_log2, col = idx & (a.TW - 1);
        const int oy = ty * a.TH + yy, ox = tx * a.TW + col;
        if (oy >= a.S || ox >= a.S) continue;
        const int cnt = cy[a.TH + yy];
        const uint8_t *q = mid + col * a.RP + cy[yy];
        uint32_t acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 1u << (PB - 1);
        for (int x = 0; x < cnt; x++) {
            const uint32_t k = (uint32_t)cy[(2 + x) * a.TH + yy];
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = __umul24(k, (uint32_t)q[c * cstride + x]) + acc[c];
        }
        uint32_t L;
        if (C == 3) {
            const uint32_t R = min(acc[0] >> PB, 255u), G = min(acc[C > 1 ? 1 : 0] >> PB, 255u), B = min(acc[C > 2 ? 2 : 0] >> PB, 255u);
            L = (19595u * R + 38470u * G + 7471u * B + 32768u) >> 16;       // Pillow's L24 with its rounding
        } else
            L = min(acc[0] >> PB, 255u);
        const size_t o = (size_t)n * a.S * a.S + (size_t)oy * a.S + ox;
        if (U8) a.out_u8[o] = (uint8_t)L;
        else a.out[o] = __fdiv_rn((float)L, 255.0f);
    }
}

template <int C>
__global__ __launch_bounds__(NT) void frames_ingest_kernel(const IngestArgs a) { ingest_body<C, false>(a); }

// the same image as bytes: what the augmentation (frames_augment.hip) reads
template <int C>
__global__ __launch_bounds__(NT) void frames_ingest_u8_kernel(const IngestArgs a) { ingest_body<C, true>(a); }

// ---- host: tables and plan ----

struct Axis { int in, S, ks; std::vector<int> lo, cnt, coef; };       // coef [S][ks]

// the table of an axis: axis_entry (frames_common.hpp) for every output index
static void build_axis(int in, int S, Axis &ax)
{
    ax.in = in; ax.S = S;
    ax.lo.assign(S, 0); ax.cnt.assign(S, 0);
    const double scale = (double)in / (double)S;
    ax.ks = in == S ? 1 : 2 * (int)ceil(scale < 1.0 ? 1.0 : scale) + 1;
    ax.coef.assign((size_t)S * ax.ks, 0);
    for (int xx = 0; xx < S; xx++) axis_entry(in, S, xx, ax.lo[xx], ax.cnt[xx], &ax.coef[(size_t)xx * ax.ks], 1);
}

struct Plan {
    int H, W, C, S;
    bool used;
    uint64_t stamp;
    int32_t *dev;
    IngestArgs args;               // everything but frames / out / N / total_bytes
    size_t lds_bytes;
    int win_rows_max, win_bytes_max;
    uint64_t read_bytes;           // per image: 16-byte pieces that stage A loads, summed over the tiles
};

struct State {
    Plan plans[4];
    uint64_t clock;
    float *fbuf; size_t fbuf_floats;   // os_vit_encode_frames: the frames between the two halves
};

struct Windows { int n, T; std::vector<int> w0, wn; int wn_max; };

static void windows_of(const Axis &ax, int T, Windows &wd)
{
    wd.T = T; wd.n = (ax.S + T - 1) / T; wd.wn_max = 0;
    wd.w0.assign(wd.n, 0); wd.wn.assign(wd.n, 0);
    for (int t = 0; t < wd.n; t++) {
        int lo = ax.in, hi = 0;
        for (int i = t * T; i < ax.S && i < (t + 1) * T; i++) {
            if (ax.lo[i] < lo) lo = ax.lo[i];
            if (ax.lo[i] + ax.cnt[i] > hi) hi = ax.lo[i] + ax.cnt[i];
        }
        wd.w0[t] = lo; wd.wn[t] = hi - lo;
        if (hi - lo > wd.wn_max) wd.wn_max = hi - lo;
    }
}

// [rel | cnt | ks coefficient rows][T] per tile; entries past the axis end stay zero (cnt 0)
static void tile_blocks(const Axis &ax, const Windows &wd, std::vector<int32_t> &out)
{
    const int T = wd.T, per = (2 + ax.ks) * T;
    const size_t at = out.size();
    out.resize(at + (size_t)wd.n * per, 0);
    for (int t = 0; t < wd.n; t++) {
        int32_t *b = out.data() + at + (size_t)t * per;
        for (int j = 0; j < T && t * T + j < ax.S; j++) {
            const int i = t * T + j;
            b[j] = ax.lo[i] - wd.w0[t];
            b[T + j] = ax.cnt[i];
            for (int x = 0; x < ax.cnt[i]; x++) b[(2 + x) * T + j] = ax.coef[(size_t)i * ax.ks + x];
        }
    }
}

struct HostPlan {
    IngestArgs a;                  // everything but frames / out / plan / N / total_bytes
    size_t lds_bytes;
    int win_rows_max, win_bytes_max;
    uint64_t read_bytes;
    std::vector<int32_t> table;    // [x windows | y windows | x tile blocks | y tile blocks]
};

// Tables, tile choice and LDS layout of a geometry; false: no tile of the menu holds it.  soft: the preferred LDS bytes per workgroup.
static bool plan_host(int soft, int H, int W, int C, int S, HostPlan &hp)
{
    Axis ax, ay;
    build_axis(W, S, ax);
    build_axis(H, S, ay);
    static const int menu[4][2] = {{32, 64}, {16, 64}, {16, 32}, {8, 32}};
    IngestArgs &a = hp.a;
    memset(&a, 0, sizeof(a));
    Windows wx, wy;
    bool found = false;
    // largest tile that holds its whole window within the preferred budget, then within the hard limit, then the largest that
    // holds the 8-bit array and at least one row of the window (stages A and B in chunks)
    for (int pass = 0; pass < 3 && !found; pass++)
        for (int m = 0; m < 4 && !found; m++) {
            const int TH = menu[m][0], TW = menu[m][1];
            if (TW == 64 && S <= 32) continue;
            windows_of(ax, TW, wx);
            windows_of(ay, TH, wy);
            const long tab = ((long)(2 + ax.ks) * TW + (long)(2 + ay.ks) * TH) * 4;
            const long P = ((long)wx.wn_max * C + 15 + 15) / 16 * 16 + 4;
            long RP = ((long)wy.wn_max + 3) / 4 * 4;
            if ((RP / 4) % 2 == 0) RP += 4;
            const long mid = (long)C * TW * RP;
            const long limit = pass == 0 ? soft : LDS_HARD;
            long rcp = wy.wn_max;
            if (pass == 2 && (limit - tab - mid) / P < rcp) rcp = (limit - tab - mid) / P;
            if (rcp < 1 || tab + mid + rcp * P > limit) continue;
            if (rcp * ((P - 4) / 16) >= 65536 || rcp * TW >= 65536) continue;       // range of the multiply-high divisions
            found = true;
            a.TH = TH; a.TW = TW; a.tw_log2 = TW == 64 ? 6 : 5; a.ntx = wx.n; a.nty = wy.n; a.ksx = ax.ks; a.ksy = ay.ks;
            a.P = (int)P; a.cpr = (int)((P - 4) / 16); a.RCP = (int)rcp; a.RP = (int)RP;
            a.cpr_magic = magic_of(a.cpr); a.rcp_magic = magic_of(a.RCP);
            a.lds_raw = (int)tab; a.lds_mid = (int)(tab + rcp * P);
            hp.lds_bytes = (size_t)(tab + rcp * P + mid);
        }
    if (!found) return false;
    a.S = S; a.row_bytes = W * C; a.img_bytes = (size_t)H * W * C;
    hp.win_rows_max = wy.wn_max; hp.win_bytes_max = wx.wn_max * C;
    std::vector<int32_t> &tb = hp.table;
    tb.clear();
    a.xwin_off = 0;
    for (int t = 0; t < wx.n; t++) { tb.push_back(wx.w0[t]); tb.push_back(wx.wn[t]); }
    a.ywin_off = (int)tb.size();
    for (int t = 0; t < wy.n; t++) { tb.push_back(wy.w0[t]); tb.push_back(wy.wn[t]); }
    a.xblk_off = (int)tb.size();
    tile_blocks(ax, wx, tb);
    a.yblk_off = (int)tb.size();
    tile_blocks(ay, wy, tb);
    // read traffic of one image: per tile, rows x 16-byte pieces (a row's misalignment can add one more piece)
    hp.read_bytes = 0;
    for (int ty = 0; ty < wy.n; ty++)
        for (int tx = 0; tx < wx.n; tx++)
            hp.read_bytes += (uint64_t)wy.wn[ty] * (uint64_t)(((long)wx.wn[tx] * C + 15) / 16 * 16);
    return true;
}

// Builds the plan of a geometry into slot p and uploads its tables.  -4: the geometry is outside what the tile menu can hold in LDS.
static int build_plan(os_ctx *ctx, Plan &p, int H, int W, int C, int S)
{
    HostPlan hp;
    if (!plan_host(ctx->tune_frames_lds_kb * 1024, H, W, C, S, hp)) {
        snprintf(ctx->err, sizeof(ctx->err),
                 "os_frames_ingest: %d x %d x %d -> %d: the source window of the smallest tile (8 x 32) needs more than the %d bytes of LDS "
                 "a workgroup has; supported are H, W <= 8192 at a per-axis down-scale ratio up to 32", H, W, C, S, LDS_HARD);
        return -4;
    }
    p.used = false;                // from here on the slot's previous plan is gone
    if (p.dev) { OS_HIP(ctx, hipFree(p.dev)); p.dev = nullptr; }       // waits for the launches that still read it
    OS_HIP(ctx, hipMalloc((void **)&p.dev, hp.table.size() * sizeof(int32_t)));
    OS_HIP(ctx, hipMemcpy(p.dev, hp.table.data(), hp.table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    p.args = hp.a;
    p.args.plan = p.dev;
    p.lds_bytes = hp.lds_bytes; p.win_rows_max = hp.win_rows_max; p.win_bytes_max = hp.win_bytes_max; p.read_bytes = hp.read_bytes;
    p.H = H; p.W = W; p.C = C; p.S = S; p.used = true;
    return 0;
}

static State *state_get(os_ctx *ctx)
{
    if (!ctx->frames) {
        ctx->frames = calloc(1, sizeof(State));
        if (!ctx->frames) os_fail(ctx, -13, "os_frames: out of memory");
    }
    return (State *)ctx->frames;
}

// the cached plan of a geometry, built and uploaded the first time it is seen (least recently used of four replaced)
static int plan_get(os_ctx *ctx, int H, int W, int C, int S, Plan **out)
{
    State *st = state_get(ctx);
    if (!st) return -13;
    Plan *victim = nullptr;
    for (Plan &p : st->plans) {
        if (p.used && p.H == H && p.W == W && p.C == C && p.S == S) { p.stamp = ++st->clock; *out = &p; return 0; }
        if (!victim || (victim->used && (!p.used || p.stamp < victim->stamp))) victim = &p;
    }
    if (int rc = build_plan(ctx, *victim, H, W, C, S)) return rc;
    victim->stamp = ++st->clock;
    *out = victim;
    return 0;
}

static int check_geometry(os_ctx *ctx, const char *who, int N, const void *frames, int H, int W, int C, int S, const void *out)
{
    if (N < 1 || !frames || !out || H < 1 || W < 1 || S < 1 || (C != 1 && C != 3)) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: bad argument (N >= 1, H, W, out_size >= 1, C = 1 | 3, non-null pointers)", who);
        return -2;
    }
    if (H > (1 << 20) || W > (1 << 20) || S > 8192) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: %d x %d -> %d is outside the supported range (H, W <= 8192 at a per-axis down-scale "
                 "ratio up to 32, out_size <= 8192)", who, H, W, S);
        return -4;
    }
    return 0;
}

// out: float32 [N][S][S], or with u8 the bytes before the division
static int ingest(os_ctx *ctx, int N, const uint8_t *frames, int H, int W, int C, int S, void *out, bool u8, hipStream_t s)
{
    Plan *p = nullptr;
    if (int rc = plan_get(ctx, H, W, C, S, &p)) return rc;
    IngestArgs a = p->args;
    const uint64_t blocks = (uint64_t)N * a.ntx * a.nty;
    if (blocks > 0x7fffffffull) return os_fail(ctx, -4, "os_frames_ingest: more than 2^31 - 1 tiles in one call: split the batch");
    a.frames = frames; a.out = u8 ? nullptr : (float *)out; a.out_u8 = u8 ? (uint8_t *)out : nullptr; a.N = N; a.total_bytes = (size_t)N * a.img_bytes;
    const int slot = os_prof_begin(ctx, OS_PHASE_VIT_MISC, s, u8 ? (C == 3 ? "frames_ingest_u8_kernel<3>" : "frames_ingest_u8_kernel<1>")
                                                                   : (C == 3 ? "frames_ingest_kernel<3>" : "frames_ingest_kernel<1>"));
    if (u8 && C == 3) hipLaunchKernelGGL(frames_ingest_u8_kernel<3>, dim3((unsigned)blocks), dim3(NT), p->lds_bytes, s, a);
    else if (u8) hipLaunchKernelGGL(frames_ingest_u8_kernel<1>, dim3((unsigned)blocks), dim3(NT), p->lds_bytes, s, a);
    else if (C == 3) hipLaunchKernelGGL(frames_ingest_kernel<3>, dim3((unsigned)blocks), dim3(NT), p->lds_bytes, s, a);
    else hipLaunchKernelGGL(frames_ingest_kernel<1>, dim3((unsigned)blocks), dim3(NT), p->lds_bytes, s, a);
    os_prof_end(ctx, slot, s);
    OS_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace osfr

void os_frames_destroy(os_ctx *ctx)
{
    osfr::State *st = (osfr::State *)ctx->frames;
    if (!st) return;
    for (osfr::Plan &p : st->plans)
        if (p.dev) (void)hipFree(p.dev);
    if (st->fbuf) (void)hipFree(st->fbuf);
    free(st);
    ctx->frames = nullptr;
}

extern "C" {

int os_frames_ingest(os_ctx *ctx, int32_t N, const uint8_t *frames, int32_t H, int32_t W, int32_t C, int32_t out_size, float *out,
                     void *stream)
{
    OS_CHECK_CTX(ctx);
    if (int rc = osfr::check_geometry(ctx, "os_frames_ingest", N, frames, H, W, C, out_size, out)) return rc;
    OS_HIP(ctx, hipSetDevice(ctx->device));
    return osfr::ingest(ctx, N, frames, H, W, C, out_size, out, false, (hipStream_t)stream);
}

int os_frames_ingest_u8(os_ctx *ctx, int32_t N, const uint8_t *frames, int32_t H, int32_t W, int32_t C, int32_t out_size, uint8_t *gray,
                        void *stream)
{
    OS_CHECK_CTX(ctx);
    if (int rc = osfr::check_geometry(ctx, "os_frames_ingest_u8", N, frames, H, W, C, out_size, gray)) return rc;
    OS_HIP(ctx, hipSetDevice(ctx->device));
    return osfr::ingest(ctx, N, frames, H, W, C, out_size, gray, true, (hipStream_t)stream);
}

int os_vit_encode_frames(os_ctx *ctx, int32_t N, const uint8_t *frames, int32_t H, int32_t W, int32_t C, float *latent, void *stream)
{
    OS_CHECK_CTX(ctx);
    os_vit_state *v = (os_vit_state *)ctx->vit;
    if (!v || !v->w) return os_fail(ctx, -5, "os_vit_encode_frames: call os_vit_load first");
    const int S = v->d.img;
    if (int rc = osfr::check_geometry(ctx, "os_vit_encode_frames", N, frames, H, W, C, S, latent)) return rc;
    OS_HIP(ctx, hipSetDevice(ctx->device));
    osfr::State *st = osfr::state_get(ctx);
    if (!st) return -13;
    if (os_ensure_scratch(ctx, &st->fbuf, &st->fbuf_floats, (size_t)N * S * S)) return -10;
    if (int rc = osfr::ingest(ctx, N, frames, H, W, C, S, st->fbuf, false, (hipStream_t)stream)) return rc;
    return os_vit_encode(ctx, N, st->fbuf, latent, stream);
}

int os_frames_plan_info(os_ctx *ctx, int32_t H, int32_t W, int32_t C, int32_t out_size, int64_t *info)
{
    OS_CHECK_CTX(ctx);
    if (int rc = osfr::check_geometry(ctx, "os_frames_plan_info", 1, info, H, W, C, out_size, info)) return rc;
    OS_HIP(ctx, hipSetDevice(ctx->device));
    osfr::Plan *p = nullptr;
    if (int rc = osfr::plan_get(ctx, H, W, C, out_size, &p)) return rc;
    info[0] = p->args.TH; info[1] = p->args.TW; info[2] = (int64_t)p->lds_bytes; info[3] = p->args.RCP;
    info[4] = p->win_rows_max; info[5] = p->win_bytes_max; info[6] = (int64_t)p->read_bytes; info[7] = (int64_t)p->args.ntx * p->args.nty;
    return 0;
}

}  // extern "C"
