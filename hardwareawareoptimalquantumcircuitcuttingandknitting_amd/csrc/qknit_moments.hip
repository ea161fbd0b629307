// qknit_moments.hip — second moments of the knit (gfx950): the cross-Gram of two tall row sets, the hot path
// of sum_x R[x] R'[x] without the 2^N output ("Second moments").
//
//   qk_gram_rows        G[i * ldg + j] = sum_{x < 2^m} A[i * lda + x] * B[j * ldb + x]   for i < RA, j < RB
//
// Layout. The output is cut into blocks of 64 x 64 row pairs and the reduction dimension x into S equal
// chunks; a workgroup of 256 threads (4 waves) owns one (block, chunk). It walks its chunk in tiles of 32 x,
// each staged through LDS as [64 rows][32 x] of A and of B (row pitch 34 doubles: the 32 lanes of a
// ds_read_b64 group, 16 rows x 2 k, fall on 32 distinct 8-byte banks). Global loads are 8 bytes per lane
// (rows sit at any 8-byte offset), 32 consecutive lanes on 256 contiguous bytes of a row; the next tile is in
// flight in registers while the current one is multiplied. Rows at or past RA / RB and x at or past the chunk
// end are zero-filled in registers on the way to LDS, never read; so m < 2 is a single 4-wide k-step whose
// missing terms are 0.0 * 0.0. On a diagonal block of the symmetric case (A == B, lda == ldb) that holds as
// many rows of B as of A the B tile is the A tile and is not loaded a second time; the values are the same
// either way, so the bits do not depend on it.
// The products are v_mfma_f64_16x16x4_f64: wave w owns the 2 x 2 sub-blocks (2 (w >> 1) + {0, 1},
// 2 (w & 1) + {0, 1}) of 16 x 16; lane l supplies A[row l & 15][x = l >> 4] and B[row l & 15][x = l >> 4] and
// holds D[row (l >> 4) + 4 r][col l & 15] in register r. A sub-block wholly outside RA x RB is skipped.
//
// Splitting (gr_make_shape; observables.gram_split is its host model): S is the smallest power of two with
// blocks * S >= 512 (two workgroups per CU: one's loads and barriers hide behind the other's MFMAs; measured
// against 256 and 1024) that is at most 256 and leaves a chunk of at least 256 x; it depends on
// (RA, RB, m) alone. With S > 1 the workgroups write their 64 x 64 partials to the workspace and
// gram_rows_stage2 adds the S partials of an output in ascending chunk order.
//
// Association (fixed by (RA, RB, m); the other rows, the launch and the run do not enter):
//   p_s[i][j] = the accumulator chain acc <- mfma(a, b, acc) from acc = +0.0 over the k-steps
//               x = x0(s), x0(s) + 4, ... of chunk s ascending; within a k-step the instruction's own
//               fixed order over its 4 products
//   G[i][j]   = ((p_0 + p_1) + p_2) + ... + p_{S-1}
// a * b is commutative and the order over x is the same on either side of the diagonal, so for A == B
// G[i][j] and G[j][i] are the same bits. No atomics; A and B are only read.
//
// Error: every partial is a chain of at most 2^m / S fused multiply-adds and the final sum adds S - 1
// roundings, so |G - exact| <= (2^m / S + S - 1) * 2^-53 * (|A| |B|^T)[i][j] to first order: within
// 2^m * 2^-53 * (|A| |B|^T)[i][j], the bound of a 2^m-term dot product in any order. Integer data whose
// partial sums stay below 2^53 is exact.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_BLOCK = 64;                   // rows of A and of B per workgroup
constexpr int GR_KT = 32;                      // x per LDS tile
constexpr int GR_PITCH = GR_KT + 2;            // row pitch of a tile, doubles
constexpr int GR_LOADS = GR_BLOCK * GR_KT / GR_THREADS;  // 8-byte loads per thread, tile and side
constexpr int64_t GR_MIN_GROUPS = 512;         // split x until this many workgroups exist (two per CU)
constexpr int64_t GR_MAX_SPLIT = 256;          // ... into at most this many chunks (stage 2 holds them in LDS)
constexpr int64_t GR_MIN_CHUNK = 256;          // ... but leave a chunk at least this long
constexpr int64_t GR_MAX_ROWS = (int64_t)1 << 30;
constexpr int GR_S2_COLS = 16;                 // outputs per stage-2 workgroup
constexpr int GR_S2_MAX_SPLIT = (int)GR_MAX_SPLIT;

typedef double gr_d4 __attribute__((ext_vector_type(4)));

struct gr_shape {
    int64_t ba, bb;  // blocks of 64 rows of A, of B
    int64_t split;   // S
    int64_t chunk;   // 2^m / S
};

gr_shape gr_make_shape(int64_t RA, int64_t RB, int m) {
    gr_shape s;
    s.ba = (RA + GR_BLOCK - 1) / GR_BLOCK;
    s.bb = (RB + GR_BLOCK - 1) / GR_BLOCK;
    const int64_t W = (int64_t)1 << m;
    s.split = 1;
    while (s.ba * s.bb * s.split < GR_MIN_GROUPS && s.split < GR_MAX_SPLIT && W / (2 * s.split) >= GR_MIN_CHUNK)
        s.split *= 2;
    s.chunk = W / s.split;
    return s;
}

int64_t gr_work_bytes(const gr_shape& sh) {
    return sh.split == 1 ? 0 : sh.ba * sh.bb * sh.split * GR_BLOCK * GR_BLOCK * (int64_t)sizeof(double);
}

__global__ __launch_bounds__(GR_THREADS) void gram_rows_kernel(gr_shape sh, int64_t RA, int64_t RB,
                                                                const double* __restrict__ A, int64_t lda,
                                                                const double* __restrict__ B, int64_t ldb,
                                                                double* __restrict__ G, int64_t ldg,
                                                                double* __restrict__ part) {
    __shared__ double sA[GR_BLOCK][GR_PITCH];
    __shared__ double sB[GR_BLOCK][GR_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, l4 = lane >> 4;
    int64_t g = blockIdx.x;
    const int64_t s = g % sh.split;
    g /= sh.split;
    const int64_t bj = g % sh.bb, bi = g / sh.bb;
    const int64_t i0 = bi * GR_BLOCK, j0 = bj * GR_BLOCK;
    const int64_t x0 = s * sh.chunk, x1 = x0 + sh.chunk;
    const int na = (int)(RA - i0 < GR_BLOCK ? RA - i0 : GR_BLOCK);  // rows of the block that exist
    const int nb = (int)(RB - j0 < GR_BLOCK ? RB - j0 : GR_BLOCK);
    // the B tile is the A tile: the same rows of the same buffer, and as many of them (RA != RB may leave a
    // diagonal block with na != nb; it then loads its B tile like any other block)
    const bool same = A == B && lda == ldb && bi == bj && na == nb;

    // loader: thread -> column lc of the tile, rows lr, lr + 8, ...
    const int lc = tid & (GR_KT - 1), lr = tid / GR_KT;
    const double* pa = A + (i0 + lr) * lda + lc;
    const double* pb = B + (j0 + lr) * ldb + lc;
    double ra[GR_LOADS], rb[GR_LOADS];
    auto load = [&](int64_t x) {
        const bool in = x + lc < x1;
#pragma unroll
        for (int v = 0; v < GR_LOADS; ++v) {
            const int r = lr + v * (GR_THREADS / GR_KT);
            ra[v] = (in && r < na) ? pa[(int64_t)v * (GR_THREADS / GR_KT) * lda + x] : 0.0;
            rb[v] = (!same && in && r < nb) ? pb[(int64_t)v * (GR_THREADS / GR_KT) * ldb + x] : 0.0;
        }
    };

    const int ai = 2 * (wave >> 1), bk = 2 * (wave & 1);  // this wave's sub-blocks: (ai + u, bk + v)
    const double(*tB)[GR_PITCH] = same ? sA : sB;
    bool live[2][2];
    gr_d4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            live[u][v] = 16 * (ai + u) < na && 16 * (bk + v) < nb;
            acc[u][v] = (gr_d4){0.0, 0.0, 0.0, 0.0};
        }

    load(x0);
    for (int64_t x = x0; x < x1; x += GR_KT) {
        __syncthreads();  // the previous tile is fully read
#pragma unroll
        for (int v = 0; v < GR_LOADS; ++v) {
            const int r = lr + v * (GR_THREADS / GR_KT);
            sA[r][lc] = ra[v];
            if (!same) sB[r][lc] = rb[v];
        }
        __syncthreads();
        if (x + GR_KT < x1) load(x + GR_KT);
        const int64_t left = x1 - x;
        const int ks = left < GR_KT ? (int)((left + 3) >> 2) : GR_KT / 4;
        if (ks == GR_KT / 4) {
#pragma unroll
            for (int kk = 0; kk < GR_KT / 4; ++kk) {
                double a[2], b[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    a[u] = sA[16 * (ai + u) + l16][4 * kk + l4];
                    b[u] = tB[16 * (bk + u) + l16][4 * kk + l4];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 2; ++v)
                        if (live[u][v]) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
            }
        } else {  // m < 5: one short tile
            for (int kk = 0; kk < ks; ++kk) {
                double a[2], b[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    a[u] = sA[16 * (ai + u) + l16][4 * kk + l4];
                    b[u] = tB[16 * (bk + u) + l16][4 * kk + l4];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 2; ++v)
                        if (live[u][v]) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
            }
        }
    }

    // D[row l4 + 4 r][col l16] of sub-block (u, v)
    double* p = part + ((bi * sh.bb + bj) * sh.split + s) * (GR_BLOCK * GR_BLOCK);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * (ai + u) + l4 + 4 * r, col = 16 * (bk + v) + l16;
                if (sh.split > 1)
                    p[row * GR_BLOCK + col] = acc[u][v][r];  // a skipped sub-block writes its zeros
                else if (row < na && col < nb)
                    G[(i0 + row) * ldg + j0 + col] = acc[u][v][r];
            }
}

// G[i][j] = sum_{s < S} part[((block * S + s) * 64 + i - i0) * 64 + j - j0], s ascending. A workgroup takes 16
// consecutive columns of one block row: all its S * 16 partials are loaded at once (S / 16 independent loads
// per thread) into LDS, then 16 threads add their column's S values in order.
__global__ __launch_bounds__(GR_THREADS) void gram_rows_stage2(gr_shape sh, int64_t RA, int64_t RB,
                                                                const double* __restrict__ part,
                                                                double* __restrict__ G, int64_t ldg) {
    __shared__ double buf[GR_S2_MAX_SPLIT][GR_S2_COLS];
    constexpr int RUNS = GR_BLOCK * GR_BLOCK / GR_S2_COLS;  // runs of 16 outputs per block
    constexpr int SL = GR_THREADS / GR_S2_COLS;             // partials per load round
    const int tid = threadIdx.x, el = tid & (GR_S2_COLS - 1), sl = tid / GR_S2_COLS;
    const int64_t blk = blockIdx.x / RUNS;
    const int e0 = (int)(blockIdx.x % RUNS) * GR_S2_COLS;
    const int64_t i = (blk / sh.bb) * GR_BLOCK + e0 / GR_BLOCK, j = (blk % sh.bb) * GR_BLOCK + e0 % GR_BLOCK;
    if (i >= RA || j >= RB) return;  // uniform: the whole run lies outside
    const double* p = part + blk * sh.split * (GR_BLOCK * GR_BLOCK) + e0 + el;
    const int S = (int)sh.split;
    double v[GR_S2_MAX_SPLIT / SL];
#pragma unroll
    for (int r = 0; r < GR_S2_MAX_SPLIT / SL; ++r) {
        const int sx = sl + r * SL;
        v[r] = sx < S ? p[(int64_t)sx * (GR_BLOCK * GR_BLOCK)] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < GR_S2_MAX_SPLIT / SL; ++r) {
        const int sx = sl + r * SL;
        if (sx < S) buf[sx][el] = v[r];
    }
    __syncthreads();
    if (tid < GR_S2_COLS && j + tid < RB) {
        double sum = buf[0][tid];
        for (int sx = 1; sx < S; ++sx) sum += buf[sx][tid];
        G[i * ldg + j + tid] = sum;
    }
}

int gr_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int gr_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

bool gr_overlap(const double* a, int64_t na, const double* b, int64_t nb) {  // [a, a + na) and [b, b + nb), doubles
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 8, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 8;
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int qk_gram_rows_workspace_bytes(int64_t RA, int64_t RB, int m, int64_t* bytes) {
    if (!bytes || m < 0 || m > 30 || RA < 1 || RB < 1 || RA > GR_MAX_ROWS || RB > GR_MAX_ROWS) return QK_EARG;
    *bytes = gr_work_bytes(gr_make_shape(RA, RB, m));
    return QK_OK;
}

int qk_gram_rows(qk_ctx* ctx, int64_t RA, int64_t RB, int m, const double* A, int64_t lda, const double* B,
                 int64_t ldb, double* G, int64_t ldg, void* ws, int64_t ws_bytes) {
    if (!ctx) return QK_EARG;
    if (m < 0 || m > 30) return gr_fail(ctx, "qk_gram_rows: m must be in 0..30");
    if (RA < 1 || RB < 1) return gr_fail(ctx, "qk_gram_rows: RA and RB must be at least 1");
    if (RA > GR_MAX_ROWS || RB > GR_MAX_ROWS) return gr_fail(ctx, "qk_gram_rows: more than 2^30 rows");
    const int64_t W = (int64_t)1 << m;
    if (lda < W || ldb < W) return gr_fail(ctx, "qk_gram_rows: lda or ldb < 2^m");
    if (ldg < RB) return gr_fail(ctx, "qk_gram_rows: ldg < RB");
    if (!A || !B || !G) return gr_fail(ctx, "qk_gram_rows: null buffer");
    if (lda > (INT64_MAX >> 4) / RA || ldb > (INT64_MAX >> 4) / RB || ldg > (INT64_MAX >> 4) / RA)
        return gr_fail(ctx, "qk_gram_rows: RA * lda, RB * ldb or RA * ldg overflows");
    const int64_t ng = (RA - 1) * ldg + RB;
    if (gr_overlap(G, ng, A, (RA - 1) * lda + W) || gr_overlap(G, ng, B, (RB - 1) * ldb + W))
        return gr_fail(ctx, "qk_gram_rows: G overlaps A or B");
    const gr_shape sh = gr_make_shape(RA, RB, m);
    const int64_t need = gr_work_bytes(sh);
    if (need > 0 && (!ws || ws_bytes < need))
        return gr_fail(ctx, "qk_gram_rows: workspace too small (qk_gram_rows_workspace_bytes)");
    const int64_t grid = sh.ba * sh.bb * sh.split;
    if (grid > 0x7fffffffLL / (GR_BLOCK * GR_BLOCK / GR_S2_COLS))
        return gr_fail(ctx, "qk_gram_rows: RA * RB exceeds the grid limit");
    int rc = gr_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(gram_rows_kernel, dim3((unsigned)grid), dim3(GR_THREADS), 0, ctx->stream, sh, RA, RB, A, lda, B,
                       ldb, G, ldg, part);
    rc = gr_hip(ctx, hipGetLastError(), "gram_rows_kernel");
    if (rc || sh.split == 1) return rc;
    const int64_t g2 = sh.ba * sh.bb * (GR_BLOCK * GR_BLOCK / GR_S2_COLS);
    hipLaunchKernelGGL(gram_rows_stage2, dim3((unsigned)g2), dim3(GR_THREADS), 0, ctx->stream, sh, RA, RB, part, G, ldg);
    return gr_hip(ctx, hipGetLastError(), "gram_rows_stage2");
}

}  // extern "C"
