// qknit_shots.hip — inverse-CDF draws from rows of a product that is never stored (gfx950): the hot
// kernel of shot sampling from the exact knit ("Shots").
//
//   w[r][x] = max(sum_{k<K} C[r][k] X[k][x], 0)       r < n_rows, x < 2^m
//   draw d of row r:  x_out[d] = the first x (ascending) whose inclusive prefix sum of w[r] exceeds
//                     u[d] * row_total[r],  w_out[d] = w[r][x_out[d]]
//
// The [n_rows, 2^m] product would be 10-40 GB for 20000 rows of a 2^16..2^18 wide fragment; only one
// double per (row, tile) is kept. A row is cut into tiles of T = 2^t consecutive x (t = min(m, 10)).
//
//   sr_tile_sums   a 256-thread workgroup owns one tile and a block of up to 16 rows. Thread tid holds
//                  xl = e * 256 + tid (e < 4): one coalesced 8-byte load of X[k][tile * T + xl] per k
//                  feeds 16 x 4 fused multiply-adds acc[r][e] = fma(C[r][k], x, acc[r][e]), k ascending,
//                  the coefficients staged in LDS (64 k at a time) and read as broadcasts. Then the clamp
//                  at 0 and the tile's sum in a fixed order: register slots ascending, shfl_xor over the
//                  wave (both lanes of a pair form the same a + b), the four waves ascending through LDS.
//                  The kernel is bound by the reads of X from L2 (8 bytes per SR_ROWS fma): 16 rows
//                  (128 accumulator VGPRs, 3 waves per SIMD) measured 22 % faster than 8 on syc 32 5.
//   sr_tile_scan   one workgroup per row: inclusive prefix sums of its tile sums, in place. Thread tid
//                  sums 8 consecutive tiles serially; thread 0 then chains the thread totals serially
//                  (B[t+1] = B[t] + total[t], carried from one 2048-tile chunk to the next) and every
//                  thread writes B[tid] + its running sum. The result is monotone and flat over empty
//                  tiles (B[t+1] is bit for bit the last prefix of thread t), which a tree scan of
//                  doubles does not guarantee and the binary search below needs. row_total is the last
//                  prefix itself, so u * row_total < row_total always finds a tile.
//   sr_locate      one workgroup per draw: the row of the draw (binary search in draw_off), the first
//                  tile whose prefix exceeds the target (binary search; its sum is > 0 by the above),
//                  that tile's weights again by the same fma chain as sr_tile_sums (same bits), a scan
//                  over them in x order (4 consecutive x per thread, lanes by shfl_up, waves ascending)
//                  and the smallest x with w > 0 whose prefix exceeds the target; if rounding leaves none
//                  (the in-tile scan and the tile sum associate differently), the last x with w > 0.
//
// No atomics; X, C, u are only read; the order of every sum depends on (K, m) alone (a row's values do
// not depend on which block of rows it is in), so two launches give identical bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "internal.h"
#include "rng.h"

namespace {

constexpr int SR_TILE_BITS = 10;  // tile of 2^10 doubles: 4 per thread
constexpr int SR_THREADS = 256;
constexpr int SR_E = 4;
constexpr int SR_ROWS = 16;  // rows per workgroup of sr_tile_sums
constexpr int SR_KC = 64;   // coefficients staged per row and LDS fill
constexpr int SR_SPT = 8;   // tiles per thread and chunk in sr_tile_scan

__global__ __launch_bounds__(SR_THREADS) void sr_uniforms_kernel(uint64_t seed, int64_t label, int64_t first,
                                                                 int64_t n, double* __restrict__ u) {
    for (int64_t i = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SR_THREADS)
        u[i] = draw(seed, label, first + i);
}

__global__ __launch_bounds__(SR_THREADS) void sr_tile_sums(int t, int64_t n_tiles, int64_t n_rb, int64_t K,
                                                           const double* __restrict__ X, int64_t ldx, int64_t n_rows,
                                                           const double* __restrict__ C, int64_t ldc,
                                                           double* __restrict__ work) {
    __shared__ double cs[SR_KC][SR_ROWS];
    __shared__ double red[SR_ROWS][SR_THREADS / 64];
    const int tid = threadIdx.x;
    const uint32_t T = 1u << t;
    // consecutive workgroups share the tile of X (row blocks fastest): it stays in cache
    const int64_t tile = (int64_t)blockIdx.x / n_rb, row0 = ((int64_t)blockIdx.x % n_rb) * SR_ROWS;
    const double* xp = X + (tile << t);

    double acc[SR_ROWS][SR_E];
#pragma unroll
    for (int r = 0; r < SR_ROWS; ++r)
#pragma unroll
        for (int e = 0; e < SR_E; ++e) acc[r][e] = 0.0;

    for (int64_t k0 = 0; k0 < K; k0 += SR_KC) {
        const int kn = (int)(K - k0 < SR_KC ? K - k0 : SR_KC);
        __syncthreads();  // the previous chunk's coefficients are no longer read
        for (int i = tid; i < SR_KC * SR_ROWS; i += SR_THREADS) {
            const int r = i / SR_KC, kk = i % SR_KC;
            cs[kk][r] = (row0 + r < n_rows && kk < kn) ? C[(row0 + r) * ldc + k0 + kk] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kn; ++kk) {
            const double* p = xp + (k0 + kk) * ldx;
            double x[SR_E];
#pragma unroll
            for (int e = 0; e < SR_E; ++e) {
                const uint32_t xl = (uint32_t)e * SR_THREADS + tid;
                x[e] = xl < T ? p[xl] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < SR_ROWS; ++r) {
                const double c = cs[kk][r];
#pragma unroll
                for (int e = 0; e < SR_E; ++e) acc[r][e] = fma(c, x[e], acc[r][e]);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < SR_ROWS; ++r) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < SR_E; ++e) {
            const double w = acc[r][e] > 0.0 ? acc[r][e] : 0.0;
            s = e == 0 ? w : s + w;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
        if ((tid & 63) == 0) red[r][tid >> 6] = s;
    }
    __syncthreads();
    if (tid < SR_ROWS && row0 + tid < n_rows)
        work[(row0 + tid) * n_tiles + tile] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

__global__ __launch_bounds__(SR_THREADS) void sr_tile_scan(int64_t n_tiles, double* __restrict__ work,
                                                           double* __restrict__ row_total) {
    __shared__ double part[SR_THREADS];
    __shared__ double carry_s;
    const int tid = threadIdx.x;
    double* p = work + (int64_t)blockIdx.x * n_tiles;
    if (tid == 0) carry_s = 0.0;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += (int64_t)SR_THREADS * SR_SPT) {
        double v[SR_SPT];
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < SR_SPT; ++k) {
            const int64_t i = base + (int64_t)tid * SR_SPT + k;
            run += i < n_tiles ? p[i] : 0.0;
            v[k] = run;
        }
        part[tid] = run;
        __syncthreads();
        if (tid == 0) {  // the thread totals chained serially: part[t] becomes the prefix before thread t
            const int64_t left = (n_tiles - base + SR_SPT - 1) / SR_SPT;
            const int used = (int)(left < SR_THREADS ? left : SR_THREADS);
            double b = carry_s;
            for (int th = 0; th < used; ++th) {
                const double tot = part[th];
                part[th] = b;
                b += tot;
            }
            carry_s = b;
        }
        __syncthreads();
        const double b = part[tid];
#pragma unroll
        for (int k = 0; k < SR_SPT; ++k) {
            const int64_t i = base + (int64_t)tid * SR_SPT + k;
            if (i < n_tiles) p[i] = b + v[k];
        }
        __syncthreads();
    }
    if (tid == 0) row_total[blockIdx.x] = carry_s;  // bit for bit the last prefix
}

__global__ __launch_bounds__(SR_THREADS) void sr_locate(int t, int64_t n_tiles, int64_t K,
                                                        const double* __restrict__ X, int64_t ldx, int64_t n_rows,
                                                        const double* __restrict__ C, int64_t ldc,
                                                        const int64_t* __restrict__ draw_off,
                                                        const double* __restrict__ u, const double* __restrict__ pre,
                                                        const double* __restrict__ row_total,
                                                        int64_t* __restrict__ x_out, double* __restrict__ w_out) {
    __shared__ double wl[SR_E * SR_THREADS];
    __shared__ double wsum[SR_THREADS / 64];
    __shared__ int first_s[SR_THREADS / 64], last_s[SR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t T = 1u << t;
    const int64_t d = blockIdx.x;

    int64_t lo = 0, hi = n_rows - 1;  // the last row with draw_off[r] <= d
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (draw_off[mid] <= d) lo = mid;
        else hi = mid - 1;
    }
    const int64_t r = lo;
    const double total = row_total[r];
    if (!(total > 0.0) || total == INFINITY) {  // the whole workgroup leaves: nothing to draw from
        if (tid == 0) {
            x_out[d] = -1;
            w_out[d] = 0.0;
        }
        return;
    }
    const double target = u[d] * total;
    const double* P = pre + r * n_tiles;
    lo = 0, hi = n_tiles - 1;  // the first tile whose inclusive prefix exceeds the target
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (P[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    const int64_t tile = lo;
    const double before = tile ? P[tile - 1] : 0.0;

    // the tile's weights, by the fma chain of sr_tile_sums
    double acc[SR_E];
#pragma unroll
    for (int e = 0; e < SR_E; ++e) acc[e] = 0.0;
    const double* xp = X + (tile << t);
    const double* cr = C + r * ldc;
    for (int64_t k = 0; k < K; ++k) {
        const double c = cr[k];
        const double* p = xp + k * ldx;
#pragma unroll
        for (int e = 0; e < SR_E; ++e) {
            const uint32_t xl = (uint32_t)e * SR_THREADS + tid;
            acc[e] = fma(c, xl < T ? p[xl] : 0.0, acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < SR_E; ++e) wl[e * SR_THREADS + tid] = acc[e] > 0.0 ? acc[e] : 0.0;
    __syncthreads();

    // prefix sums in x order: 4 consecutive x per thread, lanes by shfl_up, waves ascending
    double w[SR_E], v[SR_E];
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < SR_E; ++e) {
        w[e] = wl[tid * SR_E + e];
        run += w[e];
        v[e] = run;
    }
    double inc = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    double wpre = 0.0;
    for (int wv = 0; wv < wave; ++wv) wpre += wsum[wv];
    ex += wpre;

    int first = 1 << 30, last = -1;  // smallest x with w > 0 and prefix > target; largest x with w > 0
#pragma unroll
    for (int e = 0; e < SR_E; ++e) {
        if (w[e] > 0.0) {
            last = tid * SR_E + e;
            if (first == (1 << 30) && before + (ex + v[e]) > target) first = tid * SR_E + e;
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int f2 = __shfl_xor(first, off, 64), l2 = __shfl_xor(last, off, 64);
        first = f2 < first ? f2 : first;
        last = l2 > last ? l2 : last;
    }
    if (lane == 0) {
        first_s[wave] = first;
        last_s[wave] = last;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < SR_THREADS / 64; ++wv) {
            first = first_s[wv] < first ? first_s[wv] : first;
            last = last_s[wv] > last ? last_s[wv] : last;
        }
        const int xs = first != (1 << 30) ? first : last;
        x_out[d] = xs < 0 ? -1 : (tile << t) + xs;
        w_out[d] = xs < 0 ? 0.0 : wl[xs];
    }
}

int sr_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int sr_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

int64_t sr_tiles(int m) { return (int64_t)1 << (m > SR_TILE_BITS ? m - SR_TILE_BITS : 0); }

}  // namespace

extern "C" {

int qk_uniforms(qk_ctx* ctx, uint64_t seed, int64_t label, int64_t first, int64_t n, double* u) {
    if (!ctx) return QK_EARG;
    if (n < 0 || first < 0 || label < 0) return sr_fail(ctx, "qk_uniforms: label, first, n >= 0");
    if (n == 0) return QK_OK;
    if (!u) return sr_fail(ctx, "qk_uniforms: null buffer");
    int rc = sr_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    const int64_t blocks = (n + SR_THREADS - 1) / SR_THREADS;
    hipLaunchKernelGGL(sr_uniforms_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(SR_THREADS), 0,
                       ctx->stream, seed, label, first, n, u);
    return sr_hip(ctx, hipGetLastError(), "sr_uniforms_kernel");
}

int qk_sample_rows_workspace_bytes(int64_t n_rows, int m, int64_t* bytes) {
    if (!bytes || n_rows < 0 || m < 0 || m > 30 || n_rows > (INT64_MAX >> 24) / sr_tiles(m)) return QK_EARG;
    *bytes = n_rows * sr_tiles(m) * (int64_t)sizeof(double);
    return QK_OK;
}

int qk_sample_rows(qk_ctx* ctx, int64_t K, int m, const double* X, int64_t ldx, int64_t n_rows, const double* C,
                   int64_t ldc, const int64_t* draw_off, int64_t n_draws, const double* u, int64_t* x_out,
                   double* w_out, double* row_total, void* work, int64_t work_bytes) {
    if (!ctx) return QK_EARG;
    if (m < 0 || m > 30) return sr_fail(ctx, "qk_sample_rows: m must be in 0..30");
    if (K < 1) return sr_fail(ctx, "qk_sample_rows: K must be at least 1");
    if (n_rows < 0 || n_draws < 0) return sr_fail(ctx, "qk_sample_rows: n_rows >= 0, n_draws >= 0");
    if (ldx < ((int64_t)1 << m)) return sr_fail(ctx, "qk_sample_rows: ldx < 2^m");
    if (ldc < K) return sr_fail(ctx, "qk_sample_rows: ldc < K");
    if (n_rows == 0) {
        if (n_draws) return sr_fail(ctx, "qk_sample_rows: draws without rows");
        return QK_OK;
    }
    if (!X || !C || !draw_off || !row_total || (n_draws && (!u || !x_out || !w_out)))
        return sr_fail(ctx, "qk_sample_rows: null buffer");
    const int t = m < SR_TILE_BITS ? m : SR_TILE_BITS;
    const int64_t n_tiles = sr_tiles(m), n_rb = (n_rows + SR_ROWS - 1) / SR_ROWS;
    if (n_rows > 0x7fffffffLL || n_draws > 0x7fffffffLL || n_rb > 0x7fffffffLL / n_tiles)
        return sr_fail(ctx, "qk_sample_rows: rows, draws or row blocks * tiles exceed the grid limit");
    if (!work || work_bytes < n_rows * n_tiles * (int64_t)sizeof(double))
        return sr_fail(ctx, "qk_sample_rows: workspace too small (qk_sample_rows_workspace_bytes)");
    int rc = sr_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    double* pre = static_cast<double*>(work);
    const dim3 bl(SR_THREADS);
    hipLaunchKernelGGL(sr_tile_sums, dim3((unsigned)(n_rb * n_tiles)), bl, 0, ctx->stream, t, n_tiles, n_rb, K, X, ldx,
                       n_rows, C, ldc, pre);
    rc = sr_hip(ctx, hipGetLastError(), "sr_tile_sums");
    if (rc) return rc;
    hipLaunchKernelGGL(sr_tile_scan, dim3((unsigned)n_rows), bl, 0, ctx->stream, n_tiles, pre, row_total);
    rc = sr_hip(ctx, hipGetLastError(), "sr_tile_scan");
    if (rc || n_draws == 0) return rc;
    hipLaunchKernelGGL(sr_locate, dim3((unsigned)n_draws), bl, 0, ctx->stream, t, n_tiles, K, X, ldx, n_rows, C, ldc,
                       draw_off, u, pre, row_total, x_out, w_out);
    return sr_hip(ctx, hipGetLastError(), "sr_locate");
}

}  // extern "C"
