// qknit_lookup.hip — the knit at chosen keys (gfx950): probabilities of given bitstrings without the 2^N
// output ("Probabilities at chosen keys").
//
//   qk_transpose_rows   Xt[x * ldt + k] = X[k * ldx + x]  for k < K, x < 2^m;  0.0 for K <= k < ldt
//   qk_knit_at          out[j] = sum_{k < K} prod_{f < F} Xt_f[x_f(j) * ldt + k],  bit i of x_f(j) = bit pos_f[i] of keys[j]
//
// Layout. After the transposition the K factors a key takes from one fragment are one contiguous row of
// 8 * ldt bytes, ldt = K rounded up to a multiple of 16 doubles (128 bytes); the pad columns hold exact
// zeros in every fragment, so the lookup has no tail predicate and a padded term adds +0.0.
//
// qk_transpose_rows: tiles of 32 x 32 doubles through LDS (row pitch 33: the column reads of a tile hit 32
// distinct 8-byte banks), 256 threads, 8-byte loads and stores in runs of 32 lanes = 256 contiguous bytes
// on both sides. A bit-exact permutation plus the zero pad.
//
// qk_knit_at: a group of 16 lanes per key, 4 keys per wave, 16 per workgroup of 256 threads, LK_U = 2 keys
// in flight per group, a grid-stride loop over the keys.
//   split   lane f < F of the group forms x_f for its fragment: the position table is cut into runs of
//           consecutive positions on the host (src bit, dst bit, length), staged in LDS once per workgroup;
//           a fragment whose clbits are contiguous in the key is one shift and mask. The other lanes
//           fetch x_f with a 16-lane __shfl.
//   gather  lane l takes k = l, l + 16, ...: a group's load of one fragment row is runs of 128 contiguous
//           bytes. Chunks of 16 k are taken LK_C = 4 at a time (one __shfl per fragment and 4 chunks).
//
// Association (fixed by K, F and ldt alone; n, j and the neighbouring keys do not enter):
//   term(k)  = ((X_0 * X_1) * X_2) * ...            the fragments in ascending order
//   lane(l)  = (((0 + term(l)) + term(l + 16)) + term(l + 32)) + ...   k ascending, up to ldt
//   out      = the xor butterfly over the 16 lanes with partners 8, 4, 2, 1 in this order
//              (a + b is commutative, so every lane of the group holds the same bits; lane 0 stores).
// A key with a `dead` bit set stores exactly 0.0. No atomics; the operands and the keys are only read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace {

constexpr int TR_TILE = 32;
constexpr int TR_THREADS = 256;

constexpr int LK_THREADS = 256;
constexpr int LK_LANES = 16;                       // lanes per key
constexpr int LK_GROUPS = LK_THREADS / LK_LANES;   // keys per workgroup and step
constexpr int LK_U = 2;                            // keys in flight per group
constexpr int LK_C = 4;                            // chunks of 16 terms per fragment fetch
constexpr int LK_MAX_F = QK_KNIT_AT_MAX_FRAGMENTS;
constexpr int LK_MAX_BITS = 62;
constexpr int LK_MAX_BLOCKS = 2048;                // 8 workgroups of 4 waves on each of 256 CUs

__global__ __launch_bounds__(TR_THREADS) void lk_transpose_kernel(int64_t K, int64_t W, const double* __restrict__ X,
                                                                  int64_t ldx, double* __restrict__ Xt, int64_t ldt) {
    __shared__ double tile[TR_TILE][TR_TILE + 1];
    const int tx = threadIdx.x & (TR_TILE - 1), ty = threadIdx.x / TR_TILE;  // ty < 8
    const int64_t x0 = (int64_t)blockIdx.x * TR_TILE, k0 = (int64_t)blockIdx.y * TR_TILE;
#pragma unroll
    for (int i = 0; i < TR_TILE; i += TR_THREADS / TR_TILE) {
        const int64_t k = k0 + ty + i, x = x0 + tx;
        tile[ty + i][tx] = (k < K && x < W) ? X[k * ldx + x] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TR_TILE; i += TR_THREADS / TR_TILE) {
        const int64_t x = x0 + ty + i, k = k0 + tx;
        if (x < W && k < ldt) Xt[x * ldt + k] = tile[tx][ty + i];
    }
}

// a run of consecutive key bits: x |= ((key >> src) & (2^len - 1)) << dst
struct lk_params {
    const double* xt[LK_MAX_F];
    uint32_t run[LK_MAX_BITS];      // src | dst << 8 | len << 16
    uint8_t run_off[LK_MAX_F + 1];  // fragment f owns run[run_off[f] .. run_off[f + 1])
    int F;
    int64_t chunks;                 // ldt / 16
    int64_t ldt;
    uint64_t dead;
};

__global__ __launch_bounds__(LK_THREADS) void lk_knit_at_kernel(lk_params p, const int64_t* __restrict__ keys, int64_t n,
                                                                double* __restrict__ out) {
    __shared__ uint32_t s_run[LK_MAX_BITS];
    __shared__ uint32_t s_off[LK_MAX_F + 1];
    if (threadIdx.x < LK_MAX_BITS) s_run[threadIdx.x] = p.run[threadIdx.x];
    if (threadIdx.x <= LK_MAX_F) s_off[threadIdx.x] = p.run_off[threadIdx.x];
    __syncthreads();

    const int l = threadIdx.x & (LK_LANES - 1);
    const int64_t group = (int64_t)blockIdx.x * LK_GROUPS + threadIdx.x / LK_LANES;
    const int64_t n_groups = (int64_t)gridDim.x * LK_GROUPS;
    const uint32_t r0 = l < p.F ? s_off[l] : 0u, r1 = l < p.F ? s_off[l + 1] : 0u;

    // every lane stays active through the loop (the shuffles need their partners): a group past the end
    // works on key 0 and does not store
    for (int64_t base = group; base < n; base += n_groups * LK_U) {
        uint64_t key[LK_U];
        int x[LK_U];
#pragma unroll
        for (int u = 0; u < LK_U; ++u) {
            const int64_t j = base + u * n_groups;
            key[u] = j < n ? (uint64_t)keys[j] : 0ull;
            x[u] = 0;
        }
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t run = s_run[r];
            const uint32_t src = run & 0xffu, dst = (run >> 8) & 0xffu, len = run >> 16;
#pragma unroll
            for (int u = 0; u < LK_U; ++u) x[u] |= (int)(((uint32_t)(key[u] >> src) & ((1u << len) - 1u)) << dst);
        }

        double acc[LK_U];
#pragma unroll
        for (int u = 0; u < LK_U; ++u) acc[u] = 0.0;
        for (int64_t c0 = 0; c0 < p.chunks; c0 += LK_C) {
            double term[LK_U][LK_C];
            for (int f = 0; f < p.F; ++f) {
                const double* xt = p.xt[f] + c0 * LK_LANES + l;
#pragma unroll
                for (int u = 0; u < LK_U; ++u) {
                    const double* row = xt + (int64_t)__shfl(x[u], f, LK_LANES) * p.ldt;
#pragma unroll
                    for (int c = 0; c < LK_C; ++c) {
                        if (c0 + c < p.chunks) {
                            const double v = row[c * LK_LANES];
                            term[u][c] = f == 0 ? v : term[u][c] * v;
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < LK_C; ++c) {
                if (c0 + c < p.chunks) {
#pragma unroll
                    for (int u = 0; u < LK_U; ++u) acc[u] += term[u][c];
                }
            }
        }

#pragma unroll
        for (int u = 0; u < LK_U; ++u) {
            double a = acc[u];
            a += __shfl_xor(a, 8, LK_LANES);
            a += __shfl_xor(a, 4, LK_LANES);
            a += __shfl_xor(a, 2, LK_LANES);
            a += __shfl_xor(a, 1, LK_LANES);
            const int64_t j = base + u * n_groups;
            if (l == 0 && j < n) out[j] = (key[u] & p.dead) ? 0.0 : a;
        }
    }
}

int lk_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int lk_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

}  // namespace

extern "C" {

int qk_transpose_rows(qk_ctx* ctx, int64_t K, int m, const double* X, int64_t ldx, double* Xt, int64_t ldt) {
    if (!ctx) return QK_EARG;
    if (m < 0 || m > 30) return lk_fail(ctx, "qk_transpose_rows: m must be in 0..30");
    if (K < 1) return lk_fail(ctx, "qk_transpose_rows: K must be at least 1");
    const int64_t W = (int64_t)1 << m;
    if (ldx < W) return lk_fail(ctx, "qk_transpose_rows: ldx < 2^m");
    if (ldt < K || ldt % 16) return lk_fail(ctx, "qk_transpose_rows: ldt must be a multiple of 16, at least K");
    if (!X || !Xt) return lk_fail(ctx, "qk_transpose_rows: null buffer");
    if (K > (INT64_MAX >> 4) / ldx || ldt > (INT64_MAX >> 4) / W)
        return lk_fail(ctx, "qk_transpose_rows: K * ldx or 2^m * ldt overflows");
    const int64_t gx = (W + TR_TILE - 1) / TR_TILE, gy = (ldt + TR_TILE - 1) / TR_TILE;
    if (gy > 65535) return lk_fail(ctx, "qk_transpose_rows: ldt exceeds the grid limit (32 * 65535)");
    int rc = lk_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    hipLaunchKernelGGL(lk_transpose_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(TR_THREADS), 0, ctx->stream, K, W, X,
                       ldx, Xt, ldt);
    return lk_hip(ctx, hipGetLastError(), "lk_transpose_kernel");
}

int qk_knit_at(qk_ctx* ctx, int F, int64_t K, int64_t ldt, const double* const* Xt, const int* m, const int* pos,
               const int64_t* keys, int64_t n, uint64_t dead, double* out) {
    if (!ctx) return QK_EARG;
    if (F < 1 || F > LK_MAX_F) return lk_fail(ctx, "qk_knit_at: F must be in 1..16");
    if (K < 1) return lk_fail(ctx, "qk_knit_at: K must be at least 1");
    if (ldt < K || ldt % 16) return lk_fail(ctx, "qk_knit_at: ldt must be a multiple of 16, at least K");
    if (n < 0) return lk_fail(ctx, "qk_knit_at: n >= 0");
    if (!Xt || !m) return lk_fail(ctx, "qk_knit_at: null buffer");
    lk_params p = {};
    int total = 0, n_runs = 0;
    for (int f = 0; f < F; ++f) {
        if (m[f] < 0 || m[f] > 30) return lk_fail(ctx, "qk_knit_at: m must be in 0..30");
        if (ldt > (INT64_MAX >> 4) >> m[f]) return lk_fail(ctx, "qk_knit_at: 2^m * ldt overflows");
        if (!Xt[f]) return lk_fail(ctx, "qk_knit_at: null buffer");
        total += m[f];
    }
    if (total > LK_MAX_BITS) return lk_fail(ctx, "qk_knit_at: more than 62 bits over the fragments");
    if (total && !pos) return lk_fail(ctx, "qk_knit_at: null buffer");
    for (int f = 0, at = 0; f < F; at += m[f], ++f) {
        p.xt[f] = Xt[f];
        p.run_off[f] = (uint8_t)n_runs;
        for (int i = 0; i < m[f]; ++i) {
            const int b = pos[at + i];
            if (b < 0 || b > 62) return lk_fail(ctx, "qk_knit_at: a position outside 0..62");
            if (i && b == pos[at + i - 1] + 1)
                p.run[n_runs - 1] += 1u << 16;  // the run goes on
            else
                p.run[n_runs++] = (uint32_t)b | ((uint32_t)i << 8) | (1u << 16);
        }
    }
    p.run_off[F] = (uint8_t)n_runs;
    p.F = F;
    p.ldt = ldt;
    p.chunks = ldt / LK_LANES;
    p.dead = dead;
    if (n == 0) return QK_OK;
    if (!keys || !out) return lk_fail(ctx, "qk_knit_at: null buffer");
    int rc = lk_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    const int64_t steps = (n + (int64_t)LK_GROUPS * LK_U - 1) / ((int64_t)LK_GROUPS * LK_U);
    const unsigned grid = (unsigned)(steps < LK_MAX_BLOCKS ? steps : LK_MAX_BLOCKS);
    hipLaunchKernelGGL(lk_knit_at_kernel, dim3(grid), dim3(LK_THREADS), 0, ctx->stream, p, keys, n, out);
    return lk_hip(ctx, hipGetLastError(), "lk_knit_at_kernel");
}

}  // extern "C"
