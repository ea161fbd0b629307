// qknit_dot.hip — batched deterministic fp64 dot of swept rows with a cotangent (gfx950): the per-shift
// work of a parameter-shift gradient ("Gradients").
//
//   out[u] = sum_{i < n} Q[u * ldq + i] * D[(u / per) * ldd + i]          u < units
//
// One read of every element and 2 flops per 16 bytes: the kernel is bound by memory bandwidth.
//
// Stage 1. n is cut into segments of DOT_SEG = 8192 doubles; one workgroup of 256 threads takes one
// (unit, segment) pair. Thread t owns the element pairs p = t + 256 * k, k = 0..15, of its segment (a wave
// instruction covers 1 KiB of consecutive addresses) and keeps two accumulators, one for the even and one
// for the odd element of its pairs, each advanced by one fma per pair in the order of k; elements at and
// beyond n are skipped. The thread's value is even + odd; a wave sums its 64 values by the shuffle tree of
// offsets 32, 16, 8, 4, 2, 1 (lane l takes v[l] + v[l + off]); thread 0 adds the four wave sums from LDS
// in wave order and stores the partial at ws[u * nseg + s].
// Stage 2. One wave per unit: lane l adds the partials l, l + 64, ... in index order, then the same
// shuffle tree; lane 0 stores out[u].
//
// Determinism. No atomics. Which elements meet in which order is fixed by n alone: units, per, the grid
// and the neighbouring units do not enter, so a unit has the same bits alone and inside any batch. A pair
// is read by one 16-byte load where the operand's base and leading dimension are even multiples of 8 bytes
// (checked per operand on the host), else by two 8-byte loads; the arithmetic is the same instruction
// sequence on the same values, so the aligned and the misaligned form agree bit for bit. The longest
// chain of additions that an element passes through is 16 + 1 + 6 + 3 in stage 1 and ceil(nseg / 64) + 6
// in stage 2.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "internal.h"

namespace {

constexpr int DOT_THREADS = 256;
constexpr int DOT_PAIRS = 16;                            // pairs per thread and segment
constexpr int64_t DOT_SEG = 2 * DOT_THREADS * DOT_PAIRS;  // 8192 doubles

__device__ __forceinline__ double dot_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum
}

// elements i, i + 1 of a row; i is even, and with VEC the row is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void dot_load(const double* __restrict__ row, int64_t i, int64_t n, double& a, double& b) {
    if (VEC && i + 1 < n) {
        const double2 v = *reinterpret_cast<const double2*>(row + i);
        a = v.x;
        b = v.y;
    } else {
        a = row[i];
        b = i + 1 < n ? row[i + 1] : 0.0;
    }
}

template <bool VQ, bool VD>
__global__ __launch_bounds__(DOT_THREADS) void rows_dot_partial_kernel(int64_t per, int64_t n, int64_t nseg,
                                                                       const double* __restrict__ Q, int64_t ldq,
                                                                       const double* __restrict__ D, int64_t ldd,
                                                                       double* __restrict__ ws) {
    __shared__ double wsum[DOT_THREADS / 64];
    const int64_t g = blockIdx.x;
    const int64_t u = g / nseg, s = g - u * nseg;
    const double* __restrict__ q = Q + u * ldq;
    const double* __restrict__ d = D + (u / per) * ldd;
    const int64_t i0 = s * DOT_SEG + 2 * (int64_t)threadIdx.x;

    double qa[DOT_PAIRS], qb[DOT_PAIRS], da[DOT_PAIRS], db[DOT_PAIRS];
#pragma unroll
    for (int k = 0; k < DOT_PAIRS; ++k) {
        const int64_t i = i0 + (int64_t)k * (2 * DOT_THREADS);
        qa[k] = qb[k] = da[k] = db[k] = 0.0;
        if (i < n) {
            dot_load<VQ>(q, i, n, qa[k], qb[k]);
            dot_load<VD>(d, i, n, da[k], db[k]);
        }
    }
    double even = 0.0, odd = 0.0;
#pragma unroll
    for (int k = 0; k < DOT_PAIRS; ++k) {
        const int64_t i = i0 + (int64_t)k * (2 * DOT_THREADS);
        if (i < n) even = fma(qa[k], da[k], even);
        if (i + 1 < n) odd = fma(qb[k], db[k], odd);
    }
    const double w = dot_wave_sum(even + odd);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) ws[g] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(DOT_THREADS) void rows_dot_final_kernel(int64_t units, int64_t nseg,
                                                                     const double* __restrict__ ws,
                                                                     double* __restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * (DOT_THREADS / 64) + (threadIdx.x >> 6);
    if (u >= units) return;  // whole waves leave: no barrier follows
    const int lane = threadIdx.x & 63;
    const double* __restrict__ p = ws + u * nseg;
    double acc = 0.0;
    for (int64_t j = lane; j < nseg; j += 64) acc = acc + p[j];
    acc = dot_wave_sum(acc);
    if (lane == 0) out[u] = acc;
}

int dot_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int dot_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

bool dot_aligned(const double* p, int64_t ld) { return ((uintptr_t)p & 15u) == 0 && (ld & 1) == 0; }

}  // namespace

extern "C" {

int qk_rows_dot_workspace_bytes(int64_t units, int64_t n, int64_t* bytes) {
    if (!bytes || units < 0 || n < 1) return QK_EARG;
    const int64_t nseg = (n + DOT_SEG - 1) / DOT_SEG;
    if (units > (INT64_MAX >> 4) / nseg) return QK_EARG;
    *bytes = units * nseg * (int64_t)sizeof(double);
    return QK_OK;
}

int qk_rows_dot(qk_ctx* ctx, int64_t units, int64_t per, int64_t n, const double* Q, int64_t ldq, const double* D,
                int64_t ldd, double* out, void* ws, int64_t ws_bytes) {
    if (!ctx) return QK_EARG;
    if (units < 0) return dot_fail(ctx, "qk_rows_dot: units >= 0");
    if (per < 1) return dot_fail(ctx, "qk_rows_dot: per >= 1");
    if (units % per != 0) return dot_fail(ctx, "qk_rows_dot: units must be a multiple of per");
    if (n < 1) return dot_fail(ctx, "qk_rows_dot: n >= 1");
    if (ldq < n) return dot_fail(ctx, "qk_rows_dot: ldq < n");
    if (ldd < n) return dot_fail(ctx, "qk_rows_dot: ldd < n");
    if (!Q || !D || !out) return dot_fail(ctx, "qk_rows_dot: null buffer");
    int64_t need = 0;
    if (qk_rows_dot_workspace_bytes(units, n, &need) != QK_OK || units > (INT64_MAX >> 4) / ldq ||
        units / per > (INT64_MAX >> 4) / ldd)
        return dot_fail(ctx, "qk_rows_dot: units * ld overflows");
    if (units == 0) return QK_OK;
    if (!ws || ws_bytes < need) return dot_fail(ctx, "qk_rows_dot: workspace too short (qk_rows_dot_workspace_bytes)");
    if (((uintptr_t)Q | (uintptr_t)D | (uintptr_t)out | (uintptr_t)ws) & 7u)
        return dot_fail(ctx, "qk_rows_dot: buffers must be 8-byte aligned");
    const int64_t nseg = (n + DOT_SEG - 1) / DOT_SEG;
    const int64_t grid = units * nseg;
    if (grid > 0x7fffffffLL) return dot_fail(ctx, "qk_rows_dot: units * ceil(n / 8192) exceeds the grid limit");
    int rc = dot_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    const bool vq = dot_aligned(Q, ldq), vd = dot_aligned(D, ldd);
    auto kernel = vq ? (vd ? rows_dot_partial_kernel<true, true> : rows_dot_partial_kernel<true, false>)
                     : (vd ? rows_dot_partial_kernel<false, true> : rows_dot_partial_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(DOT_THREADS), 0, ctx->stream, per, n, nseg, Q, ldq, D, ldd,
                       (double*)ws);
    rc = dot_hip(ctx, hipGetLastError(), "rows_dot_partial_kernel");
    if (rc) return rc;
    const int64_t per_block = DOT_THREADS / 64;
    hipLaunchKernelGGL(rows_dot_final_kernel, dim3((unsigned)((units + per_block - 1) / per_block)), dim3(DOT_THREADS), 0,
                       ctx->stream, units, nseg, (const double*)ws, out);
    return dot_hip(ctx, hipGetLastError(), "rows_dot_final_kernel");
}

}  // extern "C"
