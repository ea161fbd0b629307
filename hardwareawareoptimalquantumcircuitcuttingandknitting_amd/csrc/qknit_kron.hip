// qknit_kron.hip — a real 2x2 matrix per outcome bit, applied to every row (gfx950): per-clbit channels on
// the knit, e.g. readout error and its mitigation ("Per-clbit channels").
//
//   dst[r * ld_dst + y] = sum_{x < 2^m} prod_{b < m} coef[b][2 * y_b + x_b] * src[r * ld_src + x]
//
// The sibling of qk_wht_rows (qknit_wht.hip), which is the special case coef[b] = {1, 1, 1, -1} for every b:
// the same tile of 2^13 doubles per workgroup of 512 threads, the same passes (wh_schedule: pass 0 the low
// min(m, 13) bits src -> dst, then at most 9 strided bits per pass in place on dst) and the same walk of
// the element index over (lane, wave, register slot), see that file. What differs is the butterfly: with a
// the element whose bit is clear and b the one whose bit is set,
//
//   (a, b) -> (c[0] a + c[1] b, c[2] a + c[3] b)
//
// and c depends on the bit. A pass carries the matrices of its (at most 13) bits by value in its kernel
// argument, indexed by the bit of the element index: no device allocation, no host synchronisation. A bit
// whose matrix is the identity is not touched (uniform branches, as the inactive bits of a Walsh-Hadamard
// pass); a pass without any other bit is not launched, except pass 0 when it has to copy src to dst.
//
// Rounding. Every output of a butterfly is fma(c_own, own, round(c_other * other)), `own` being the input
// that stands where the output goes: two roundings on one term, one on the other, whether the bit lives in
// a register slot or in the lane index. After the m bits an output lies within gamma_{2m} of the exact sum
// taken with |coef| and |src|.
//
// Determinism. No atomics; an output is the root of a radix-2 tree whose shape and operand order are fixed
// by m and the set of non-identity bits alone: bits in the order 9 10 11 12 4 5 0 1 2 3 6 7 8 of each pass.
// Rows, grid and neighbours do not enter, and in place equals out of place.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "internal.h"
#include "kron_plan.h"

namespace {

// register bit B
template <int B>
__device__ __forceinline__ void kr_bfly(double (&v)[WH_E], const double (&c)[4]) {
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
#pragma unroll
    for (int r = 0; r < WH_E; ++r) {
        if (r & (1 << B)) continue;
        const double a = v[r], b = v[r | (1 << B)];
        v[r] = __builtin_fma(c0, a, c1 * b);
        v[r | (1 << B)] = __builtin_fma(c3, b, c2 * a);
    }
}

// lane bit L: the lane with the bit clear holds a and forms the y = 0 output, its partner holds b
template <int L>
__device__ __forceinline__ void kr_lane_bfly(double (&v)[WH_E], bool set, const double (&c)[4]) {
    const double c_own = set ? c[3] : c[0], c_other = set ? c[2] : c[1];
#pragma unroll
    for (int r = 0; r < WH_E; ++r) {
        const double p = __shfl_xor(v[r], 1 << L, 64);
        v[r] = __builtin_fma(c_own, v[r], c_other * p);
    }
}

// src and dst may be the same buffer: no __restrict__
__global__ __launch_bounds__(WH_THREADS) void kron2_pass_kernel(kr_pass k, int64_t rows, const double* src,
                                                                int64_t ld_src, double* dst, int64_t ld_dst) {
    __shared__ double tile[1 << WH_TILE_BITS];
    const wh_pass& p = k.p;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const kr_origin o = kr_tile_origin(p, blockIdx.x);

    double v[WH_E];
#pragma unroll
    for (int j = 0; j < WH_E; ++j) {
        int64_t row, col;
        kr_element(p, o, ((uint32_t)j << 9) | tid, row, col);
        v[j] = row < rows ? src[row * ld_src + col] : 0.0;
    }

    if (p.active & (1u << 9)) kr_bfly<0>(v, k.c[9]);
    if (p.active & (1u << 10)) kr_bfly<1>(v, k.c[10]);
    if (p.active & (1u << 11)) kr_bfly<2>(v, k.c[11]);
    if (p.active & (1u << 12)) kr_bfly<3>(v, k.c[12]);
    wh_xchg<0, 4>(v);  // register bit 0: e4, lane bit 4: e9
    wh_xchg<1, 5>(v);  // register bit 1: e5, lane bit 5: e10
    if (p.active & (1u << 4)) kr_bfly<0>(v, k.c[4]);
    if (p.active & (1u << 5)) kr_bfly<1>(v, k.c[5]);
    if (p.active & (1u << 0)) kr_lane_bfly<0>(v, lane & 1u, k.c[0]);
    if (p.active & (1u << 1)) kr_lane_bfly<1>(v, lane & 2u, k.c[1]);
    if (p.active & (1u << 2)) kr_lane_bfly<2>(v, lane & 4u, k.c[2]);
    if (p.active & (1u << 3)) kr_lane_bfly<3>(v, lane & 8u, k.c[3]);

    // the LDS transpose of qknit_wht.hip: written at e, read back as e = lane + 64 * j + 1024 * wave
    const uint32_t ebase = (lane & 15u) | (wave << 6) | (((lane >> 4) & 1u) << 9) | ((lane >> 5) << 10);
#pragma unroll
    for (int j = 0; j < WH_E; ++j)
        tile[ebase | ((uint32_t)(j & 3) << 4) | ((uint32_t)(j >> 2) << 11)] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WH_E; ++j) v[j] = tile[lane | ((uint32_t)j << 6) | (wave << 10)];

    if (p.active & (1u << 6)) kr_bfly<0>(v, k.c[6]);
    if (p.active & (1u << 7)) kr_bfly<1>(v, k.c[7]);
    if (p.active & (1u << 8)) kr_bfly<2>(v, k.c[8]);

#pragma unroll
    for (int j = 0; j < WH_E; ++j) {
        int64_t row, col;
        kr_element(p, o, lane | ((uint32_t)j << 6) | (wave << 10), row, col);
        if (row < rows) dst[row * ld_dst + col] = v[j];
    }
}

int kr_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

}  // namespace

extern "C" {

int qk_kron2_rows(qk_ctx* ctx, int64_t rows, int m, const double* coef, const double* src, int64_t ld_src,
                  double* dst, int64_t ld_dst) {
    if (!ctx) return QK_EARG;
    kr_plan plan;
    if (const char* msg = kr_make_plan(rows, m, coef, src, ld_src, dst, ld_dst, &plan)) {
        ctx->err = msg;
        return QK_EARG;
    }
    if (rows == 0) return QK_OK;
    int rc = kr_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    for (int i = 0; i < plan.n_pass; ++i) {
        if (!plan.launch[i]) continue;
        const double* from = i == 0 ? src : dst;
        const int64_t ld_from = i == 0 ? ld_src : ld_dst;
        hipLaunchKernelGGL(kron2_pass_kernel, dim3((unsigned)plan.grid), dim3(WH_THREADS), 0, ctx->stream,
                           plan.pass[i], rows, from, ld_from, dst, ld_dst);
        rc = kr_hip(ctx, hipGetLastError(), "kron2_pass_kernel");
        if (rc) return rc;
    }
    return QK_OK;
}

}  // extern "C"
