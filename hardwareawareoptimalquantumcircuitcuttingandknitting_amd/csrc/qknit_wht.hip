// qknit_wht.hip — row-wise Walsh-Hadamard transform over outcome bits (gfx950): every Z-string parity
// of a fragment's rows at once ("All Z strings: the Walsh-Hadamard spectrum").
//
//   dst[r * ld_dst + z] = sum_{x < 2^m} (-1)^popcount(x & z) * src[r * ld_src + x]        (unnormalised)
//
// Passes. A workgroup of 512 threads owns a tile of 2^13 doubles, 16 per thread, and transforms up to 13
// bits of the index in one read and one write of every element:
//   pass 0      the low t0 = min(m, 13) bits of contiguous tiles (src -> dst); with m < 13 a tile holds
//               2^(13 - m) whole rows;
//   pass i > 0  the next nb_i <= 9 bits (dst -> dst, in place): a tile is 2^c consecutive indices
//               (c = 13 - nb_i >= 4, runs of at least 128 bytes) times 2^nb_i indices of stride 2^lo_i.
// The m - t0 high bits are spread evenly over ceil((m - t0) / 9) later passes (wh_schedule): one pass
// for m <= 13, two for m <= 22, three for m <= 30. Every workgroup reads its whole tile before it writes
// any of it and the tiles of a pass are disjoint, so src == dst is as good as two buffers.
//
// Inside a tile the element index e (13 bits) sits on (lane, wave, register slot j):
//   load        e = j * 512 + tid: bits 0..5 lane, 6..8 wave, 9..12 register      (coalesced 8-byte loads)
//   bits 9..12  add / sub butterflies between register slots
//   bits 4, 5   v_permlane16_swap / v_permlane32_swap trade register bits 0, 1 (e9, e10) for lane bits
//               4, 5; then register butterflies again. The slots are not traded back: e9, e10 stay on
//               the lanes and the LDS index below accounts for it.
//   bits 0..3   __shfl_xor with the partner lane: the lane with the bit clear forms a + b, the other a - b
//   bits 6..8   one LDS transpose: written at e, read back as e = lane + 64 * j + 1024 * wave, so bits
//               6..9 are register bits. Writes are 16-lane runs of consecutive doubles and reads 64-lane
//               runs, which is conflict-free for 8-byte LDS accesses without padding.
//   store       from that layout: 64 consecutive e per wave and slot.
// Bits outside the pass's range are skipped (uniform branches); the data movement is the same.
//
// Determinism. No atomics; an output is the root of a radix-2 tree of depth m whose shape and operand
// order (the element with the bit clear is the left operand) are fixed by m alone: bits in the order
// 9 10 11 12 4 5 0 1 2 3 6 7 8 of each pass. Rows, grid and neighbours do not enter.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"
#include "wh_tile.h"  // the tile, wh_pass / wh_schedule, wh_xchg

namespace {

template <int B>
__device__ __forceinline__ void wh_bfly(double (&v)[WH_E]) {
#pragma unroll
    for (int r = 0; r < WH_E; ++r) {
        if (r & (1 << B)) continue;
        const double a = v[r], b = v[r | (1 << B)];
        v[r] = a + b;
        v[r | (1 << B)] = a - b;
    }
}

template <int L>
__device__ __forceinline__ void wh_lane_bfly(double (&v)[WH_E], bool set) {
#pragma unroll
    for (int r = 0; r < WH_E; ++r) {
        const double p = __shfl_xor(v[r], 1 << L, 64);
        v[r] = set ? p - v[r] : v[r] + p;
    }
}

// src and dst may be the same buffer: no __restrict__
__global__ __launch_bounds__(WH_THREADS) void wht_pass_kernel(wh_pass p, int64_t rows, const double* src,
                                                              int64_t ld_src, double* dst, int64_t ld_dst) {
    __shared__ double tile[1 << WH_TILE_BITS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int64_t g = blockIdx.x;
    const int64_t row0 = (g >> p.tbits) << p.rowshift;
    const int64_t t = g & (((int64_t)1 << p.tbits) - 1);
    const int64_t u = t & (((int64_t)1 << p.ubits) - 1), h = t >> p.ubits;
    const int64_t colbase = (h << p.hshift) | (u << p.ushift);

    double v[WH_E];
#pragma unroll
    for (int j = 0; j < WH_E; ++j) {
        const uint32_t e = ((uint32_t)j << 9) | tid;
        const int64_t row = row0 + (e >> p.rshift);
        const int64_t col = colbase + (e & p.cmask) + ((int64_t)(e >> p.cshift) << p.lo);
        v[j] = row < rows ? src[row * ld_src + col] : 0.0;
    }

    if (p.active & (1u << 9)) wh_bfly<0>(v);
    if (p.active & (1u << 10)) wh_bfly<1>(v);
    if (p.active & (1u << 11)) wh_bfly<2>(v);
    if (p.active & (1u << 12)) wh_bfly<3>(v);
    wh_xchg<0, 4>(v);  // register bit 0: e4, lane bit 4: e9
    wh_xchg<1, 5>(v);  // register bit 1: e5, lane bit 5: e10
    if (p.active & (1u << 4)) wh_bfly<0>(v);
    if (p.active & (1u << 5)) wh_bfly<1>(v);
    if (p.active & (1u << 0)) wh_lane_bfly<0>(v, lane & 1u);
    if (p.active & (1u << 1)) wh_lane_bfly<1>(v, lane & 2u);
    if (p.active & (1u << 2)) wh_lane_bfly<2>(v, lane & 4u);
    if (p.active & (1u << 3)) wh_lane_bfly<3>(v, lane & 8u);

    const uint32_t ebase = (lane & 15u) | (wave << 6) | (((lane >> 4) & 1u) << 9) | ((lane >> 5) << 10);
#pragma unroll
    for (int j = 0; j < WH_E; ++j)
        tile[ebase | ((uint32_t)(j & 3) << 4) | ((uint32_t)(j >> 2) << 11)] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WH_E; ++j) v[j] = tile[lane | ((uint32_t)j << 6) | (wave << 10)];

    if (p.active & (1u << 6)) wh_bfly<0>(v);
    if (p.active & (1u << 7)) wh_bfly<1>(v);
    if (p.active & (1u << 8)) wh_bfly<2>(v);

#pragma unroll
    for (int j = 0; j < WH_E; ++j) {
        const uint32_t e = lane | ((uint32_t)j << 6) | (wave << 10);
        const int64_t row = row0 + (e >> p.rshift);
        const int64_t col = colbase + (e & p.cmask) + ((int64_t)(e >> p.cshift) << p.lo);
        if (row < rows) dst[row * ld_dst + col] = v[j];
    }
}

int wh_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int wh_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

}  // namespace

extern "C" {

int qk_wht_rows(qk_ctx* ctx, int64_t rows, int m, const double* src, int64_t ld_src, double* dst, int64_t ld_dst) {
    if (!ctx) return QK_EARG;
    if (m < 0 || m > 30) return wh_fail(ctx, "qk_wht_rows: m must be in 0..30");
    if (rows < 0) return wh_fail(ctx, "qk_wht_rows: rows >= 0");
    const int64_t n = (int64_t)1 << m;
    if (ld_src < n) return wh_fail(ctx, "qk_wht_rows: ld_src < 2^m");
    if (ld_dst < n) return wh_fail(ctx, "qk_wht_rows: ld_dst < 2^m");
    if (!src || !dst) return wh_fail(ctx, "qk_wht_rows: null buffer");
    if (rows == 0) return QK_OK;
    if (rows > (INT64_MAX >> 4) / ld_src || rows > (INT64_MAX >> 4) / ld_dst)
        return wh_fail(ctx, "qk_wht_rows: rows * ld overflows");
    if (!(src == dst && ld_src == ld_dst)) {
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((rows - 1) * ld_src + n) * sizeof(double);
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((rows - 1) * ld_dst + n) * sizeof(double);
        if (s0 < d1 && d0 < s1)
            return wh_fail(ctx, "qk_wht_rows: src and dst overlap (only src == dst with equal ld is in place)");
    }
    wh_pass passes[1 + WH_MAX_PASSES];
    const int n_pass = wh_schedule(m, passes);
    const int64_t per_tile = (int64_t)1 << passes[0].rowshift;
    const int64_t grid = ((rows + per_tile - 1) / per_tile) << passes[0].tbits;
    if (grid > 0x7fffffffLL) return wh_fail(ctx, "qk_wht_rows: rows * 2^(m - 13) exceeds the grid limit");
    int rc = wh_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    for (int i = 0; i < n_pass; ++i) {
        const double* from = i == 0 ? src : dst;
        const int64_t ld_from = i == 0 ? ld_src : ld_dst;
        hipLaunchKernelGGL(wht_pass_kernel, dim3((unsigned)grid), dim3(WH_THREADS), 0, ctx->stream, passes[i], rows, from,
                           ld_from, dst, ld_dst);
        rc = wh_hip(ctx, hipGetLastError(), "wht_pass_kernel");
        if (rc) return rc;
    }
    return QK_OK;
}

}  // extern "C"
