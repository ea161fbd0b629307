// qknit_obs.hip — bit reductions of swept rows (gfx950): marginals and Z-string parities of a
// fragment's distributions without the 2^N knit output ("Reductions of the knit").
//
//   dst[r][j * 2^k + y] = sum over x in [0, 2^m) with pext(x, keep) == y of
//                         (-1)^popcount(x & flip[j]) * src[r * ld_src + x]
//
// Layout. A row is cut into tiles of T = 2^t consecutive x (t = min(m, 10)); x = tile * T + xl. A
// workgroup of 256 threads owns one (row, y_hi) — y_hi = the kept bits of the tile index — and walks
// the tiles that share it (the dropped high bits, ascending) in a fixed order. Thread tid holds the
// elements xl = e * 256 + tid (e < 4) of the current tile: one coalesced 8-byte load per lane, every
// source element read once per launch. For each of the launch's NB <= 16 flip masks it keeps its own
// accumulators acc[j][e] in registers (NB * 4 doubles) and adds the loaded values with the sign
//   parity(x & flip) = parity(tile * T & flip)   (per tile: uniform, scalar unit)
//                    ^ parity(tid & flip)        (per lane: one bit per mask, formed once per launch)
//                    ^ the bits 8, 9 of xl       (per register slot: applied in the butterfly below)
// so no popcount is formed per element and mask.
//
// After the walk the dropped bits of xl are summed out, lowest level first and in a fixed order:
//   bits 8, 9 (register slots)  acc[e] += +-acc[e | bit]            in registers
//   bits 0..5 (lanes)           v += shfl_xor(v, bit)                across the wave (both lanes of a
//                                                                    pair form the same a + b)
//   bits 6, 7 (waves)           through LDS: the holders write red[xl], the output threads sum the
//                               dropped wave bits ascending
// Kept low bits take no step at all: consecutive y are consecutive x there and the output threads
// read consecutive LDS words and write consecutive outputs. With k = m nothing is added: the values
// pass through unchanged (first-tile assignment, so a -0.0 stays -0.0).
//
// Splitting. With few (row, y_hi) groups the walk over the dropped high bits is cut into S equal
// chunks (S a power of two chosen from the shape alone: the smallest with groups * S >= 256) that
// run as workgroups of their own and write partials into the workspace; reduce_bits_stage2 sums the
// S partials of an output in ascending chunk order. No atomics anywhere: the order of every sum
// depends on (rows, m, keep, n_flips) only, and two launches give identical bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace {

constexpr int RB_TILE_BITS = 10;  // tile of 2^10 doubles: 4 per thread
constexpr int RB_THREADS = 256;
constexpr int RB_E = 4;
constexpr int RB_BATCH = QK_REDUCE_BITS_BATCH;
constexpr uint32_t RB_WAVE_BITS = 0xC0u;  // bits of xl that select the wave
constexpr int64_t RB_MIN_GROUPS = 256;    // split the walk until this many workgroups exist

struct rb_flips {
    uint32_t f[RB_BATCH];
};

struct rb_shape {
    int t, klo, khi, dhi;
    uint32_t keep_lo, drop_lo, keep_hi, drop_hi;
    int64_t groups, split;  // rows * 2^khi, S
};

rb_shape rb_make_shape(int64_t rows, int m, uint64_t keep) {
    rb_shape s;
    s.t = m < RB_TILE_BITS ? m : RB_TILE_BITS;
    const uint32_t lo = (1u << s.t) - 1u, hi = (1u << (m - s.t)) - 1u;
    s.keep_lo = (uint32_t)keep & lo;
    s.drop_lo = ~(uint32_t)keep & lo;
    s.keep_hi = (uint32_t)(keep >> s.t) & hi;
    s.drop_hi = ~(uint32_t)(keep >> s.t) & hi;
    s.klo = __builtin_popcount(s.keep_lo);
    s.khi = __builtin_popcount(s.keep_hi);
    s.dhi = __builtin_popcount(s.drop_hi);
    s.groups = rows << s.khi;
    s.split = 1;
    while (s.groups * s.split < RB_MIN_GROUPS && s.split < ((int64_t)1 << s.dhi)) s.split *= 2;
    return s;
}

__device__ __forceinline__ uint32_t rb_pdep(uint32_t v, uint32_t mask) {
    uint32_t out = 0;
    while (mask) {
        const uint32_t low = mask & (0u - mask);
        if (v & 1u) out |= low;
        v >>= 1;
        mask ^= low;
    }
    return out;
}

template <int NB>
__global__ __launch_bounds__(RB_THREADS) void reduce_bits_kernel(rb_shape sh, int nb, rb_flips fl,
                                                                 const double* __restrict__ src, int64_t ld_src,
                                                                 int k, int64_t j0, double* __restrict__ dst,
                                                                 int64_t ld_dst, double* __restrict__ part) {
    __shared__ double red[2][1 << RB_TILE_BITS];
    const int tid = threadIdx.x;
    const uint32_t T = 1u << sh.t;
    int64_t g = blockIdx.x;
    const int64_t s = g % sh.split;
    g /= sh.split;
    const uint32_t yhi = (uint32_t)(g & (((int64_t)1 << sh.khi) - 1));
    const int64_t r = g >> sh.khi;
    const uint32_t base_hi = rb_pdep(yhi, sh.keep_hi);
    const uint32_t chunk = (1u << sh.dhi) / (uint32_t)sh.split;
    uint32_t sub = rb_pdep((uint32_t)s * chunk, sh.drop_hi);

    uint32_t lanebits = 0;  // bit j: parity(tid & flip[j])
#pragma unroll
    for (int j = 0; j < NB; ++j) lanebits |= (uint32_t)(__popc((uint32_t)tid & fl.f[j]) & 1) << j;

    double acc[NB][RB_E];
    const double* row = src + r * ld_src;
    for (uint32_t it = 0; it < chunk; ++it) {
        const uint32_t tile = base_hi | sub;
        const double* p = row + ((int64_t)tile << sh.t);
        double v[RB_E];
#pragma unroll
        for (int e = 0; e < RB_E; ++e) {
            const uint32_t xl = (uint32_t)e * RB_THREADS + tid;
            v[e] = xl < T ? p[xl] : 0.0;
        }
        const uint32_t tbase = tile << sh.t;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const uint32_t neg = ((lanebits >> j) ^ (uint32_t)__popc(tbase & fl.f[j])) & 1u;
#pragma unroll
            for (int e = 0; e < RB_E; ++e) {
                const double sv = neg ? -v[e] : v[e];
                acc[j][e] = it == 0 ? sv : acc[j][e] + sv;
            }
        }
        sub = ((sub | ~sh.drop_hi) + 1u) & sh.drop_hi;  // next subset of the dropped high bits, ascending
    }

    // dropped bits 8, 9: register slots
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if ((sh.drop_lo >> (8 + b)) & 1u) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const bool neg = (fl.f[j] >> (8 + b)) & 1u;
#pragma unroll
                for (int e = 0; e < RB_E; ++e)
                    if (!(e & (1 << b))) acc[j][e] += neg ? -acc[j][e | (1 << b)] : acc[j][e | (1 << b)];
            }
        }
    }
    // dropped bits 0..5: lanes of the wave (signs are applied already)
    for (int b = 0; b < 6; ++b) {
        if ((sh.drop_lo >> b) & 1u) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int e = 0; e < RB_E; ++e) acc[j][e] += __shfl_xor(acc[j][e], 1 << b, 64);
        }
    }

    // dropped bits 6, 7 (waves) and the compaction onto the kept bits, through LDS
    const uint32_t wdrop = sh.drop_lo & RB_WAVE_BITS;
    const uint32_t n_out = 1u << sh.klo;
    uint32_t x0[RB_E];
#pragma unroll
    for (int o = 0; o < RB_E; ++o) x0[o] = rb_pdep((uint32_t)o * RB_THREADS + tid, sh.keep_lo);
    const int64_t gs = g * sh.split + s;  // (group, chunk) index of this workgroup's partials
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j < nb) {
            double* buf = red[j & 1];
#pragma unroll
            for (int e = 0; e < RB_E; ++e) {
                const uint32_t xl = (uint32_t)e * RB_THREADS + tid;
                if (xl < T && (xl & sh.drop_lo & ~RB_WAVE_BITS) == 0) buf[xl] = acc[j][e];
            }
            __syncthreads();
#pragma unroll
            for (int o = 0; o < RB_E; ++o) {
                const uint32_t oi = (uint32_t)o * RB_THREADS + tid;
                if (oi < n_out) {
                    double sum = buf[x0[o]];
                    for (uint32_t w = ((0u | ~wdrop) + 1u) & wdrop; w; w = ((w | ~wdrop) + 1u) & wdrop)
                        sum += buf[x0[o] | w];
                    if (sh.split == 1)
                        dst[r * ld_dst + ((j0 + j) << k) + (((int64_t)yhi << sh.klo) | oi)] = sum;
                    else
                        part[((gs * nb + j) << sh.klo) + oi] = sum;
                }
            }
        }
    }
}

// dst[r][(j0 + j) * 2^k + y] = sum_{s < S} part[(((r * 2^khi + y_hi) * S + s) * nb + j) * 2^klo + y_lo], s ascending
__global__ __launch_bounds__(RB_THREADS) void reduce_bits_stage2(rb_shape sh, int nb, int64_t rows, int k, int64_t j0,
                                                                 const double* __restrict__ part,
                                                                 double* __restrict__ dst, int64_t ld_dst) {
    const int64_t total = (rows * nb) << k;
    for (int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RB_THREADS) {
        const int64_t y = i & (((int64_t)1 << k) - 1);
        const int64_t rj = i >> k, j = rj % nb, r = rj / nb;
        const int64_t yhi = y >> sh.klo, oi = y & (((int64_t)1 << sh.klo) - 1);
        const int64_t g = (r << sh.khi) | yhi;
        const double* p = part + (((g * sh.split) * nb + j) << sh.klo) + oi;
        const int64_t step = (int64_t)nb << sh.klo;
        double sum = p[0];
        for (int64_t s = 1; s < sh.split; ++s) sum += p[s * step];
        dst[r * ld_dst + ((j0 + j) << k) + y] = sum;
    }
}

int rb_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int rb_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

int64_t rb_work_bytes(const rb_shape& sh, int64_t n_flips) {
    if (sh.split == 1) return 0;
    const int64_t nb = n_flips < RB_BATCH ? n_flips : RB_BATCH;
    return ((sh.groups * sh.split * nb) << sh.klo) * (int64_t)sizeof(double);
}

}  // namespace

extern "C" {

int qk_reduce_bits_workspace_bytes(int64_t rows, int m, uint64_t keep_mask, int64_t n_flips, int64_t* bytes) {
    if (!bytes || rows < 0 || m < 0 || m > 30 || n_flips < 1 || (keep_mask >> m) != 0) return QK_EARG;
    *bytes = rb_work_bytes(rb_make_shape(rows, m, keep_mask), n_flips);
    return QK_OK;
}

int qk_reduce_bits(qk_ctx* ctx, int64_t rows, int m, const double* src, int64_t ld_src, uint64_t keep_mask,
                   int64_t n_flips, const uint64_t* flip_masks, double* dst, int64_t ld_dst, void* work,
                   int64_t work_bytes) {
    if (!ctx) return QK_EARG;
    if (m < 0 || m > 30) return rb_fail(ctx, "qk_reduce_bits: m must be in 0..30");
    if (rows < 0 || n_flips < 1) return rb_fail(ctx, "qk_reduce_bits: rows >= 0, n_flips >= 1");
    if ((keep_mask >> m) != 0) return rb_fail(ctx, "qk_reduce_bits: keep_mask has bits at or above m");
    if (!flip_masks) return rb_fail(ctx, "qk_reduce_bits: null flip_masks");
    for (int64_t j = 0; j < n_flips; ++j) {
        if ((flip_masks[j] >> m) != 0) return rb_fail(ctx, "qk_reduce_bits: flip mask has bits at or above m");
        if (flip_masks[j] & keep_mask) return rb_fail(ctx, "qk_reduce_bits: flip mask overlaps keep_mask");
    }
    const int k = __builtin_popcountll(keep_mask);
    if (ld_src < ((int64_t)1 << m)) return rb_fail(ctx, "qk_reduce_bits: ld_src < 2^m");
    if (n_flips > (INT64_MAX >> (k + 4)) || ld_dst < (n_flips << k))
        return rb_fail(ctx, "qk_reduce_bits: ld_dst < n_flips * 2^k");
    if (!src || !dst) return rb_fail(ctx, "qk_reduce_bits: null buffer");
    if (rows == 0) return QK_OK;
    const rb_shape sh = rb_make_shape(rows, m, keep_mask);
    const int64_t need = rb_work_bytes(sh, n_flips);
    if (need > 0 && (!work || work_bytes < need))
        return rb_fail(ctx, "qk_reduce_bits: workspace too small (qk_reduce_bits_workspace_bytes)");
    const int64_t grid = sh.groups * sh.split;
    if (grid > 0x7fffffffLL) return rb_fail(ctx, "qk_reduce_bits: rows * 2^(kept high bits) exceeds the grid limit");
    int rc = rb_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    double* part = static_cast<double*>(work);
    for (int64_t j0 = 0; j0 < n_flips; j0 += RB_BATCH) {
        const int nb = (int)(n_flips - j0 < RB_BATCH ? n_flips - j0 : RB_BATCH);
        rb_flips fl;
        for (int j = 0; j < RB_BATCH; ++j) fl.f[j] = j < nb ? (uint32_t)flip_masks[j0 + j] : 0u;
        const dim3 gr((unsigned)grid), bl(RB_THREADS);
        if (nb == 1)
            hipLaunchKernelGGL(reduce_bits_kernel<1>, gr, bl, 0, ctx->stream, sh, nb, fl, src, ld_src, k, j0, dst, ld_dst,
                               part);
        else if (nb <= 4)
            hipLaunchKernelGGL(reduce_bits_kernel<4>, gr, bl, 0, ctx->stream, sh, nb, fl, src, ld_src, k, j0, dst, ld_dst,
                               part);
        else
            hipLaunchKernelGGL(reduce_bits_kernel<RB_BATCH>, gr, bl, 0, ctx->stream, sh, nb, fl, src, ld_src, k, j0, dst,
                               ld_dst, part);
        rc = rb_hip(ctx, hipGetLastError(), "reduce_bits_kernel");
        if (rc) return rc;
        if (sh.split > 1) {
            const int64_t total = (rows * nb) << k, blocks = (total + RB_THREADS - 1) / RB_THREADS;
            const unsigned g2 = (unsigned)(blocks < 1 ? 1 : (blocks < 4096 ? blocks : 4096));
            hipLaunchKernelGGL(reduce_bits_stage2, dim3(g2), bl, 0, ctx->stream, sh, nb, rows, k, j0, part, dst, ld_dst);
            rc = rb_hip(ctx, hipGetLastError(), "reduce_bits_stage2");
            if (rc) return rc;
        }
    }
    return QK_OK;
}

}  // extern "C"
