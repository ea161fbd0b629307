// qknit_scan.hip — nonlinear functionals of the knit without its 2^N output (gfx950; DESIGN.md §4a,
// "Nonlinear functionals: the streamed scan").
//
//   qk_knit_scan      R[i][j] = sum_{k<K} A[k][i] B[k][j] for i in [i_begin, i_end), j < 2^mb is formed tile by
//                     tile on the fp64 matrix cores and consumed in registers: sums, extrema and their flat
//                     indices (i << mb | j), counts and a histogram of binades; with a second knit R' on the same
//                     (i, j) also the cross terms (sum R R', Hellinger sum, L1 and max difference).
//   qk_knit_collect   the same mainloop; appends (flat index, R) of every output with R > tau.
//   qk_knit_project_scan  the same mainloop; one pass of the nearest-probability-distribution iteration: sums and
//                     counts of the members (|R| > accuracy) and of the kept (R > max(theta, accuracy)), and the
//                     statistics of p = R - theta on the kept; with a second knit also of p' and of the pair.
//   qk_knit_project_tiles  the same mainloop; per tile the mass of p, signed by up to 8 Z masks.
//   qk_knit_project_draw   inverse-CDF draws from p in (tile, walk) order: a prefix over the tile masses, then the
//                     mainloop again on the one tile that a draw falls into.
//
// Layout. A workgroup of 256 threads forms one 128 x 128 tile of R: 2 x 2 waves of 64 x 64 = 4 x 4
// v_mfma_f64_16x16x4_f64 blocks each, K streamed in chunks of 16 rows through a double-buffered LDS stage
// (row pitch 144 doubles, as qk_gemm_keyed's tile kernel), the next chunk's global loads in flight in registers
// during the current chunk's MFMAs, one barrier per chunk. Operands are [K, 2^m] row-major: a thread loads two
// adjacent columns of four chunk rows, as one 16-byte load each where the operand allows it (even ld, 16-byte
// aligned base, even first column, whole tile and chunk in range), else as 8-byte loads. Columns at or past
// i_end / 2^mb and k at or past K are zero-filled in registers on the way to LDS and never read; their outputs
// are masked out of every epilogue.
//
// Decomposition (sc_make_shape; observables.scan_shape is its host model): tiles_m x tiles_n tiles, tile t =
// (t / tiles_n, t % tiles_n), tile rows counted from i_begin; G = min(tiles, 512) workgroups, workgroup g owns
// tiles g, g + G, g + 2G, ...: a function of (mb, i_begin, i_end) alone, not of the device.
//
// Association (fixed by the shape; no floating-point atomics):
//   R[i][j]    the chain acc <- mfma(a, b, acc) from +0.0 over k = 0, 4, 8, ... (missing k are 0.0 * 0.0)
//   thread     adds its outputs tile by tile, ascending, within a tile in the fixed order (block row, block
//              column, register)
//   workgroup  halving tree over its 256 threads' partials in LDS (t += t + 128, 64, ..., 1)
//   result     stage 2 adds the G workgroup partials in ascending order
// Extrema carry the lowest flat index among equals at every step. Counts and the histogram are integers (LDS and
// global integer atomics): independent of order. Two launches give identical bytes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "internal.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_T = 128;              // tile edge
constexpr int SC_K = 16;               // k rows per chunk
constexpr int SC_PITCH = SC_T + 16;    // LDS row pitch, doubles
constexpr int64_t SC_MAX_GROUPS = 512;
constexpr int SC_SLOTS = QK_SCAN_NSTATS;

typedef double sc_d4 __attribute__((ext_vector_type(4)));
typedef double sc_d2 __attribute__((ext_vector_type(2)));

struct sc_shape {
    int64_t tiles_m, tiles_n, tiles, groups;
};

sc_shape sc_make_shape(int mb, int64_t i_begin, int64_t i_end) {
    sc_shape s;
    s.tiles_m = (i_end - i_begin + SC_T - 1) / SC_T;
    s.tiles_n = (((int64_t)1 << mb) + SC_T - 1) / SC_T;
    s.tiles = s.tiles_m * s.tiles_n;
    s.groups = s.tiles < SC_MAX_GROUPS ? s.tiles : SC_MAX_GROUPS;
    return s;
}

int64_t sc_work_bytes(const sc_shape& sh) { return sh.groups * (SC_SLOTS + 2) * 8; }

struct ScanArgs {
    int K;
    const double* __restrict__ A;
    int64_t lda;
    const double* __restrict__ B;
    int64_t ldb;
    int K2;
    const double* __restrict__ A2;
    int64_t lda2;
    const double* __restrict__ B2;
    int64_t ldb2;
    int64_t i_begin, i_end, N;
    int mb;
    sc_shape sh;
    double tau;
    double* __restrict__ pstats;   // [SC_SLOTS][groups]
    int64_t* __restrict__ pidx;    // [2][groups]: flat index of the workgroup's maximum, of its minimum
    unsigned long long* __restrict__ counts;  // [0] > tau, [1] > 0 (zeroed before the launch)
    unsigned long long* __restrict__ hist;    // [QK_SCAN_BINS] or null (zeroed before the launch)
    // collect
    int64_t capacity;
    int64_t* __restrict__ idx;
    double* __restrict__ vals;
    unsigned long long* __restrict__ count;
};

// This thread's share of chunk rows [k0, k0 + 16) of columns [c0, c0 + 128): rows k0 + (tid >> 6) + 4 v,
// columns c0 + 2 (tid & 63) + {0, 1}; zero where k >= K or the column >= cols.
__device__ __forceinline__ void sc_load(sc_d2 (&r)[4], const double* __restrict__ X, int64_t ld, int k0, int K,
                                        int64_t c0, int64_t cols) {
    const int rl = threadIdx.x >> 6, cl = 2 * (threadIdx.x & 63);
    const double* p = X + (int64_t)(k0 + rl) * ld + c0 + cl;
    const bool vec = ((ld | c0) & 1) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && c0 + SC_T <= cols &&
                     k0 + SC_K <= K;  // workgroup-uniform
    if (vec) {
#pragma unroll
        for (int v = 0; v < 4; ++v) r[v] = *reinterpret_cast<const sc_d2*>(p + 4 * v * ld);
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const bool rv = k0 + rl + 4 * v < K;
            r[v].x = (rv && c0 + cl < cols) ? p[4 * v * ld] : 0.0;
            r[v].y = (rv && c0 + cl + 1 < cols) ? p[4 * v * ld + 1] : 0.0;
        }
    }
}

// acc = the 128 x 128 tile of X^T Y at rows m0 (of X's columns, below m_end) and columns n0 (of Y's, below N).
// `buf`: the LDS buffer the next store goes to; it alternates per chunk across tiles, so a buffer is rewritten only
// after the barrier that follows its last read.
__device__ __forceinline__ void sc_tile(const double* __restrict__ X, int64_t ldx, const double* __restrict__ Y,
                                        int64_t ldy, int K, int64_t m0, int64_t m_end, int64_t n0, int64_t N,
                                        sc_d4 (&acc)[4][4], double (*As)[SC_K][SC_PITCH],
                                        double (*Bs)[SC_K][SC_PITCH], int& buf) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (sc_d4){0.0, 0.0, 0.0, 0.0};
    const int lr = tid >> 6, lc = 2 * (tid & 63);
    sc_d2 ra[4], rb[4];
    sc_load(ra, X, ldx, 0, K, m0, m_end);
    sc_load(rb, Y, ldy, 0, K, n0, N);
    for (int k0 = 0; k0 < K; k0 += SC_K) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            *reinterpret_cast<sc_d2*>(&As[buf][lr + 4 * v][lc]) = ra[v];
            *reinterpret_cast<sc_d2*>(&Bs[buf][lr + 4 * v][lc]) = rb[v];
        }
        __syncthreads();
        if (k0 + SC_K < K) {
            sc_load(ra, X, ldx, k0 + SC_K, K, m0, m_end);
            sc_load(rb, Y, ldy, k0 + SC_K, K, n0, N);
        }
        // a short last chunk runs all four k-steps: its rows at or past K hold zeros, and acc + 0.0 * 0.0 = acc
#pragma unroll
        for (int kk = 0; kk < SC_K / 4; ++kk) {
            const int kr = kk * 4 + (lane >> 4);
            double fa[4], fb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fa[t] = As[buf][kr][wm * 64 + t * 16 + (lane & 15)];
                fb[t] = Bs[buf][kr][wn * 64 + t * 16 + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        buf ^= 1;
    }
}

// Output (i, j, r) of this lane: row m0 + wm 64 + 16 i + (lane >> 4) + 4 r, column n0 + wn 64 + 16 j + (lane & 15).
__device__ __forceinline__ int64_t sc_row(int64_t m0, int i, int r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return m0 + (wave & 1) * 64 + i * 16 + (lane >> 4) + 4 * r;
}
__device__ __forceinline__ int64_t sc_col(int64_t n0, int j) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return n0 + (wave >> 1) * 64 + j * 16 + (lane & 15);
}

template <bool PAIR, bool ENT, bool HIST>
__global__ __launch_bounds__(SC_THREADS, PAIR ? 1 : 2) void knit_scan_kernel(ScanArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][SC_K][SC_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[2][SC_K][SC_PITCH];
    __shared__ unsigned long long shist[QK_SCAN_BINS];
    __shared__ unsigned long long scount[2];
    __shared__ unsigned long long sarg[2];
    static_assert(sizeof(As) >= sizeof(double) * SC_SLOTS * SC_THREADS, "the reduction scratch aliases As");
    const int tid = threadIdx.x, lane = tid & 63;
    if (HIST && tid < QK_SCAN_BINS) shist[tid] = 0;
    if (tid < 2) {
        scount[tid] = 0;
        sarg[tid] = ~0ull;
    }
    double st[SC_SLOTS];
#pragma unroll
    for (int s = 0; s < SC_SLOTS; ++s) st[s] = 0.0;
    st[QK_SCAN_MAX] = -INFINITY;
    st[QK_SCAN_MIN] = INFINITY;
    int64_t imax = INT64_MAX, imin = INT64_MAX;
    unsigned long long n_tau = 0, n_pos = 0;
    int buf = 0;
    __syncthreads();

    for (int64_t t = blockIdx.x; t < a.sh.tiles; t += gridDim.x) {
        const int64_t m0 = a.i_begin + (t / a.sh.tiles_n) * SC_T, n0 = (t % a.sh.tiles_n) * SC_T;
        sc_d4 acc[4][4];
        sc_d4 acc2[PAIR ? 4 : 1][PAIR ? 4 : 1];
        if constexpr (PAIR) {
            sc_tile(a.A2, a.lda2, a.B2, a.ldb2, a.K2, m0, a.i_end, n0, a.N, acc2, As, Bs, buf);
        }
        sc_tile(a.A, a.lda, a.B, a.ldb, a.K, m0, a.i_end, n0, a.N, acc, As, Bs, buf);
        bool cok[4];
        int64_t col[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            col[j] = sc_col(n0, j);
            cok[j] = col[j] < a.N;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = sc_row(m0, i, r);
                    const bool ok = row < a.i_end && cok[j];
                    const double v = acc[i][j][r];
                    const int64_t flat = (row << a.mb) | col[j];
                    if (ok) {
                        const double p = v > 0.0 ? v : 0.0;
                        st[QK_SCAN_SUM] += v;
                        st[QK_SCAN_ABS] += fabs(v);
                        st[QK_SCAN_POS] += p;
                        st[QK_SCAN_SQ] = fma(v, v, st[QK_SCAN_SQ]);
                        if (ENT) st[QK_SCAN_ENT] += v > 0.0 ? -(p * log(p)) : 0.0;
                        if (v > st[QK_SCAN_MAX] || (v == st[QK_SCAN_MAX] && flat < imax)) {
                            st[QK_SCAN_MAX] = v;
                            imax = flat;
                        }
                        if (v < st[QK_SCAN_MIN] || (v == st[QK_SCAN_MIN] && flat < imin)) {
                            st[QK_SCAN_MIN] = v;
                            imin = flat;
                        }
                        n_tau += v > a.tau ? 1 : 0;
                        n_pos += v > 0.0 ? 1 : 0;
                        if constexpr (PAIR) {
                            const double w = acc2[i][j][r];
                            const double q = w > 0.0 ? w : 0.0;
                            const double d = fabs(v - w);
                            st[QK_SCAN_SUM2] += w;
                            st[QK_SCAN_POS2] += q;
                            st[QK_SCAN_CROSS] = fma(v, w, st[QK_SCAN_CROSS]);
                            st[QK_SCAN_HELL] += sqrt(p * q);
                            st[QK_SCAN_L1D] += d;
                            st[QK_SCAN_MAXD] = d > st[QK_SCAN_MAXD] ? d : st[QK_SCAN_MAXD];
                        }
                    }
                    if constexpr (HIST) {
                        // bin = clamp(-ilogb(v), 0, 127) from the exponent field (a denormal reads -1023: bin 127)
                        int bin = -1;
                        if (ok && v > 0.0) {
                            const int e = 1023 - (int)((__double_as_longlong(v) >> 52) & 0x7ff);
                            bin = e < 0 ? 0 : (e > QK_SCAN_BINS - 1 ? QK_SCAN_BINS - 1 : e);
                        }
                        // one LDS atomic per distinct bin of the wave
                        unsigned long long todo = __ballot(bin >= 0);
                        while (todo) {
                            const int leader = __ffsll((long long)todo) - 1;
                            const int b = __shfl(bin, leader);
                            const unsigned long long same = __ballot(bin == b);
                            if (lane == leader) atomicAdd(&shist[b], (unsigned long long)__popcll(same));
                            todo &= ~same;
                        }
                    }
                }
    }

    // workgroup: halving tree over the threads' partials; the extrema's indices by an integer minimum over the
    // threads that hold the extreme value
    __syncthreads();  // the last tile's LDS reads are done: As becomes the scratch
    double(*red)[SC_THREADS] = reinterpret_cast<double(*)[SC_THREADS]>(&As[0][0][0]);
#pragma unroll
    for (int s = 0; s < SC_SLOTS; ++s) red[s][tid] = st[s];
    __syncthreads();
    for (int h = SC_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int s = 0; s < SC_SLOTS; ++s) {
                const double x = red[s][tid], y = red[s][tid + h];
                red[s][tid] = (s == QK_SCAN_MAX || s == QK_SCAN_MAXD) ? (y > x ? y : x)
                              : s == QK_SCAN_MIN                       ? (y < x ? y : x)
                                                                       : x + y;
            }
        }
        __syncthreads();
    }
    if (st[QK_SCAN_MAX] == red[QK_SCAN_MAX][0]) atomicMin(&sarg[0], (unsigned long long)imax);
    if (st[QK_SCAN_MIN] == red[QK_SCAN_MIN][0]) atomicMin(&sarg[1], (unsigned long long)imin);
    if (n_tau) atomicAdd(&scount[0], n_tau);
    if (n_pos) atomicAdd(&scount[1], n_pos);
    __syncthreads();
    const int64_t G = gridDim.x, g = blockIdx.x;
    if (tid < SC_SLOTS) a.pstats[tid * G + g] = red[tid][0];
    if (tid < 2) {
        a.pidx[tid * G + g] = (int64_t)sarg[tid];
        if (scount[tid]) atomicAdd(&a.counts[tid], scount[tid]);
    }
    if (HIST && tid < QK_SCAN_BINS && shist[tid]) atomicAdd(&a.hist[tid], shist[tid]);
}

// stats[s] = the G partials of slot s combined in ascending workgroup order; counts[2], counts[3] = the flat
// indices of the maximum and of the minimum (lowest index among equal values).
__global__ __launch_bounds__(SC_THREADS) void knit_scan_stage2(int64_t G, const double* __restrict__ pstats,
                                                               const int64_t* __restrict__ pidx, int pair, int ent,
                                                               double* __restrict__ stats,
                                                               int64_t* __restrict__ counts) {
    __shared__ double sv[SC_SLOTS][SC_MAX_GROUPS];
    __shared__ int64_t si[2][SC_MAX_GROUPS];
    const int tid = threadIdx.x;
    for (int64_t e = tid; e < SC_SLOTS * G; e += SC_THREADS) sv[e / G][e % G] = pstats[e];
    for (int64_t e = tid; e < 2 * G; e += SC_THREADS) si[e / G][e % G] = pidx[e];
    __syncthreads();
    if (tid < SC_SLOTS) {
        const int s = tid;
        double x = sv[s][0];
        if (s == QK_SCAN_MAX || s == QK_SCAN_MIN) {
            const bool mx = s == QK_SCAN_MAX;
            int64_t at = si[mx ? 0 : 1][0];
            for (int64_t g = 1; g < G; ++g) {
                const double y = sv[s][g];
                const int64_t yi = si[mx ? 0 : 1][g];
                if ((mx ? y > x : y < x) || (y == x && yi < at)) {
                    x = y;
                    at = yi;
                }
            }
            counts[mx ? QK_SCAN_ARGMAX : QK_SCAN_ARGMIN] = at;
        } else if (s == QK_SCAN_MAXD) {
            for (int64_t g = 1; g < G; ++g) x = sv[s][g] > x ? sv[s][g] : x;
        } else {
            for (int64_t g = 1; g < G; ++g) x += sv[s][g];
        }
        const bool pair_slot = s >= QK_SCAN_SUM2 && s <= QK_SCAN_MAXD;
        if ((pair_slot && !pair) || (s == QK_SCAN_ENT && !ent) || s > QK_SCAN_MAXD) x = 0.0;
        stats[s] = x;
    }
}

__global__ __launch_bounds__(SC_THREADS, 2) void knit_collect_kernel(ScanArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][SC_K][SC_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[2][SC_K][SC_PITCH];
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    int buf = 0;
    for (int64_t t = blockIdx.x; t < a.sh.tiles; t += gridDim.x) {
        const int64_t m0 = a.i_begin + (t / a.sh.tiles_n) * SC_T, n0 = (t % a.sh.tiles_n) * SC_T;
        sc_d4 acc[4][4];
        sc_tile(a.A, a.lda, a.B, a.ldb, a.K, m0, a.i_end, n0, a.N, acc, As, Bs, buf);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = sc_row(m0, i, r), col = sc_col(n0, j);
                    const double v = acc[i][j][r];
                    const bool keep = row < a.i_end && col < a.N && v > a.tau;
                    const unsigned long long m = __ballot(keep);
                    if (m) {  // wave-uniform
                        unsigned long long base = 0;
                        if (lane == 0) base = atomicAdd(a.count, (unsigned long long)__popcll(m));
                        base = __shfl(base, 0);
                        if (keep) {
                            const int64_t at = (int64_t)base + __popcll(m & below);
                            if (at < a.capacity) {
                                a.idx[at] = (row << a.mb) | col;
                                a.vals[at] = v;
                            }
                        }
                    }
                }
    }
}

// ---- one pass of the nearest-probability-distribution iteration ("Nearest probability
// distribution"): the scan's mainloop, another epilogue. The single-knit variant carries the six slots of the first
// knit only; the pair variant all fifteen.
constexpr int PJ_SLOTS = QK_PROJ_NSTATS;
constexpr int PJ_SINGLE = QK_PROJ_PMAX + 1;
constexpr int PJ_PAIR = QK_PROJ_MAXD + 1;

struct ProjArgs {
    int K;
    const double* __restrict__ A;
    int64_t lda;
    const double* __restrict__ B;
    int64_t ldb;
    int K2;
    const double* __restrict__ A2;
    int64_t lda2;
    const double* __restrict__ B2;
    int64_t ldb2;
    int64_t i_begin, i_end, N;
    int mb;
    sc_shape sh;
    double accuracy, theta, lower, theta2, lower2;  // lower = max(theta, accuracy)
    double* __restrict__ pstats;              // [PJ_SLOTS][groups]
    int64_t* __restrict__ pidx;               // [groups]: flat index of the workgroup's PMAX
    int ent_slot;                             // knit_project_entropy_kernel: the slot it fills
    unsigned long long* __restrict__ counts;  // NMEMBER, NKEPT, NMEMBER2, NKEPT2 (zeroed before the launch)
};

__device__ __forceinline__ bool pj_is_max(int s) {
    return s == QK_PROJ_PMAX || s == QK_PROJ_PMAX2 || s == QK_PROJ_MAXD;
}

// Everything but the entropy slots. The counts leave the registers after every tile (a wave sum, then one LDS
// atomic per wave) and the pair variant's sums wait in LDS while the mainloop runs, so that neither holds vector
// registers across it.
template <bool PAIR>
__global__ __launch_bounds__(SC_THREADS, PAIR ? 1 : 2) void knit_project_kernel(ProjArgs a) {
    constexpr int NS = PAIR ? PJ_PAIR : PJ_SINGLE;
    constexpr int NPARK = PAIR ? NS : 0;
    __shared__ __attribute__((aligned(16))) double As[2][SC_K][SC_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[2][SC_K][SC_PITCH];
    __shared__ double park[NPARK ? NPARK : 1][SC_THREADS];
    __shared__ unsigned long long scount[4];
    __shared__ unsigned long long sarg;
    static_assert(sizeof(As) >= sizeof(double) * PJ_PAIR * SC_THREADS, "the reduction scratch aliases As");
    const int tid = threadIdx.x;
    if (tid < 4) scount[tid] = 0;
    if (tid == 0) sarg = ~0ull;
    double st[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) st[s] = 0.0;
    st[QK_PROJ_PMAX] = -INFINITY;  // every output has a p >= 0: the first one replaces it
    int64_t imax = INT64_MAX;
    int buf = 0;
#pragma unroll
    for (int s = 0; s < NPARK; ++s) park[s][tid] = st[s];
    __syncthreads();

    for (int64_t t = blockIdx.x; t < a.sh.tiles; t += gridDim.x) {
        const int64_t m0 = a.i_begin + (t / a.sh.tiles_n) * SC_T, n0 = (t % a.sh.tiles_n) * SC_T;
        sc_d4 acc[4][4];
        sc_d4 acc2[PAIR ? 4 : 1][PAIR ? 4 : 1];
        if constexpr (PAIR) {
            sc_tile(a.A2, a.lda2, a.B2, a.ldb2, a.K2, m0, a.i_end, n0, a.N, acc2, As, Bs, buf);
        }
        sc_tile(a.A, a.lda, a.B, a.ldb, a.K, m0, a.i_end, n0, a.N, acc, As, Bs, buf);
#pragma unroll
        for (int s = 0; s < NPARK; ++s) st[s] = park[s][tid];
        unsigned cnt[PAIR ? 2 : 1] = {};  // of this tile, per knit: members (at most 64) | kept << 16
        bool cok[4];
        int64_t col[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            col[j] = sc_col(n0, j);
            cok[j] = col[j] < a.N;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = sc_row(m0, i, r);
                    if (!(row < a.i_end && cok[j])) continue;
                    const double v = acc[i][j][r];
                    const int64_t flat = (row << a.mb) | col[j];
                    const bool mem = fabs(v) > a.accuracy, kept = v > a.lower;
                    const double p = kept ? v - a.theta : 0.0;
                    st[QK_PROJ_MSUM] += mem ? v : 0.0;
                    st[QK_PROJ_TSUM] += kept ? v : 0.0;
                    st[QK_PROJ_PSUM] += p;
                    st[QK_PROJ_PSQ] = fma(p, p, st[QK_PROJ_PSQ]);
                    if (p > st[QK_PROJ_PMAX] || (p == st[QK_PROJ_PMAX] && flat < imax)) {
                        st[QK_PROJ_PMAX] = p;
                        imax = flat;
                    }
                    cnt[0] += (mem ? 1u : 0u) | (kept ? 0x10000u : 0u);
                    if constexpr (PAIR) {
                        const double w = acc2[i][j][r];
                        const bool mem2 = fabs(w) > a.accuracy, kept2 = w > a.lower2;
                        const double q = kept2 ? w - a.theta2 : 0.0;
                        const double d = fabs(p - q);
                        st[QK_PROJ_MSUM2] += mem2 ? w : 0.0;
                        st[QK_PROJ_TSUM2] += kept2 ? w : 0.0;
                        st[QK_PROJ_PSUM2] += q;
                        st[QK_PROJ_PSQ2] = fma(q, q, st[QK_PROJ_PSQ2]);
                        st[QK_PROJ_PMAX2] = q > st[QK_PROJ_PMAX2] ? q : st[QK_PROJ_PMAX2];
                        st[QK_PROJ_HELL] += sqrt(p * q);
                        st[QK_PROJ_L1D] += d;
                        st[QK_PROJ_MAXD] = d > st[QK_PROJ_MAXD] ? d : st[QK_PROJ_MAXD];
                        cnt[1] += (mem2 ? 1u : 0u) | (kept2 ? 0x10000u : 0u);
                    }
                }
#pragma unroll
        for (int c = 0; c < (PAIR ? 2 : 1); ++c) {
            unsigned n = cnt[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);  // of the wave: at most 4096 in either half
            if ((tid & 63) == 0 && n) {
                atomicAdd(&scount[2 * c], (unsigned long long)(n & 0xffffu));
                atomicAdd(&scount[2 * c + 1], (unsigned long long)(n >> 16));
            }
        }
#pragma unroll
        for (int s = 0; s < NPARK; ++s) park[s][tid] = st[s];
    }

    // workgroup: the scan's halving tree; the index of PMAX by an integer minimum over the threads that hold it
    __syncthreads();  // the last tile's LDS reads are done: As becomes the scratch
    double(*red)[SC_THREADS] = reinterpret_cast<double(*)[SC_THREADS]>(&As[0][0][0]);
#pragma unroll
    for (int s = 0; s < NS; ++s) red[s][tid] = st[s];
    __syncthreads();
    for (int h = SC_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double x = red[s][tid], y = red[s][tid + h];
                red[s][tid] = pj_is_max(s) ? (y > x ? y : x) : x + y;
            }
        }
        __syncthreads();
    }
    if (st[QK_PROJ_PMAX] == red[QK_PROJ_PMAX][0]) atomicMin(&sarg, (unsigned long long)imax);
    __syncthreads();
    const int64_t G = gridDim.x, g = blockIdx.x;
    if (tid < NS && tid != QK_PROJ_PENT && tid != QK_PROJ_PENT2) a.pstats[tid * G + g] = red[tid][0];
    if (tid == 0) a.pidx[g] = (int64_t)sarg;
    if (tid < 4 && scount[tid]) atomicAdd(&a.counts[tid], scount[tid]);
}

// One entropy slot (PENT of the first knit, or PENT2 of the second: the entry passes that knit as the first, its
// theta and `ent_slot`), in a launch of its own: the logarithm beside the other sums does not fit the registers
// that the mainloop leaves.
__global__ __launch_bounds__(SC_THREADS, 2) void knit_project_entropy_kernel(ProjArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][SC_K][SC_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[2][SC_K][SC_PITCH];
    const int tid = threadIdx.x;
    double ent = 0.0;
    int buf = 0;
    for (int64_t t = blockIdx.x; t < a.sh.tiles; t += gridDim.x) {
        const int64_t m0 = a.i_begin + (t / a.sh.tiles_n) * SC_T, n0 = (t % a.sh.tiles_n) * SC_T;
        sc_d4 acc[4][4];
        sc_tile(a.A, a.lda, a.B, a.ldb, a.K, m0, a.i_end, n0, a.N, acc, As, Bs, buf);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[i][j][r];
                    const bool kept = sc_row(m0, i, r) < a.i_end && sc_col(n0, j) < a.N && v > a.lower;
                    const double p = kept ? v - a.theta : 0.0;
                    ent += kept ? -(p * log(p)) : 0.0;
                }
    }
    __syncthreads();  // the last tile's LDS reads are done: As becomes the scratch
    double* red = &As[0][0][0];
    red[tid] = ent;
    __syncthreads();
    for (int h = SC_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) a.pstats[a.ent_slot * (int64_t)gridDim.x + blockIdx.x] = red[0];
}

// stats[s] = the G partials of slot s combined in ascending workgroup order (slots past `slots` and the entropy
// slots without the flag: 0.0); counts[QK_PROJ_ARGMAX] = the flat index of PMAX, the lowest among equal values.
__global__ __launch_bounds__(SC_THREADS) void knit_project_stage2(int64_t G, const double* __restrict__ pstats,
                                                                  const int64_t* __restrict__ pidx, int slots, int ent,
                                                                  double* __restrict__ stats,
                                                                  int64_t* __restrict__ counts) {
    __shared__ double sv[PJ_SLOTS][SC_MAX_GROUPS];
    __shared__ int64_t si[SC_MAX_GROUPS];
    const int tid = threadIdx.x;
    for (int64_t e = tid; e < slots * G; e += SC_THREADS) sv[e / G][e % G] = pstats[e];
    for (int64_t e = tid; e < G; e += SC_THREADS) si[e] = pidx[e];
    __syncthreads();
    if (tid < PJ_SLOTS) {
        const int s = tid;
        double x = 0.0;
        if (s < slots && !((s == QK_PROJ_PENT || s == QK_PROJ_PENT2) && !ent)) {
            x = sv[s][0];
            if (s == QK_PROJ_PMAX) {
                int64_t at = si[0];
                for (int64_t g = 1; g < G; ++g) {
                    const double y = sv[s][g];
                    if (y > x || (y == x && si[g] < at)) {
                        x = y;
                        at = si[g];
                    }
                }
                counts[QK_PROJ_ARGMAX] = at;
            } else if (pj_is_max(s)) {
                for (int64_t g = 1; g < G; ++g) x = sv[s][g] > x ? sv[s][g] : x;
            } else {
                for (int64_t g = 1; g < G; ++g) x += sv[s][g];
            }
        }
        stats[s] = x;
    }
}

int64_t pj_work_bytes(const sc_shape& sh) { return sh.groups * (PJ_SLOTS + 1) * 8; }

// ---- the projection as a distribution ("The projection as a distribution"): signed tile masses of
// p and inverse-CDF draws from it, in (tile, walk) order. The walk order of a tile: thread tid ascending, within a
// thread block row i, block column j, register r ascending (the outputs sc_row(m0, i, r), sc_col(n0, j)).
// Association: a thread adds its 64 p in walk order from +0.0; the 256 thread sums are chained serially in tid
// order from +0.0 (b <- b + sum[tid]). The sums wait for the chain in the LDS stage that the mainloop writes next
// (every read of it precedes the last chunk's barrier); `buf` is then flipped, so that the next tile's first store
// goes to the other stage, whose reads precede the barrier before the chain. One barrier per tile, no LDS beyond
// the mainloop's.
constexpr int PT_MASKS = QK_PROJ_TILE_MASKS;
constexpr int PD_MAX_GROUPS = 4096;
constexpr int PD_SPT = 8;  // tiles per thread and chunk of the prefix
static_assert(sizeof(double) * SC_K * SC_PITCH >= sizeof(double) * PT_MASKS * SC_THREADS, "the sums alias one stage");

struct TileArgs {
    int K;
    const double* __restrict__ A;
    int64_t lda;
    const double* __restrict__ B;
    int64_t ldb;
    int64_t i_begin, i_end, N;
    int mb;
    sc_shape sh;
    double theta, lower;  // lower = max(theta, accuracy)
    int n_masks;
    uint32_t za[PT_MASKS], zb[PT_MASKS];
    double* __restrict__ W;  // [n_masks][tiles]
    // draw
    const double* __restrict__ pre;  // [tiles]: inclusive prefix of the plain tile masses
    const double* __restrict__ total;
    int64_t n_draws;
    const double* __restrict__ u;
    int64_t* __restrict__ flat;
    double* __restrict__ pval;
};

// W[m][t] for m < n_masks <= NM; the masks from n_masks on are (0, 0) and are not stored.
template <int NM>
__global__ __launch_bounds__(SC_THREADS, 2) void knit_project_tiles_kernel(TileArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][SC_K][SC_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[2][SC_K][SC_PITCH];
    const int tid = threadIdx.x;
    int buf = 0;
    for (int64_t t = blockIdx.x; t < a.sh.tiles; t += gridDim.x) {
        const int64_t m0 = a.i_begin + (t / a.sh.tiles_n) * SC_T, n0 = (t % a.sh.tiles_n) * SC_T;
        sc_d4 acc[4][4];
        sc_tile(a.A, a.lda, a.B, a.ldb, a.K, m0, a.i_end, n0, a.N, acc, As, Bs, buf);
        // The epilogue's thread index, opaque to the compiler: what it derives from it is formed here, per tile, and
        // does not wait in registers while the mainloop runs.
        int tq = tid;
        asm volatile("" : "+v"(tq));
        // The outputs become their p where they are: no second set of 64 values is ever live. Rows at or past
        // i_end and columns at or past N hold exact zeros (their operands are zero-filled) and lower >= 0: they are
        // never kept.
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[i][j][r];
                    acc[i][j][r] = v > a.lower ? v - a.theta : 0.0;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        double(*red)[SC_THREADS] = reinterpret_cast<double(*)[SC_THREADS]>(&As[buf][0][0]);
        const uint32_t row0 = (uint32_t)m0 + ((tq >> 6) & 1) * 64 + ((tq >> 4) & 3);  // sc_row(m0, i, r) = row0 + 16 i + 4 r
        const uint32_t col0 = (uint32_t)n0 + (tq >> 7) * 64 + (tq & 15);              // sc_col(n0, j) = col0 + 16 j
#pragma unroll
        for (int m = 0; m < NM; ++m) {  // one mask at a time
            // bit 4 i + r of rpar: the parity of this thread's row (i, r) under za[m]; bit j of cpar: of its column j
            // under zb[m]
            uint32_t rpar = 0, cpar = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    rpar |= (uint32_t)(__popc((row0 + 16 * i + 4 * r) & a.za[m]) & 1) << (4 * i + r);
#pragma unroll
            for (int j = 0; j < 4; ++j) cpar |= (uint32_t)(__popc((col0 + 16 * j) & a.zb[m]) & 1) << j;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double p = acc[i][j][r];  // its sign bit flipped where the parity is odd
                        const uint32_t odd = ((rpar >> (4 * i + r)) ^ (cpar >> j)) << 31;
                        s += __hiloint2double(__double2hiint(p) ^ (int)odd, __double2loint(p));
                    }
            red[m][tq] = s;
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (tid < NM && tid < a.n_masks) {
            double b = 0.0;
            for (int th = 0; th < SC_THREADS; ++th) b += red[tid][th];
            a.W[(int64_t)tid * a.sh.tiles + t] = b;
        }
        buf ^= 1;
    }
}

// pre[t] = the inclusive prefix of W[0..t], total = pre[tiles - 1]: sr_tile_scan's serial chain (qknit_shots.hip),
// out of place. Monotone where W >= 0 and flat over empty tiles, which the binary search of the draws needs.
__global__ __launch_bounds__(SC_THREADS) void knit_project_prefix_kernel(int64_t n_tiles, const double* __restrict__ W,
                                                                         double* __restrict__ pre,
                                                                         double* __restrict__ total) {
    __shared__ double part[SC_THREADS];
    __shared__ double carry_s;
    const int tid = threadIdx.x;
    if (tid == 0) carry_s = 0.0;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += (int64_t)SC_THREADS * PD_SPT) {
        double v[PD_SPT];
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < PD_SPT; ++k) {
            const int64_t i = base + (int64_t)tid * PD_SPT + k;
            run += i < n_tiles ? W[i] : 0.0;
            v[k] = run;
        }
        part[tid] = run;
        __syncthreads();
        if (tid == 0) {  // the thread totals chained serially: part[t] becomes the prefix before thread t
            const int64_t left = (n_tiles - base + PD_SPT - 1) / PD_SPT;
            const int used = (int)(left < SC_THREADS ? left : SC_THREADS);
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
        for (int k = 0; k < PD_SPT; ++k) {
            const int64_t i = base + (int64_t)tid * PD_SPT + k;
            if (i < n_tiles) pre[i] = b + v[k];
        }
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;  // bit for bit the last prefix
}

// A value that is the same in every lane but was formed by vector instructions, back in scalar registers.
__device__ __forceinline__ int64_t pd_uniform(int64_t x) {
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}
__device__ __forceinline__ double pd_uniform(double x) { return __longlong_as_double(pd_uniform((int64_t)__double_as_longlong(x))); }

// One workgroup per draw, grid-stride: the first tile whose prefix exceeds u * total, that tile again (sc_tile: the
// bits of the tiles kernel), the threads' sums and their exclusive chain, and the first kept output in walk order
// whose prefix before + (chain + running sum) exceeds the target; if rounding leaves none, the tile's last kept one.
// One workgroup per CU, as the pair kernels: the two walks beside the mainloop's addresses do not fit the 256 registers
// that two would leave each wave.
__global__ __launch_bounds__(SC_THREADS, 1) void knit_project_draw_kernel(TileArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][SC_K][SC_PITCH];
    __shared__ __attribute__((aligned(16))) double Bs[2][SC_K][SC_PITCH];
    __shared__ int first_s[SC_THREADS / 64], last_s[SC_THREADS / 64];
    constexpr int NONE = 1 << 30;
    const int tid = threadIdx.x;
    const double total = *a.total;
    if (!(total > 0.0) || total == INFINITY) {  // the whole grid leaves: nothing to draw from
        for (int64_t d = (int64_t)blockIdx.x * SC_THREADS + tid; d < a.n_draws; d += (int64_t)gridDim.x * SC_THREADS) {
            a.flat[d] = -1;
            a.pval[d] = 0.0;
        }
        return;
    }
    int buf = 0;
    for (int64_t d = blockIdx.x; d < a.n_draws; d += gridDim.x) {
        const double target = pd_uniform(a.u[d] * total);
        int64_t lo = 0, hi = a.sh.tiles - 1;  // the first tile whose inclusive prefix exceeds the target
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.pre[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        const int64_t t = pd_uniform(lo);
        const double before = pd_uniform(t ? a.pre[t - 1] : 0.0);
        const int64_t m0 = a.i_begin + (t / a.sh.tiles_n) * SC_T, n0 = (t % a.sh.tiles_n) * SC_T;
        sc_d4 acc[4][4];
        sc_tile(a.A, a.lda, a.B, a.ldb, a.K, m0, a.i_end, n0, a.N, acc, As, Bs, buf);
        // the epilogue's thread index, opaque to the compiler as in the tiles kernel
        int tq = tid;
        asm volatile("" : "+v"(tq));
        // The outputs become their p where they are, as in the tiles kernel; a kept output has p > 0 (v > theta
        // gives v - theta > 0), so the second walk knows the kept by their p.
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[i][j][r];
                    const double p = v > a.lower ? v - a.theta : 0.0;
                    acc[i][j][r] = p;
                    s += p;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        double* part = &As[buf][0][0];
        part[tq] = s;
        __syncthreads();
        double ex = 0.0;  // the chain of the tiles kernel, up to this thread
        for (int th = 0; th < tq; ++th) ex += part[th];
        int first = NONE, last = -1;  // positions 16 i + 4 j + r of this thread's walk
        double run = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double p = acc[i][j][r];
                    run += p;
                    if (p > 0.0) {
                        last = 16 * i + 4 * j + r;
                        if (first == NONE && before + (ex + run) > target) first = 16 * i + 4 * j + r;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        int f = first == NONE ? NONE : 64 * tq + first, l = last < 0 ? -1 : 64 * tq + last;  // walk positions
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int f2 = __shfl_xor(f, off, 64), l2 = __shfl_xor(l, off, 64);
            f = f2 < f ? f2 : f;
            l = l2 > l ? l2 : l;
        }
        if ((tq & 63) == 0) {
            first_s[tq >> 6] = f;
            last_s[tq >> 6] = l;
        }
        __syncthreads();
        f = first_s[0];
        l = last_s[0];
#pragma unroll
        for (int wv = 1; wv < SC_THREADS / 64; ++wv) {
            f = first_s[wv] < f ? first_s[wv] : f;
            l = last_s[wv] > l ? last_s[wv] : l;
        }
        const int at = f != NONE ? f : l;
        if (at < 0) {  // a tile without a kept output: only where the prefix is not that of these operands
            if (tq == 0) {
                a.flat[d] = -1;
                a.pval[d] = 0.0;
            }
        } else if (tq == (at >> 6)) {
            // the owner's 64 p through LDS (Bs: past the barriers above nobody reads it), so that the one at a
            // run-time position is a load, not an indexed register
            double* mine = &Bs[buf][0][0];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mine[16 * i + 4 * j + r] = acc[i][j][r];
            const int i = (at >> 4) & 3, j = (at >> 2) & 3, r = at & 3;
            const int64_t row = m0 + ((tq >> 6) & 1) * 64 + i * 16 + ((tq >> 4) & 3) + 4 * r;  // sc_row(m0, i, r)
            const int64_t col = n0 + (tq >> 7) * 64 + j * 16 + (tq & 15);                      // sc_col(n0, j)
            a.flat[d] = (row << a.mb) | col;
            a.pval[d] = mine[at & 63];
        }
        buf ^= 1;
    }
}

int sc_fail(qk_ctx* ctx, const char* msg) {
    if (ctx) ctx->err = msg;
    return QK_EARG;
}

int sc_hip(qk_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return QK_OK;
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return QK_EHIP;
}

// the checks the two entries share; null on success
const char* sc_check(int64_t K, int ma, int mb, const double* A, int64_t lda, const double* B, int64_t ldb,
                     int64_t i_begin, int64_t i_end, double tau) {
    if (ma < 0 || ma > 30 || mb < 0 || mb > 30) return "ma and mb must be in 0..30";
    if (K < 1 || K > 0x7fffffff) return "K must be at least 1";
    if (i_begin < 0 || i_begin >= i_end || i_end > ((int64_t)1 << ma)) return "need 0 <= i_begin < i_end <= 2^ma";
    if (!A || !B) return "null operand";
    if (lda < ((int64_t)1 << ma) || ldb < ((int64_t)1 << mb)) return "lda < 2^ma or ldb < 2^mb";
    if (lda > (INT64_MAX >> 4) / K || ldb > (INT64_MAX >> 4) / K) return "K * lda or K * ldb overflows";
    if (!(tau == tau)) return "tau is not a number";
    return nullptr;
}

template <bool PAIR>
void sc_launch(const ScanArgs& a, bool ent, bool hist, dim3 grid, hipStream_t st) {
    if (ent && hist) hipLaunchKernelGGL((knit_scan_kernel<PAIR, true, true>), grid, dim3(SC_THREADS), 0, st, a);
    else if (ent) hipLaunchKernelGGL((knit_scan_kernel<PAIR, true, false>), grid, dim3(SC_THREADS), 0, st, a);
    else if (hist) hipLaunchKernelGGL((knit_scan_kernel<PAIR, false, true>), grid, dim3(SC_THREADS), 0, st, a);
    else hipLaunchKernelGGL((knit_scan_kernel<PAIR, false, false>), grid, dim3(SC_THREADS), 0, st, a);
}

}  // namespace

extern "C" {

int qk_knit_scan_workspace_bytes(int ma, int mb, int64_t i_begin, int64_t i_end, int64_t* bytes) {
    if (!bytes || ma < 0 || ma > 30 || mb < 0 || mb > 30 || i_begin < 0 || i_begin >= i_end ||
        i_end > ((int64_t)1 << ma))
        return QK_EARG;
    *bytes = sc_work_bytes(sc_make_shape(mb, i_begin, i_end));
    return QK_OK;
}

int qk_knit_scan(qk_ctx* ctx, int64_t K, int ma, int mb, const double* A, int64_t lda, const double* B, int64_t ldb,
                 int64_t K2, const double* A2, int64_t lda2, const double* B2, int64_t ldb2, int64_t i_begin,
                 int64_t i_end, int flags, double tau, double* stats, int64_t* counts, int64_t* hist, void* work,
                 int64_t work_bytes) {
    if (!ctx) return QK_EARG;
    std::string msg;
    if (const char* bad = sc_check(K, ma, mb, A, lda, B, ldb, i_begin, i_end, tau)) {
        msg = std::string("qk_knit_scan: ") + bad;
        return sc_fail(ctx, msg.c_str());
    }
    if (K2 < 0) return sc_fail(ctx, "qk_knit_scan: K2 must not be negative");
    if (K2 > 0) {
        if (const char* bad = sc_check(K2, ma, mb, A2, lda2, B2, ldb2, i_begin, i_end, tau)) {
            msg = std::string("qk_knit_scan (second knit): ") + bad;
            return sc_fail(ctx, msg.c_str());
        }
    }
    if (flags & ~QK_SCAN_ENTROPY) return sc_fail(ctx, "qk_knit_scan: unknown flag");
    if (!stats || !counts) return sc_fail(ctx, "qk_knit_scan: null stats or counts");
    const sc_shape sh = sc_make_shape(mb, i_begin, i_end);
    if (!work || work_bytes < sc_work_bytes(sh))
        return sc_fail(ctx, "qk_knit_scan: workspace too small (qk_knit_scan_workspace_bytes)");
    int rc = sc_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    rc = sc_hip(ctx, hipMemsetAsync(counts, 0, QK_SCAN_NCOUNTS * sizeof(int64_t), ctx->stream), "hipMemsetAsync");
    if (rc) return rc;
    if (hist) {
        rc = sc_hip(ctx, hipMemsetAsync(hist, 0, QK_SCAN_BINS * sizeof(int64_t), ctx->stream), "hipMemsetAsync");
        if (rc) return rc;
    }
    ScanArgs a{};
    a.K = (int)K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    a.K2 = (int)K2; a.A2 = A2; a.lda2 = lda2; a.B2 = B2; a.ldb2 = ldb2;
    a.i_begin = i_begin; a.i_end = i_end; a.N = (int64_t)1 << mb; a.mb = mb;
    a.sh = sh; a.tau = tau;
    a.pstats = static_cast<double*>(work);
    a.pidx = reinterpret_cast<int64_t*>(a.pstats + SC_SLOTS * sh.groups);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    const dim3 grid((unsigned)sh.groups);
    const bool ent = flags & QK_SCAN_ENTROPY;
    if (K2 > 0) sc_launch<true>(a, ent, hist != nullptr, grid, ctx->stream);
    else sc_launch<false>(a, ent, hist != nullptr, grid, ctx->stream);
    rc = sc_hip(ctx, hipGetLastError(), "knit_scan_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(knit_scan_stage2, dim3(1), dim3(SC_THREADS), 0, ctx->stream, sh.groups, a.pstats, a.pidx,
                       K2 > 0 ? 1 : 0, ent ? 1 : 0, stats, counts);
    return sc_hip(ctx, hipGetLastError(), "knit_scan_stage2");
}

int qk_knit_collect(qk_ctx* ctx, int64_t K, int ma, int mb, const double* A, int64_t lda, const double* B,
                    int64_t ldb, int64_t i_begin, int64_t i_end, double tau, int64_t capacity, int64_t* idx,
                    double* vals, int64_t* count_dev) {
    if (!ctx) return QK_EARG;
    std::string msg;
    if (const char* bad = sc_check(K, ma, mb, A, lda, B, ldb, i_begin, i_end, tau)) {
        msg = std::string("qk_knit_collect: ") + bad;
        return sc_fail(ctx, msg.c_str());
    }
    if (capacity < 0 || !count_dev || (capacity > 0 && (!idx || !vals)))
        return sc_fail(ctx, "qk_knit_collect: negative capacity or null buffer");
    int rc = sc_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    rc = sc_hip(ctx, hipMemsetAsync(count_dev, 0, sizeof(int64_t), ctx->stream), "hipMemsetAsync");
    if (rc) return rc;
    ScanArgs a{};
    a.K = (int)K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    a.i_begin = i_begin; a.i_end = i_end; a.N = (int64_t)1 << mb; a.mb = mb;
    a.sh = sc_make_shape(mb, i_begin, i_end);
    a.tau = tau; a.capacity = capacity; a.idx = idx; a.vals = vals;
    a.count = reinterpret_cast<unsigned long long*>(count_dev);
    hipLaunchKernelGGL(knit_collect_kernel, dim3((unsigned)a.sh.groups), dim3(SC_THREADS), 0, ctx->stream, a);
    return sc_hip(ctx, hipGetLastError(), "knit_collect_kernel");
}

int qk_knit_project_scan_workspace_bytes(int ma, int mb, int64_t i_begin, int64_t i_end, int64_t* bytes) {
    if (!bytes || ma < 0 || ma > 30 || mb < 0 || mb > 30 || i_begin < 0 || i_begin >= i_end ||
        i_end > ((int64_t)1 << ma))
        return QK_EARG;
    *bytes = pj_work_bytes(sc_make_shape(mb, i_begin, i_end));
    return QK_OK;
}

int qk_knit_project_scan(qk_ctx* ctx, int64_t K, int ma, int mb, const double* A, int64_t lda, const double* B,
                         int64_t ldb, int64_t K2, const double* A2, int64_t lda2, const double* B2, int64_t ldb2,
                         int64_t i_begin, int64_t i_end, int flags, double theta, double theta2, double accuracy,
                         double* stats, int64_t* counts, void* work, int64_t work_bytes) {
    if (!ctx) return QK_EARG;
    std::string msg;
    if (const char* bad = sc_check(K, ma, mb, A, lda, B, ldb, i_begin, i_end, 0.0)) {
        msg = std::string("qk_knit_project_scan: ") + bad;
        return sc_fail(ctx, msg.c_str());
    }
    if (K2 < 0) return sc_fail(ctx, "qk_knit_project_scan: K2 must not be negative");
    if (K2 > 0) {
        if (const char* bad = sc_check(K2, ma, mb, A2, lda2, B2, ldb2, i_begin, i_end, 0.0)) {
            msg = std::string("qk_knit_project_scan (second knit): ") + bad;
            return sc_fail(ctx, msg.c_str());
        }
    }
    if (flags & ~QK_PROJ_ENTROPY) return sc_fail(ctx, "qk_knit_project_scan: unknown flag");
    if (!(theta >= 0.0) || !(theta2 >= 0.0) || !(accuracy >= 0.0))  // a NaN fails every comparison
        return sc_fail(ctx, "qk_knit_project_scan: theta, theta2 and accuracy must be numbers >= 0");
    if (!stats || !counts) return sc_fail(ctx, "qk_knit_project_scan: null stats or counts");
    const sc_shape sh = sc_make_shape(mb, i_begin, i_end);
    if (!work || work_bytes < pj_work_bytes(sh))
        return sc_fail(ctx, "qk_knit_project_scan: workspace too small (qk_knit_project_scan_workspace_bytes)");
    int rc = sc_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    rc = sc_hip(ctx, hipMemsetAsync(counts, 0, QK_PROJ_NCOUNTS * sizeof(int64_t), ctx->stream), "hipMemsetAsync");
    if (rc) return rc;
    ProjArgs a{};
    a.K = (int)K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    a.K2 = (int)K2; a.A2 = A2; a.lda2 = lda2; a.B2 = B2; a.ldb2 = ldb2;
    a.i_begin = i_begin; a.i_end = i_end; a.N = (int64_t)1 << mb; a.mb = mb;
    a.sh = sh;
    a.accuracy = accuracy; a.theta = theta; a.lower = theta > accuracy ? theta : accuracy;
    a.theta2 = theta2; a.lower2 = theta2 > accuracy ? theta2 : accuracy;
    a.pstats = static_cast<double*>(work);
    a.pidx = reinterpret_cast<int64_t*>(a.pstats + PJ_SLOTS * sh.groups);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    const dim3 grid((unsigned)sh.groups), block(SC_THREADS);
    const bool ent = flags & QK_PROJ_ENTROPY, pair = K2 > 0;
    if (ent) {
        a.ent_slot = QK_PROJ_PENT;
        hipLaunchKernelGGL(knit_project_entropy_kernel, grid, block, 0, ctx->stream, a);
        if (pair) {
            ProjArgs b = a;
            b.K = a.K2; b.A = A2; b.lda = lda2; b.B = B2; b.ldb = ldb2;
            b.theta = a.theta2; b.lower = a.lower2; b.ent_slot = QK_PROJ_PENT2;
            hipLaunchKernelGGL(knit_project_entropy_kernel, grid, block, 0, ctx->stream, b);
        }
        rc = sc_hip(ctx, hipGetLastError(), "knit_project_entropy_kernel");
        if (rc) return rc;
    }
    if (pair) hipLaunchKernelGGL(knit_project_kernel<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(knit_project_kernel<false>, grid, block, 0, ctx->stream, a);
    rc = sc_hip(ctx, hipGetLastError(), "knit_project_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(knit_project_stage2, dim3(1), block, 0, ctx->stream, sh.groups, a.pstats, a.pidx,
                       pair ? PJ_PAIR : PJ_SINGLE, ent ? 1 : 0, stats, counts);
    return sc_hip(ctx, hipGetLastError(), "knit_project_stage2");
}

int qk_knit_project_tiles(qk_ctx* ctx, int64_t K, int ma, int mb, const double* A, int64_t lda, const double* B,
                          int64_t ldb, int64_t i_begin, int64_t i_end, double theta, double accuracy, int n_masks,
                          const uint32_t* za, const uint32_t* zb, double* W) {
    if (!ctx) return QK_EARG;
    std::string msg;
    if (const char* bad = sc_check(K, ma, mb, A, lda, B, ldb, i_begin, i_end, 0.0)) {
        msg = std::string("qk_knit_project_tiles: ") + bad;
        return sc_fail(ctx, msg.c_str());
    }
    if (!(theta >= 0.0) || !(accuracy >= 0.0))  // a NaN fails every comparison
        return sc_fail(ctx, "qk_knit_project_tiles: theta and accuracy must be numbers >= 0");
    if (n_masks < 1 || n_masks > PT_MASKS)
        return sc_fail(ctx, "qk_knit_project_tiles: n_masks must be in 1..QK_PROJ_TILE_MASKS");
    if (!za || !zb || !W) return sc_fail(ctx, "qk_knit_project_tiles: null masks or W");
    for (int m = 0; m < n_masks; ++m)
        if (((uint64_t)za[m] >> ma) || ((uint64_t)zb[m] >> mb))
            return sc_fail(ctx, "qk_knit_project_tiles: a mask has a bit at or above ma (za) or mb (zb)");
    int rc = sc_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    TileArgs a{};
    a.K = (int)K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    a.i_begin = i_begin; a.i_end = i_end; a.N = (int64_t)1 << mb; a.mb = mb;
    a.sh = sc_make_shape(mb, i_begin, i_end);
    a.theta = theta; a.lower = theta > accuracy ? theta : accuracy;
    a.n_masks = n_masks;
    for (int m = 0; m < n_masks; ++m) {
        a.za[m] = za[m];
        a.zb[m] = zb[m];
    }
    a.W = W;
    const dim3 grid((unsigned)a.sh.groups), block(SC_THREADS);
    if (n_masks == 1) hipLaunchKernelGGL(knit_project_tiles_kernel<1>, grid, block, 0, ctx->stream, a);
    else if (n_masks == 2) hipLaunchKernelGGL(knit_project_tiles_kernel<2>, grid, block, 0, ctx->stream, a);
    else if (n_masks <= 4) hipLaunchKernelGGL(knit_project_tiles_kernel<4>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(knit_project_tiles_kernel<PT_MASKS>, grid, block, 0, ctx->stream, a);
    return sc_hip(ctx, hipGetLastError(), "knit_project_tiles_kernel");
}

int qk_knit_project_draw_workspace_bytes(int ma, int mb, int64_t i_begin, int64_t i_end, int64_t* bytes) {
    if (!bytes || ma < 0 || ma > 30 || mb < 0 || mb > 30 || i_begin < 0 || i_begin >= i_end ||
        i_end > ((int64_t)1 << ma))
        return QK_EARG;
    *bytes = sc_make_shape(mb, i_begin, i_end).tiles * (int64_t)sizeof(double);
    return QK_OK;
}

int qk_knit_project_draw(qk_ctx* ctx, int64_t K, int ma, int mb, const double* A, int64_t lda, const double* B,
                         int64_t ldb, int64_t i_begin, int64_t i_end, double theta, double accuracy, const double* W,
                         int64_t n_draws, const double* u, int64_t* flat, double* pval, double* total, void* work,
                         int64_t work_bytes) {
    if (!ctx) return QK_EARG;
    std::string msg;
    if (const char* bad = sc_check(K, ma, mb, A, lda, B, ldb, i_begin, i_end, 0.0)) {
        msg = std::string("qk_knit_project_draw: ") + bad;
        return sc_fail(ctx, msg.c_str());
    }
    if (!(theta >= 0.0) || !(accuracy >= 0.0))  // a NaN fails every comparison
        return sc_fail(ctx, "qk_knit_project_draw: theta and accuracy must be numbers >= 0");
    if (n_draws < 0) return sc_fail(ctx, "qk_knit_project_draw: n_draws must not be negative");
    if (!W || !total || (n_draws && (!u || !flat || !pval)))
        return sc_fail(ctx, "qk_knit_project_draw: null W, total or draw buffer");
    const sc_shape sh = sc_make_shape(mb, i_begin, i_end);
    if (!work || work_bytes < sh.tiles * (int64_t)sizeof(double))
        return sc_fail(ctx, "qk_knit_project_draw: workspace too small (qk_knit_project_draw_workspace_bytes)");
    int rc = sc_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    double* pre = static_cast<double*>(work);
    const dim3 block(SC_THREADS);
    hipLaunchKernelGGL(knit_project_prefix_kernel, dim3(1), block, 0, ctx->stream, sh.tiles, W, pre, total);
    rc = sc_hip(ctx, hipGetLastError(), "knit_project_prefix_kernel");
    if (rc || n_draws == 0) return rc;
    TileArgs a{};
    a.K = (int)K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    a.i_begin = i_begin; a.i_end = i_end; a.N = (int64_t)1 << mb; a.mb = mb;
    a.sh = sh;
    a.theta = theta; a.lower = theta > accuracy ? theta : accuracy;
    a.pre = pre; a.total = total; a.n_draws = n_draws; a.u = u; a.flat = flat; a.pval = pval;
    const int64_t groups = n_draws < PD_MAX_GROUPS ? n_draws : PD_MAX_GROUPS;
    hipLaunchKernelGGL(knit_project_draw_kernel, dim3((unsigned)groups), block, 0, ctx->stream, a);
    return sc_hip(ctx, hipGetLastError(), "knit_project_draw_kernel");
}

}  // extern "C"
