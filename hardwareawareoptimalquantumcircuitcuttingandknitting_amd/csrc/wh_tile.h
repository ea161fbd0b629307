// wh_tile.h — what the row-wise transforms over outcome bits share (qknit_wht.hip, qknit_kron.hip): the tile
// of 2^13 doubles a workgroup of 512 threads owns, the pass schedule of a 2^m transform, and the trades
// between register slots and lane bits. The layout of a tile is described in qknit_wht.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int WH_TILE_BITS = 13;
constexpr int WH_THREADS = 512;
constexpr int WH_E = 16;
constexpr int WH_LATER_BITS = 9;  // c = 13 - 9 = 4: 16 doubles = 128 bytes per run
constexpr int WH_MAX_PASSES = 3;

struct wh_pass {
    uint32_t active;  // the bits of e this pass transforms
    uint32_t cmask;   // e & cmask: the consecutive part of the column
    int cshift, lo;   // (e >> cshift) << lo: the strided part (pass 0: cshift = 13, nothing)
    int rshift;       // e >> rshift: the row inside the tile (m < 13), else 13
    int tbits;        // log2 of the tiles per row
    int rowshift;     // log2 of the rows per tile
    int ubits, ushift, hshift;  // tile index = (h << ubits) | u -> column base (h << hshift) | (u << ushift)
};

// the passes of a 2^m transform; returns their number
inline int wh_schedule(int m, wh_pass* out) {
    const int t0 = m < WH_TILE_BITS ? m : WH_TILE_BITS;
    const int tbits = m - t0;
    wh_pass p;
    p.active = (1u << t0) - 1u;
    p.cmask = (1u << t0) - 1u;
    p.cshift = WH_TILE_BITS;
    p.lo = 0;
    p.rshift = t0;
    p.tbits = tbits;
    p.rowshift = WH_TILE_BITS - t0;
    p.ubits = 0;
    p.ushift = 0;
    p.hshift = WH_TILE_BITS;
    out[0] = p;
    const int rem = m - t0, later = (rem + WH_LATER_BITS - 1) / WH_LATER_BITS;
    int lo = t0;
    for (int i = 0; i < later; ++i) {
        const int nb = rem / later + (i < rem % later ? 1 : 0), c = WH_TILE_BITS - nb;
        p.active = ((1u << nb) - 1u) << c;
        p.cmask = (1u << c) - 1u;
        p.cshift = c;
        p.lo = lo;
        p.rshift = WH_TILE_BITS;
        p.tbits = tbits;
        p.rowshift = 0;
        p.ubits = lo - c;
        p.ushift = c;
        p.hshift = lo + nb;
        out[1 + i] = p;
        lo += nb;
    }
    return 1 + later;
}

// lanes 16-31 (48-63) of a trade places with lanes 0-15 (32-47) of b for T = 4; halves of the wave for T = 5
template <int T>
__device__ __forceinline__ void wh_lane_swap(double& a, double& b) {
    const unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    const unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    if constexpr (T == 5) {
        const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
        a = __hiloint2double((int)hi[0], (int)lo[0]);
        b = __hiloint2double((int)hi[1], (int)lo[1]);
    } else {
        const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
        a = __hiloint2double((int)hi[0], (int)lo[0]);
        b = __hiloint2double((int)hi[1], (int)lo[1]);
    }
}

// register bit I <-> lane bit T
template <int I, int T>
__device__ __forceinline__ void wh_xchg(double (&v)[WH_E]) {
#pragma unroll
    for (int r = 0; r < WH_E; ++r) {
        if (r & (1 << I)) continue;
        wh_lane_swap<T>(v[r], v[r | (1 << I)]);
    }
}

}  // namespace
