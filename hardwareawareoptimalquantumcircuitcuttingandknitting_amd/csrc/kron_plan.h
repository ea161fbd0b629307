// kron_plan.h — the host side of qk_kron2_rows (qknit_kron.hip): its argument checks and its passes, and the
// index mathematics the kernel shares with them. No HIP call and no dereference of src / dst in here, so a
// stand-alone host program can walk every pass under a sanitizer (tools/kron_plan_check.hip).
#pragma once

#include <cmath>
#include <cstdint>

#include "wh_tile.h"

namespace {

// one pass: the tile geometry of the Walsh-Hadamard pass plus a 2x2 matrix per bit of the element index e.
// c[i] = {A[0][0], A[0][1], A[1][0], A[1][1]} of the outcome bit that bit i of e stands for in this pass;
// p.active holds the bits whose matrix is not the identity.
struct kr_pass {
    wh_pass p;
    double c[WH_TILE_BITS][4];
};

struct kr_plan {
    int n_pass;
    kr_pass pass[1 + WH_MAX_PASSES];
    bool launch[1 + WH_MAX_PASSES];  // a pass with no active bit is skipped, unless it has to copy src to dst
    int64_t grid;                    // workgroups per pass
};

struct kr_origin {
    int64_t row0, colbase;
};

// workgroup g of a pass -> the first row and the column base of its tile
__host__ __device__ inline kr_origin kr_tile_origin(const wh_pass& p, int64_t g) {
    const int64_t t = g & (((int64_t)1 << p.tbits) - 1);
    const int64_t u = t & (((int64_t)1 << p.ubits) - 1), h = t >> p.ubits;
    return {(g >> p.tbits) << p.rowshift, (h << p.hshift) | (u << p.ushift)};
}

// element e < 2^13 of that tile -> its row (may be >= rows in the last tile of m < 13) and column
__host__ __device__ inline void kr_element(const wh_pass& p, const kr_origin& o, uint32_t e, int64_t& row,
                                           int64_t& col) {
    row = o.row0 + (e >> p.rshift);
    col = o.colbase + (e & p.cmask) + ((int64_t)(e >> p.cshift) << p.lo);
}

// Checks the arguments of qk_kron2_rows (all but ctx) and lays out the passes. Returns nullptr and fills
// `out`, or the message for qk_last_error. rows == 0 gives n_pass = 0.
inline const char* kr_make_plan(int64_t rows, int m, const double* coef, const void* src, int64_t ld_src,
                                const void* dst, int64_t ld_dst, kr_plan* out) {
    out->n_pass = 0;
    out->grid = 0;
    if (m < 0 || m > 30) return "qk_kron2_rows: m must be in 0..30";
    if (rows < 0) return "qk_kron2_rows: rows >= 0";
    const int64_t n = (int64_t)1 << m;
    if (ld_src < n) return "qk_kron2_rows: ld_src < 2^m";
    if (ld_dst < n) return "qk_kron2_rows: ld_dst < 2^m";
    if (!src || !dst) return "qk_kron2_rows: null buffer";
    if (m > 0 && !coef) return "qk_kron2_rows: null coef";
    for (int i = 0; i < 4 * m; ++i)
        if (!std::isfinite(coef[i])) return "qk_kron2_rows: coef must be finite";
    if (rows == 0) return nullptr;
    if (rows > (INT64_MAX >> 4) / ld_src || rows > (INT64_MAX >> 4) / ld_dst)
        return "qk_kron2_rows: rows * ld overflows";
    const bool in_place = src == dst && ld_src == ld_dst;
    if (!in_place) {
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((rows - 1) * ld_src + n) * sizeof(double);
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((rows - 1) * ld_dst + n) * sizeof(double);
        if (s0 < d1 && d0 < s1)
            return "qk_kron2_rows: src and dst overlap (only src == dst with equal ld is in place)";
    }
    wh_pass passes[1 + WH_MAX_PASSES];
    const int n_pass = wh_schedule(m, passes);
    const int64_t per_tile = (int64_t)1 << passes[0].rowshift;
    const int64_t grid = ((rows + per_tile - 1) / per_tile) << passes[0].tbits;
    if (grid > 0x7fffffffLL) return "qk_kron2_rows: rows * 2^(m - 13) exceeds the grid limit";
    for (int i = 0; i < n_pass; ++i) {
        kr_pass& kp = out->pass[i];
        kp.p = passes[i];
        uint32_t active = 0;
        for (int b = 0; b < WH_TILE_BITS; ++b) {
            double* c = kp.c[b];
            c[0] = c[3] = 1.0;
            c[1] = c[2] = 0.0;
            if (!(passes[i].active >> b & 1u)) continue;
            // pass 0: bit b of e is outcome bit b; later: the bits from cshift up are outcome bits lo, lo + 1, ...
            const int bit = i == 0 ? b : passes[i].lo + (b - passes[i].cshift);
            for (int k = 0; k < 4; ++k) c[k] = coef[4 * bit + k];
            if (!(c[0] == 1.0 && c[1] == 0.0 && c[2] == 0.0 && c[3] == 1.0)) active |= 1u << b;
        }
        kp.p.active = active;
        out->launch[i] = active != 0 || (i == 0 && !in_place);
    }
    out->n_pass = n_pass;
    out->grid = grid;
    return nullptr;
}

}  // namespace
