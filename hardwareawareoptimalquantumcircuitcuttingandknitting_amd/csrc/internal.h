// internal.h — context shared by the translation units of libqknit.so (not part of the ABI).
#ifndef QKNIT_INTERNAL_H
#define QKNIT_INTERNAL_H

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/qknit.h"

struct qk_ctx {
    int device;
    hipStream_t own;     // created with the context
    hipStream_t stream;  // where launches go (own, or an external stream)
    int cus;             // compute units the stream may use (its CU mask): persistent grids are sized to it
    std::string err;     // last error message (qk_last_error)
};

// qknit_select.hip: nearest_probability_distribution (quasi_distr.py:28-43) of count (key, value) pairs
// with keys below 2^key_bits — sort by key, stably by value, prefix sums, the closed-form projection
size_t npd_pairs_bytes(int64_t count);
int npd_pairs_bits(qk_ctx* ctx, int64_t count, const int64_t* keys, const double* vals, int key_bits, void* ws,
                   int64_t ws_bytes, int64_t* out_keys, double* out_vals, int64_t* n_out_dev);

// qknit.hip: the interpreter sweep of n_units = n_bind * jobs_per_binding units with the binding table
// (qk_sweep_bound without a module; arguments already checked by qk_sweep_bound_check)
int sweep_interpreter_bound(qk_ctx* ctx, const qk_program* p, int64_t n_units, int64_t jobs_per_binding,
                            int32_t n_params, const double* bind_mats, const double* job_slots,
                            const double* job_sign, void* workspace, int64_t workspace_bytes, double* pjob);

// whether any pass of the program holds QK_PARAM ops (QK_PASS_PARAM): the unbound entries refuse it
inline bool program_has_params(const qk_program* p) {
    for (int i = 0; p && p->passes && i < p->n_passes; ++i)
        if (p->passes[i].flags & QK_PASS_PARAM) return true;
    return false;
}

#endif  // QKNIT_INTERNAL_H
