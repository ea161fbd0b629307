"""CPU model of the pipeline backend — TEST INFRASTRUCTURE ONLY.

Implements the :class:`~...pipeline.Backend` contract on torch CPU tensors:
the sweep through tests/emulator.py (numpy model of the kernel semantics), the
keyed GEMM / Khatri-Rao / gathers in numpy. Lets tests run the multi-rank
orchestration of :class:`KnitPipeline` under ``gloo`` without a GPU.
"""
import numpy as np
import torch

from emulator import emulate

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import engine, sweep_plan
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.pipeline import Backend


class _Ev:
    def record(self):
        pass

    def elapsed_time(self, other):
        return 0.0


class CpuBackend(Backend):
    routes = frozenset({"rank_factors", "prep_operands", "sweep_rows", "knit_outer_stream", "gemm_outer_paired"})
    dev = torch.device("cpu")

    def prepare_fragments(self, virt, basis: bool = False, relevance: bool = True):
        return engine.prepare_fragments(virt, upload=False, basis=basis, relevance=relevance)

    def upload_jobs(self, jobs):
        return jobs.slot_mats, torch.from_numpy(jobs.sign.copy()), torch.from_numpy(jobs.label_offsets.copy())

    def workspace_bytes(self, fs, n_jobs):
        return 0

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)

    def to_device(self, arr):
        return torch.from_numpy(np.ascontiguousarray(arr))

    def sweep(self, fs, slot, sign, n_jobs, pjob, ws):
        enc = sweep_plan.encode(fs.prog)
        pjob[:n_jobs] = torch.from_numpy(emulate(enc, slot[:n_jobs], sign.numpy()[:n_jobs]))

    def sweep_rows(self, fs):
        """Every swept row [rows, 2^m] of fs (the plan's row-pruning bound): emulated jobs, label sums."""
        enc = sweep_plan.encode(fs.prog)
        pj = torch.from_numpy(emulate(enc, fs.jobs.slot_mats, fs.jobs.sign))
        off = fs.jobs.label_offsets
        return torch.stack([pj[off[l]:off[l + 1]].sum(0) for l in range(len(off) - 1)])

    def reduce_labels(self, pjob, off, n_labels, q):
        o = off.numpy()
        for l in range(n_labels):
            q[l] = pjob[o[l]:o[l + 1]].sum(0)
        return q

    def gather_rows(self, q, idx, coef):
        return coef[:, None] * q[idx]

    def gemm_keyed(self, A, B, keyA=None, strideA=0, keyB=None, strideB=1, out=None, beta=0, skip=None):
        if skip is not None and int(skip.reshape(-1)[0]) > 0:  # qk_gemm_keyed_pred
            return out
        C = (A.T @ B).numpy()
        M, N = C.shape
        ka = keyA.numpy() if keyA is not None else np.arange(M, dtype=np.int64) * strideA
        kb = keyB.numpy() if keyB is not None else np.arange(N, dtype=np.int64) * strideB
        idx = (ka[:, None] + kb[None, :]).reshape(-1)
        o = out.numpy().reshape(-1)
        if beta:
            o[idx] += C.reshape(-1)
        else:
            o[idx] = C.reshape(-1)
        return out

    def gemm_outer_paired(self, A, B, keyB, keyA=None, strideA=0, out=None):
        kb = keyB.numpy()
        assert A.shape[0] <= 8 and (kb[1::2] == kb[0::2] + 1).all() and (kb[0::2] % 2 == 0).all()
        return self.gemm_keyed(A, B, keyA=keyA, strideA=strideA, keyB=keyB, out=out)

    def knit_outer_stream(self, A, B, clbits_a, clbits_b, nbits, out, o_begin=0, o_count=None, k_dev=None):
        """qk_knit_outer_stream_range: outputs [o_begin, o_begin + o_count) into out[o - o_begin];
        k_dev: run-time K (<= 0: nothing written)."""
        from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.knit_plan import deposit_keys

        assert A.shape[0] <= 8 and engine.stream_knit_ok(clbits_a, clbits_b, nbits)
        K = A.shape[0]
        if k_dev is not None:
            kd = int(k_dev.reshape(-1)[0])
            if kd <= 0:
                return out
            K = min(K, kd)
        if o_count is None:
            o_count = (1 << nbits) - o_begin
        ka, kb = (deposit_keys(list(c)) for c in (clbits_a, clbits_b))
        keys = (ka[:, None] + kb[None, :]).reshape(-1)
        vals = (A[:K].T @ B[:K]).numpy().reshape(-1)
        sel = (keys >= o_begin) & (keys < o_begin + o_count)
        o = out.numpy().reshape(-1)
        o[keys[sel] - o_begin] = vals[sel]
        return out

    def rank_factors(self, GA, GB, rmax=8):
        """qk_rank_factors' contract on the host algorithm (data_rank.rank_factors)."""
        from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import data_rank

        K = GA.shape[0]
        TA, TB = torch.zeros((rmax, K), dtype=torch.float64), torch.zeros((rmax, K), dtype=torch.float64)
        f = data_rank.rank_factors(GA.numpy(), GB.numpy(), rmax=rmax)
        r = 0
        if f is not None:
            r = f[0].shape[0]
            TA[:r], TB[:r] = torch.from_numpy(f[0]), torch.from_numpy(f[1])
        return TA, TB, torch.tensor([r], dtype=torch.int32)

    def prep_operands(self, WtA, qA, WtB, qB, probes):
        """qk_prep_operands' contract: (XA, XB, [GA, GB], U = XB probes^T)."""
        XA, XB = WtA.T @ qA, WtB.T @ qB
        return XA, XB, torch.stack([XA @ XA.T, XB @ XB.T]), XB @ probes.T

    def probe_errors(self, XA, A2, U, B2, probes, r=None, tol=0.0, a2_cols=None, rel_tol=0.0):
        """qk_probe_errors' contract: squared probe errors and squared reference products ([32]) over
        XA's columns (+ accepted rank)."""
        A2c = A2 if a2_cols is None else A2[:, a2_cols[0]:a2_cols[0] + a2_cols[1]]
        ref = XA.T @ U
        d = ref - A2c.T @ (B2 @ probes.T)
        e2 = torch.cat([(d * d).sum(dim=0), (ref * ref).sum(dim=0)])
        if r is None:
            return e2, None, None
        k, err = self.probe_accept(e2, r, tol, rel_tol)
        return e2, k, err

    def probe_accept(self, e2, r, tol, rel_tol=0.0):
        n = e2.numel() // 2
        err = float(e2[:n].max().sqrt())
        bound = max(tol, rel_tol * float(e2[n:].max().sqrt()))
        rv = int(r.reshape(-1)[0])
        return torch.tensor([rv if rv > 0 and err <= bound else 0], dtype=torch.int32), torch.tensor([err])

    def compress(self, TA, XA, TB, XB, a_cols=None, a_width=None):
        """qk_compress_operands' contract; a_cols = (base, n): only A2's columns [base, base + n) are
        written (from XA's, or from all of XA when it is [K, n]), the others hold NaN (a read outside
        them shows in the output); A2 is a_width wide (default XA's width)."""
        if a_cols is None:
            return (TA @ XA).contiguous(), (TB @ XB).contiguous()
        base, n = a_cols
        width = XA.shape[1] if a_width is None else a_width
        A2 = torch.full((TA.shape[0], width), float("nan"), dtype=XA.dtype)
        A2[:, base:base + n] = TA @ (XA if XA.shape[1] == n else XA[:, base:base + n])
        return A2, (TB @ XB).contiguous()

    def khatri_rao(self, A, B):
        K = A.shape[0]
        return torch.stack([torch.outer(B[k], A[k]).reshape(-1) for k in range(K)])

    def event(self):
        return _Ev()
