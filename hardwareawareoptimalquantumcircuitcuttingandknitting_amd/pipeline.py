"""Knit executor: a virtual circuit compiled once, then swept + knitted repeatedly.

``run_virtual_circuit`` (``run.py:23-71`` in the reference) rebuilds and re-runs
every instance each call. :class:`KnitPipeline` splits that into a *plan*
(fragment programs, job tables, knit operands and all device buffers, built
once) and a *step* (the hot path: batched sweep of every fragment instance,
then the dense knit), so repeated runs — and the benchmark — time only device
work. All device work goes through a backend object; the product backend is
:class:`HipBackend` (``libqknit.so``). Tests substitute a CPU model to exercise
the multi-rank orchestration with ``gloo``.

Multi-GPU (one process per GPU, ``torch.distributed`` over RCCL/xGMI): the
instance labels of every fragment are sharded contiguously across ranks; one
collective then assembles the reconstruction:

* ``reduce`` mode — each rank sweeps only the fragment rows its slice of global
  labels needs, contracts a partial distribution over that slice, and a single
  ``reduce`` (sum) lands the full distribution on rank 0. Chosen when the output
  (``2^N`` fp64) is smaller than the instance tensors (hwe/bv/qft sizes).
* ``gather`` mode — each rank sweeps its shard of every fragment's swept
  instances and computes its own block of output rows (no 34 GB reduction; the
  result stays row-sharded in ``(x_A, x_B)`` order). The row-side fragment needs
  only its column block of every instance: one ``all_to_all`` (each rank sends
  1/world of its shard to each peer); the column-side fragment is
  ``all_gather``ed (134 MB for syc 32 5 with the basis-reduced sweep). The first
  exchange overlaps the second fragment's sweep.
"""
from __future__ import annotations

import ctypes
import os
import threading
from dataclasses import dataclass
from time import perf_counter

import numpy as np

from . import _lib, engine
from .fragment_program import JobTable


_PROBES: dict = {}  # (columns, device) -> the fixed Gaussian probes [N_PROBES, n] (read-only; KnitPipeline._probes)
_PROBES_LOCK = threading.Lock()


def _mm_nt(X, Y):
    """``X @ Y.T`` for short-and-wide operands ([k1, L] x [k2, L], L up to 2^16): a plain GEMM
    has a k1 x k2 output (one or two tiles) and walks L on a few workgroups; split L into
    chunks of 256 as a batched GEMM (one output tile per chunk, whole GPU) and sum the chunks."""
    L = X.shape[1]
    nb = L // 256 if L % 256 == 0 else 1
    if nb <= 1:
        return X @ Y.T
    Xb = X.view(X.shape[0], nb, 256).transpose(0, 1)
    Yb = Y.reshape(Y.shape[0], nb, 256).transpose(0, 1)
    return (Xb @ Yb.transpose(1, 2)).sum(0)


def _pext(x: int, mask: int) -> int:
    """Bits of ``x`` at the set positions of ``mask``, packed (BMI2 pext)."""
    out, bit = 0, 0
    while mask:
        low = mask & -mask
        if x & low:
            out |= 1 << bit
        bit += 1
        mask ^= low
    return out


def _shard(n: int, rank: int, world: int) -> tuple[int, int]:
    per = -(-n // world)
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


# branch jobs per swept row at most (QKNIT_ROW_JOBS; 0: one row per label). The FINAL pass gives each
# (row, tile) one workgroup that walks the row's branch jobs serially; syc 32 5's labels carry 1-16
# jobs, and at 8 ranks the rank holding the 16-job label waited for it (FINAL 127 us for an eighth of
# the labels, profiles/r04r_rank_sim_8_timeline.txt). A longer label is swept as several rows of
# consecutive jobs whose sum is its row: the transforms repeat its row (Wt[src]), so the knit
# operands X = Wt^T q are the same sums.
ROW_JOBS = int(os.environ.get("QKNIT_ROW_JOBS", "4"))
# Swept rows the knit does not depend on are not swept (QKNIT_ROW_PRUNE: relative threshold, 0: off).
# A two-fragment knit is R = q_0^T C q_1 with the core C = W_0^T W_1 (engine._compress_core); a swept
# row whose column of the compressed transform is zero to rounding — max |W[:, j]| below ROW_PRUNE x
# max |W| — multiplies nothing: on syc 32 5, 192 of the column side's 256 light-cone basis rows (their
# core columns are exactly 0 for 42 of them and at most 1e-14 of the core's largest entry for the
# others, cancellations left at rounding level; the compressed transform's columns for them are
# 1e-20..2e-15 against entries of 1e-4..1.2 for the 64 others). Their 500 of the fragment's 625 branch
# jobs are dropped, and the operand transforms lose those rows. Whether that is sound is not assumed:
# the plan sweeps every row once (the plan's inputs are fixed, the sweep exact and deterministic, so
# every step sees the same q) and bounds the change of every output of R = X_A^T X_B, X_f = W_f q_f:
# with X_f = X'_f + D_f (kept rows / pruned rows),
#   |R - R'|[a, b] <= sum_k  m_A[k] d_B[k] + d_A[k] m_B[k] + d_A[k] d_B[k],
#   m_f[k] = sum_{j kept} |W_f[k, j]| max_x |q_f[j, x]|  (>= max_x |X'_f[k, x]|),
#   d_f[k] = sum_{j pruned} |W_f[k, j]| max_x |q_f[j, x]|
# (_prune_bound; round 5 formed m_f from X'_f itself with a GEMM, a tighter bound that waited for the
# BLAS library's first use). Rows are pruned only when that bound is at most PRUNE_TOL; otherwise the threshold
# is lowered tenfold (down to 1e-16) and, failing that, nothing is pruned. syc 32 5: see DESIGN §3.
ROW_PRUNE = float(os.environ.get("QKNIT_ROW_PRUNE", "1e-12"))
PRUNE_TOL = float(os.environ.get("QKNIT_PRUNE_TOL", "1e-13"))  # largest output change pruning may cause


def _split_rows(offsets: np.ndarray, max_jobs: int):
    """(source label of every swept row, row job offsets): labels of more than ``max_jobs`` branch
    jobs become ceil(jobs / max_jobs) rows of consecutive jobs (as even as possible)."""
    src, offs = [], [0]
    for lab in range(len(offsets) - 1):
        j0, j1 = int(offsets[lab]), int(offsets[lab + 1])
        n = j1 - j0
        pieces = max(1, -(-n // max_jobs)) if max_jobs > 0 else 1
        for p in range(pieces):
            src.append(lab)
            offs.append(j0 + (n * (p + 1)) // pieces)
    return np.asarray(src, dtype=np.int64), np.asarray(offs, dtype=np.int64)


def _deal_rows(jobs_per_row: np.ndarray, world: int) -> list:
    """Swept rows per rank, balanced by branch jobs: rows in descending job count dealt
    round-robin, reversing direction every round (at most ceil(n / world) rows per rank).
    Contiguous shards would give the rank holding a measured side program twice the jobs."""
    order = sorted(range(len(jobs_per_row)), key=lambda r: (-int(jobs_per_row[r]), r))
    out = [[] for _ in range(world)]
    for k, r in enumerate(order):
        rnd, pos = divmod(k, world)
        out[pos if rnd % 2 == 0 else world - 1 - pos].append(r)
    return [sorted(x) for x in out]


# fp64 flops per amplitude the sweep kernel spends on one op of each kind (qk_op.kind order,
# csrc/qknit.hip ap_* helpers: a complex multiply-add is 1 mul + 3 fma per component)
_OP_FLOPS = (14, 6, 14, 30, 6, 0, 0, 6, 6, 6, 2, 2, 2)


def _sweep_flops_per_job(enc) -> int:
    """fp64 flops one job of an encoded program costs: every op of a pass over the amplitudes
    the pass touches (the sparse INIT pass of a multi-pass SPLIT program only the |0..0> tile),
    plus |z|^2 (4 flops) per amplitude in the FINAL pass."""
    from . import sweep_plan

    n_amp = 1 << (enc.n_eff if enc.packed else enc.n)
    total = 0
    P = len(enc.passes)
    for ip in range(P):
        ps = enc.passes[ip]
        amps = (1 << enc.tile_bits) if (not enc.packed and ip == 0 and P > 1) else n_amp
        for gi in range(int(ps["group_begin"]), int(ps["group_end"])):
            gr = enc.groups[gi]
            for oi in range(int(gr["op_begin"]), int(gr["op_end"])):
                total += _OP_FLOPS[int(enc.ops[oi]["kind"])] * amps
    return total + 4 * n_amp


def multi_block_maps(encs: list, sweeps: list) -> list:
    """Per pass round of a multi-fragment sweep, the block order (``qk_sweep_compiled_multi``
    block_maps; None = fragments' block ranges in order). A round in which some fragment runs its
    fused FINAL pass (one workgroup per (label, tile) walking the label's branch jobs serially)
    has units of unequal work: 1 to 16 jobs per label on syc 32 5. Their blocks go heaviest first
    (longest-processing-time order, ties in range order), so the long labels start at once instead
    of in the last dispatch wave; every other round keeps the plain ranges."""
    rounds = max(len(e.passes) for e in encs)
    out = []
    for r in range(rounds):
        items, mapped, perms = [], False, {}
        for f, (enc, sw) in enumerate(zip(encs, sweeps)):
            P = len(enc.passes)
            if P <= r:
                continue
            sparse_init = r == 0 and P > 1
            fin = r == P - 1
            if sparse_init:
                work, bpu = [1] * sw["n_jobs"], 1
            elif fin and sw["fused"]:
                offs = sw["label_offsets"]
                work, bpu = list(np.diff(offs)), 1 << (enc.n - enc.pass_tile_bits(r))
                mapped = True
                perms[f] = _xcd_tile_order(enc, r)
            else:
                work, bpu = [1] * sw["n_jobs"], 1 << (enc.n - enc.pass_tile_bits(r))
            items += [(-int(w), f, u, bpu) for u, w in enumerate(work)]
        if not mapped:
            out.append(None)
            continue
        items.sort(key=lambda t: (t[0], t[1], t[2]))
        ident = {}
        m = np.fromiter(((f << 56) | (u * bpu + int(perms.get(f, ident.setdefault(bpu, range(bpu)))[t]))
                         for _, f, u, bpu in items for t in range(bpu)), dtype=np.uint64)
        out.append(m)
    return out


XCD_LINE_BITS = 5  # state bits of one 256-B run of fp64 outputs


def _xcd_tile_order(enc, r: int) -> np.ndarray:
    """Order of a (label)'s tiles in a FINAL-pass block map: tiles whose indices differ only in
    outside bits below ``XCD_LINE_BITS`` write interleaved parts of the same output lines (a
    narrowed FINAL tile leaves low state bits outside, sweep_plan.narrow_final_tile). Those bits
    become the slow bits of the block order, so such tiles land 2^(other bits) blocks apart — a
    multiple of 8 when >= 3 other bits — and blocks b, b + 8, ... share an XCD (dealt round-robin,
    MI355X_MICROARCH.md), whose L2 then merges the partial lines before they go to HBM.
    Identity when no outside bit is that low or fewer than 3 others remain. ``QKNIT_XCD_LINE_BITS``
    overrides the line width (measured on syc 32 5: 4, 5, 7 bits 0.134-0.135 ms, 8 bits 0.140)."""
    tm = int(enc.passes[r]["tile_mask"])
    outside = [q for q in range(enc.n) if not (tm >> q) & 1]
    lb = int(os.environ.get("QKNIT_XCD_LINE_BITS", XCD_LINE_BITS))
    low = [i for i, q in enumerate(outside) if q < lb]
    high = [i for i, q in enumerate(outside) if q >= lb]
    bpu = 1 << len(outside)
    if not low or len(high) < 3 or os.environ.get("QKNIT_FINAL_XCD_ORDER", "1") == "0":
        return np.arange(bpu)
    perm = np.zeros(bpu, dtype=np.int64)
    for o in range(bpu):
        t = 0
        for k, i in enumerate(high):
            t |= ((o >> k) & 1) << i
        for k, i in enumerate(low):
            t |= ((o >> (len(high) + k)) & 1) << i
        perm[o] = t
    return perm


def _joined(T, a, b):
    """``cat([a.flatten(), b.flatten()])`` without the copy when ``a`` and ``b`` are adjacent views of
    one flat buffer (engine.prep_operands' G / U, engine.compress_operands' A2 / B2): the buffer."""
    base = a._base
    if (base is not None and b._base is base and base.dim() == 1 and a.is_contiguous() and b.is_contiguous()
            and a.data_ptr() == base.data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()
            and base.numel() == a.numel() + b.numel()):
        return base
    return T.cat([a.reshape(-1), b.reshape(-1)])


class Backend:
    """What :class:`KnitPipeline` asks of the object that does its device work: the ``REQUIRED`` operations;
    ``ROUTES``, operations whose presence changes the path a step takes (a backend lists those it has in
    ``routes``, and the pipeline tests that set, never the attribute); ``OPTIONAL`` ones, called only where
    a backend's own answers lead to them; and the methods below, which have a default. A subclass is checked
    where it is defined: a missing operation or a public method the contract does not know (a misspelt one)
    is a TypeError there instead of a quietly slower route later."""

    REQUIRED = ("prepare_fragments", "upload_jobs", "workspace_bytes", "empty", "zeros", "to_device", "sweep",
                "reduce_labels", "gather_rows", "gemm_keyed", "khatri_rao", "event")
    ROUTES = {
        "rank_factors": ("rank_factors", "compress", "probe_errors"),  # the device data rank (dev_rank)
        "prep_operands": ("prep_operands",),  # its fused preparation (_fused_prep)
        "sweep_rows": ("sweep_rows",),  # the plan's row pruning (_prune_rows)
        "plan_multi": ("plan_multi", "sweep_multi"),  # one launch per pass round over all fragments
        "knit_select": ("knit_select", "npd_pairs"),  # knit_dict without the 2^N vector
        "out_buffer": ("out_buffer",),  # mapped, write-rate selected output buffers (new_out)
        "knit_outer_stream": ("knit_outer_stream",),  # the streaming small-K write
        "gemm_outer_paired": ("gemm_outer_paired",),  # the keyed small-K outer product
    }
    # with fuses_labels; with folded traced qubits; slice-mode / dense knit_dict
    OPTIONAL = ("sweep_labels", "fold_traced", "probe_accept", "select_above", "npd_dense")
    routes: frozenset = frozenset()
    dev = None  # torch device; a "cuda" one means everything before the write is stream work (overlap_ok)
    fuses_tally = False  # probe_errors(..., tally=) updates the data-rank statistics itself
    shared_init = None  # per fragment of the last plan_multi: distinct shared INIT prefixes, or None

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        needs = cls.REQUIRED + tuple(op for r in cls.routes for op in cls.ROUTES[r])  # unknown route: KeyError
        known = (set(cls.REQUIRED) | set(cls.OPTIONAL) | {op for ops in cls.ROUTES.values() for op in ops}
                 | {n for n, v in vars(Backend).items() if callable(v)})  # ... and those with a default
        bad = ([f"missing {n}" for n in needs if not callable(getattr(cls, n, None))]
               + [f"{n} is not a Backend operation" for n, v in vars(cls).items()
                  if callable(v) and not n.startswith("_") and n not in known])
        if bad:
            raise TypeError(f"{cls.__name__}: " + "; ".join(bad))

    @staticmethod
    def adopt(be):
        """``be`` under the contract. An object of a class outside it (the earlier duck-typed interface) gets
        a class of its own class and Backend: the defaults fill what it lacks, its routes are those whose
        operations it defines — the one place where the presence of a method decides anything."""
        if not isinstance(be, Backend):
            kind = type(be)
            routes = frozenset(r for r, ops in Backend.ROUTES.items()
                               if all(callable(getattr(kind, op, None)) for op in ops))
            be.__class__ = type(kind.__name__, (kind, Backend), {"routes": routes})
        return be

    def device_width(self, fs) -> int:
        """Columns of the sweep's rows of fragment ``fs``."""
        return 1 << fs.prog.m

    def fuses_labels(self, fs) -> bool:
        """Whether the sweep of ``fs`` can emit per-label rows itself (then ``sweep_labels``)."""
        return False

    def bind(self):
        """Follow the caller's current stream (nothing to do on a host backend)."""

    def outer_stream_kernel(self, K, clbits_a, clbits_b, nbits, o_begin=0, o_count=None) -> str:
        """Name of the write kernel knit_outer_stream launches for these shapes."""
        return type(self).__name__

    def compress_v(self, TA, XA, TB, XB, probes, a_cols=None, a_width=None):
        """(A2, B2, vpart): ``compress`` with the probe check's V pass fused in, or None (then the two apart)."""
        return None

    def rank_tally(self, r, k, acc):
        """acc[0] += (r == 0), acc[1] += (r > 0 and k == 0), acc[2] = k, acc[3] += 1 (int64[4])."""
        T = engine.torch()
        rv, kv = int(r.reshape(-1)[0]), int(k.reshape(-1)[0])
        acc += T.tensor([int(rv == 0), int(rv > 0 and kv == 0), 0, 1], dtype=T.int64)
        acc[2] = kv


class HipBackend(Backend):
    """Device work of the pipeline on one GPU through the C ABI."""

    routes = frozenset(Backend.ROUTES)

    def __init__(self, device: int = 0):
        self.T = engine.torch()
        self.device = device
        self.dev = self.T.device("cuda", device)
        self.ctx = engine.get_context(device)

    def prepare_fragments(self, virt, basis: bool = False, jit: bool | None = None, relevance: bool = True):
        return engine.prepare_fragments(virt, self.device, basis=basis, jit=jit, relevance=relevance)

    def upload_jobs(self, jobs: JobTable):
        return engine.jobs_to_device(jobs, self.device)

    def workspace_bytes(self, fs, n_jobs: int) -> int:
        need = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.qk_sweep_workspace_bytes(ctypes.byref(fs.dprog.struct), n_jobs,
                                                             ctypes.byref(need)), "qk_sweep_workspace_bytes")
        return need.value

    def empty(self, shape, dtype):
        return self.T.empty(shape, dtype=dtype, device=self.dev)

    def zeros(self, shape, dtype):
        return self.T.zeros(shape, dtype=dtype, device=self.dev)

    def to_device(self, arr):
        return self.T.from_numpy(np.ascontiguousarray(arr)).to(self.dev)

    def sweep(self, fs, slot, sign, n_jobs, pjob, ws):
        engine.sweep_jobs(self.ctx, fs.dprog, slot, sign, n_jobs, pjob=pjob, workspace=ws)

    def sweep_rows(self, fs):
        """Every swept row of fragment ``fs`` [rows, 2^m] (the plan's one-off sweep for the row-pruning
        bound, KnitPipeline._prune_rows)."""
        return engine.sweep_fragment(self.ctx, fs)

    def fold_traced(self, q, fold):
        return engine.fold_traced(self.ctx, q, fold)

    def device_width(self, fs) -> int:
        """Columns of the device sweep's rows (widened when traced qubits are folded afterwards)."""
        return 1 << (fs.dprog.enc.m if fs.dprog is not None else fs.prog.m)

    def bind(self):  # torch's current stream may be a forked or a graph-capture stream
        self.ctx.bind_stream()

    def plan_multi(self, frags: list, sweeps: list):
        """ctypes argument arrays of one qk_sweep_compiled_multi call over these fragments."""
        n = len(frags)
        vp = lambda xs: (ctypes.c_void_p * n)(*xs)  # noqa: E731
        i64 = lambda xs: (ctypes.c_int64 * n)(*xs)  # noqa: E731
        module = engine.compiled_multi_module(self.device, [fs.dprog.enc for fs in frags])
        outs = [(sw["q"] if sw["fused"] else sw["pjob"]) for sw in sweeps]
        maps = multi_block_maps([fs.dprog.enc for fs in frags], sweeps)
        self._maps = [None if m is None else self.to_device(m.view(np.int64)) for m in maps]  # kept alive
        rounds = len(maps)
        args = [module, (_lib.QkProgram * n)(*[fs.dprog.struct for fs in frags]), i64([sw["n_jobs"] for sw in sweeps]),
                vp([sw["slot"].data_ptr() for sw in sweeps]), vp([sw["sign"].data_ptr() for sw in sweeps]),
                i64([sw["n_local"] for sw in sweeps]),
                vp([sw["off"].data_ptr() if sw["fused"] else None for sw in sweeps]),
                vp([sw["ws"].data_ptr() for sw in sweeps]), i64([sw["ws"].numel() for sw in sweeps]),
                vp([o.data_ptr() for o in outs]),
                (ctypes.c_void_p * rounds)(*[None if m is None else m.data_ptr() for m in self._maps])]
        # shared INIT prefixes (engine.init_prefixes): one INIT tile per distinct prefix
        shared = [engine.init_prefixes(fs.dprog.enc, sw["jobs"]) if sw.get("jobs") is not None else None
                  for fs, sw in zip(frags, sweeps)]
        self.shared_init = [None if s is None else int(s[0].size) for s in shared]
        if any(s is not None for s in shared):
            self._shared = [None if s is None else (sw["slot"][self.to_device(s[0])].contiguous(),
                                                    self.to_device(s[1]))
                            for s, sw in zip(shared, sweeps)]  # kept alive
            args += [i64([0 if s is None else int(s[0].size) for s in shared]),
                     vp([None if s is None else s[0].data_ptr() for s in self._shared]),
                     vp([None if s is None else s[1].data_ptr() for s in self._shared])]
        return tuple(args)

    def sweep_multi(self, plan):
        module, progs, *rest = plan
        if len(rest) == 12:
            self.ctx.check(self.ctx.lib.qk_sweep_compiled_multi_shared(self.ctx.handle, module, len(progs), progs,
                                                                       *rest), "qk_sweep_compiled_multi_shared")
            return
        self.ctx.check(self.ctx.lib.qk_sweep_compiled_multi(self.ctx.handle, module, len(progs), progs, *rest),
                       "qk_sweep_compiled_multi")

    def fuses_labels(self, fs) -> bool:  # a compiled program's FINAL pass
        return fs.dprog is not None and fs.dprog.module is not None

    def sweep_labels(self, fs, slot, sign, n_jobs, off, n_labels, q, ws, chunks=None):
        engine.sweep_labels(self.ctx, fs.dprog, slot, sign, n_jobs, off, n_labels, q=q, workspace=ws, chunks=chunks)

    def reduce_labels(self, pjob, off, n_labels, q):
        return engine.reduce_labels(self.ctx, pjob, off, n_labels, q=q)

    def gather_rows(self, q, idx, coef):
        return engine.gather_rows(self.ctx, q, idx, coef)

    def gemm_keyed(self, A, B, **kw):
        return engine.gemm_keyed(self.ctx, A, B, **kw)

    def khatri_rao(self, A, B):
        return engine.khatri_rao(self.ctx, A, B)

    def gemm_outer_paired(self, A, B, keyB, **kw):
        return engine.gemm_outer_paired(self.ctx, A, B, keyB, **kw)

    def knit_outer_stream(self, A, B, clbits_a, clbits_b, nbits, out, o_begin=0, o_count=None, k_dev=None):
        return engine.knit_outer_stream(self.ctx, A, B, clbits_a, clbits_b, nbits, out, o_begin=o_begin,
                                        o_count=o_count, k_dev=k_dev)

    def outer_stream_kernel(self, K, clbits_a, clbits_b, nbits, o_begin=0, o_count=None):
        return engine.knit_outer_stream_kernel(K, clbits_a, clbits_b, nbits, o_begin, o_count)

    def rank_factors(self, GA, GB):
        return engine.rank_factors_device(self.ctx, GA, GB)

    def prep_operands(self, WtA, qA, WtB, qB, probes):
        return engine.prep_operands(self.ctx, WtA, qA, WtB, qB, probes)

    fuses_tally = True  # probe_errors(..., tally=) updates the data-rank statistics in its accept kernel

    def probe_errors(self, XA, A2, U, B2, probes, r=None, tol=0.0, a2_cols=None, rel_tol=0.0, tally=None, vpart=None):
        return engine.probe_errors(self.ctx, XA, A2, U, B2, probes, r=r, tol=tol, a2_cols=a2_cols, rel_tol=rel_tol,
                                   tally=tally, vpart=vpart)

    def compress_v(self, TA, XA, TB, XB, probes, a_cols=None, a_width=None):
        """qk_compress_probe_v, or None where it does not take the operands."""
        if os.environ.get("QKNIT_COMPRESS_V", "1") == "0" or not engine.compress_probe_v_ok(XA, XB, a_cols):
            return None
        return engine.compress_probe_v(self.ctx, TA, XA, TB, XB, probes, a_cols=a_cols, a_width=a_width)

    def probe_accept(self, e2, r, tol, rel_tol=0.0):
        return engine.probe_accept(self.ctx, e2, r, tol, rel_tol)

    def rank_tally(self, r, k, acc):  # on the device
        self.ctx.check(self.ctx.lib.qk_rank_tally(self.ctx.handle, r.data_ptr(), k.data_ptr(), acc.data_ptr()),
                       "qk_rank_tally")

    def compress(self, TA, XA, TB, XB, a_cols=None, a_width=None):
        return engine.compress_operands(self.ctx, TA, XA, TB, XB, a_cols=a_cols, a_width=a_width)

    def knit_select(self, A, B, clbits_a, clbits_b, nbits, accuracy, k_dev=None):
        return engine.knit_select(self.ctx, A, B, clbits_a, clbits_b, nbits, accuracy, k_dev=k_dev)

    def npd_pairs(self, keys, vals):
        return engine.npd_pairs(self.ctx, keys, vals)

    def select_above(self, dense, accuracy, key_base=0):
        return engine.select_above(self.ctx, dense, accuracy, key_base=key_base)

    def npd_dense(self, dense, accuracy):
        return engine.nearest_probability_distribution(self.ctx, dense, accuracy)

    def out_buffer(self, n: int, select: bool = True):
        """(tensor [n] float64, owner): the knit output, 1-GiB-mapped when large (engine.out_buffer)."""
        return engine.out_buffer(self.ctx, n, select=select)

    def event(self):
        return self.T.cuda.Event(enable_timing=True)


@dataclass
class PreparedStep:
    """What the preparation of a device data-rank step (``_prep_dev_rank`` / ``_prep_slice``) hands to its
    write (``_launch_dev_rank`` / ``_launch_slice``, ``knit_dict``)."""
    A2: object  # compressed row-side operand [rmax, 2^mA]
    B2: object  # compressed column-side operand [rmax, 2^mB]
    k_eff: object  # device int32[1]: the accepted rank, 0 = rejected (the exact contraction runs)
    mats: list  # per fragment: the exact operand X = Wt^T q (None for fragments outside the pair)
    # finisher of the asynchronous exact gather -> (A, keyA, B, keyB): _prep_slice sets, _launch_slice calls it
    exact: object = None
    # QKNIT_SLICE_EXACT=host: (pinned copy of k_eff, its event or None); _prep_slice sets, _launch_slice waits
    host_verdict: tuple | None = None
    # the predicated exact slice is queued ahead of the write: _step_overlapped sets, _launch_slice reads
    exact_queued: bool = False


class KnitPipeline:
    def __init__(self, virt, device: int = 0, factored: bool = False, rank: int = 0, world: int = 1,
                 mode: str | None = None, group=None, backend=None, chunk_jobs: int | None = None,
                 jit: bool | None = None, light_cone: bool = True, data_rank: bool | None = None):
        self.be = Backend.adopt(backend) if backend is not None else HipBackend(device)
        # branch jobs per sweep chunk of a fused (compiled) fragment; 0 = the whole fragment at once
        self.chunk_jobs = int(os.environ.get("QKNIT_SWEEP_CHUNK_JOBS", "0")) if chunk_jobs is None else chunk_jobs
        self.fork = False  # single mode: sweep each fragment on its own stream (set by capture_sweep)
        self._multi = None
        self._streams = []
        self._sweep_graph = None
        self.T = engine.torch()
        self.virt = virt
        self.rank, self.world, self.group = rank, world, group
        # a virtual gate with both endpoints in one fragment: the direct knit (engine.factored_ok)
        factored = factored and engine.factored_ok(virt)
        self.factored = factored
        # light_cone (factored knit): exact light-cone projections in the basis reduction and the
        # rank-compressed two-fragment core (fragment_program.slot_relevance,
        # engine._compress_core); False keeps the plain factored knit (prod r_j terms)
        kw = {} if light_cone else {"relevance": False}
        if jit is not None:
            kw["jit"] = jit
        # host time of each planning phase (ms; device work inside a phase is included only where
        # the phase waits for it): the drop-in's first-call breakdown (bench.py drop_in)
        self.plan_ms = {}
        tick = perf_counter()
        with engine.host_planning():
            self.frags = self.be.prepare_fragments(virt, basis=factored, **kw)
            tick = self._phase("prepare_fragments", tick)
            self.ops = engine.knit_operands(virt, self.frags, factored, compress=light_cone)
            tick = self._phase("knit_operands", tick)
        self.N = virt.circuit.num_clbits
        q_bytes = sum(len(fs.labels) << fs.prog.m for fs in self.frags) * 8
        out_bytes = (1 << self.N) * 8
        self.order = engine.contract_order(self.ops.clbits)
        if mode is None:
            if world == 1:
                mode = "single"
            elif out_bytes <= q_bytes and not factored:
                mode = "reduce"
            else:
                mode = "slice" if self.slice_ok(world) else "gather"
        if mode == "reduce" and factored:
            raise ValueError("reduce mode needs the direct (label-sliced) knit")
        if mode not in ("single", "reduce", "gather", "slice"):
            raise ValueError(f"unknown mode {mode}")
        if mode == "slice" and not self.slice_ok(world):
            raise ValueError("slice mode needs a factored two-fragment knit whose fragments partition the output "
                             "bits, a power-of-two world and >= 2^9 outputs per rank")
        self.mode = mode
        # data_rank (single mode, factored, two fragments): each step compresses the two knit
        # operands to the numerical rank of R = A^T B (engine.data_rank_factors), contracts with
        # the output-write-bound small-K kernel, and verifies the result by random probes
        # (falls back to the exact contraction if a probe exceeds rank_tol)
        two = len(self.frags) == 2 and not any(fs.dropped for fs in self.frags)
        ok = mode in ("single", "gather", "slice") and factored and two
        # default: only where the write dominates (>= 2^24 outputs); below that the factorisation and
        # its probe check cost more than the whole knit (bv 5 / hwe 16: < 0.02 ms)
        self.data_rank = (ok and virt.circuit.num_clbits >= 24) if data_rank is None else (data_rank and ok)
        # rank_tol: bound on every probe's ||(R - A''^T B'') x||_2 (x: N_PROBES fixed Gaussian vectors):
        # tol = max(rank_tol, rank_tol_rel * max_j ||R x_j||), an absolute floor plus the scale of the knit
        # itself (||R x|| ~ ||R||_F; syc 32 5: 2e-5, so the floor decides there; a distribution with
        # wide entries, ||R||_F ~ 0.1, gets 1e-13 instead of being rejected on rounding every step).
        # With 16 probes, P(max_j ||D x_j|| <= tol while ||D||_F > 10 tol) <= P(chi2_1 <= 0.01)^16 < 3e-18
        # (rank-one D is the worst case), and every entry of D is at most ||D||_F: the accepted
        # compression moves no output by more than 10 tol (1e-13 at the floor; 1e-12 ||R||_F at most)
        # except with that probability.
        self.rank_tol = 1e-14
        self.rank_tol_rel = 1e-12
        self.rank_fallbacks = 0  # steps whose probe check rejected the compression
        self.rank_incompressible = 0  # device path: steps with no factorisation of rank <= 8
        self.last_rank = None
        cA, cB = self._stream_bits()
        # device data rank (single / slice): qk_rank_factors + probe check + the predicated knits,
        # no host round trip before the write (single mode: none at all)
        self.dev_rank = bool(self.data_rank and cA is not None and self.ops.num_terms <= 64
                             and "rank_factors" in self.be.routes)
        self._pending = 0  # device-rank steps whose statistics are not yet read back (sync_stats)
        self._tally = None  # device int64[4]: incompressible, rejected, last accepted rank, steps (_note_rank)
        self._tally_read = np.zeros(4, dtype=np.int64)
        self._rank_rejects = 0  # host data rank: consecutive rejected compressions (RANK_GIVE_UP)
        self._prune_mq = None  # while the plan prunes rows: per side, every swept row's largest entry
        self._x_local = None  # sharded slice mode: this rank's column block of the fixed probes
        self._exact_plan = None  # slice mode: per side, the columns and keys of this rank's exact slice
        self._exact_stream = None  # sharded slice mode: helper stream reordering the gathered exact operands
        self._started = []  # pipelined steps: events at the start of the last out_buffers steps
        self._last_owner = None  # owner of the mapping new_out made last (None: a torch / backend tensor)
        self._call_owner = None  # owner of the drop-in's output mapping, reused by later calls (take_out)
        self._time_call_write = False  # the drop-in call's own write decides if that mapping stays
        # slice mode, fused preparation: every rank factors the same all-reduced Grams with the same
        # deterministic kernel, so no broadcast of the factors; each rank checks the rows of R in its
        # A column block against every probe, and a MIN all-reduce of the accepted ranks gives one
        # decision for all ranks (the A blocks cover all of R; a rejection anywhere sends every rank
        # to the exact slice, so its collectives match). Factors that differed between ranks would mix
        # compressed columns and fail some rank's check. QKNIT_SLICE_SYNC=1: rank 0's factors broadcast.
        self.slice_sync = os.environ.get("QKNIT_SLICE_SYNC", "0") == "1"
        # slice mode, the exact fallback of a rejected compression: "predicated" (default) all-gathers
        # its operands every step and predicates the contraction on the device verdict (no host sync
        # in the step); "host" reads the verdict on the host and gathers only on a rejection
        self.slice_exact = os.environ.get("QKNIT_SLICE_EXACT", "predicated")
        self.last_kernel = None  # kernel of the last compressed contraction (None: qk_gemm_keyed)
        self.last_prep = None  # data-rank preparation of the last step: "fused" (qk_prep_operands) or "torch"
        self._probe = None
        self._pinned = None  # host staging of the two Gram matrices (pinned on a GPU)
        self._prep_stream = None
        self._write_stream = None
        self.overlap_cus = None  # (prep CUs, write CUs) of pipelined steps
        # software-pipelined steps (_step_overlapped), off by default: measured on syc 32 5 (one box,
        # same build) 5.82 ms per step without, 7.20 with (the persistent write grid holds every CU,
        # so the side stream's sweep waits for it), 6.55 with a one-workgroup-per-task write grid,
        # 6.06 with 4 write workgroups per CU. QKNIT_OVERLAP=1 turns it on.
        self.overlap = os.environ.get("QKNIT_OVERLAP", "0") == "1"
        # pipelined steps: output buffers (QKNIT_OUT_BUFFERS; 2: steps alternate between two buffers and
        # two write streams, so step i+1's write may start while step i's drains). Default 2 at 4 ranks
        # only: rank_sim (modelled xGMI, 20 steps, 4 runs each) 1.56-1.64 vs 1.70-1.80 ms per step at 4
        # ranks, 2.71 vs 2.67-2.74 at 2, 0.94-1.21 vs 0.90-1.13 at 8; 5.00-5.03 vs 4.97-5.06 pipelined
        # on one GPU (profiles/r04bq_*)
        # Round 5 (replicated slice preparation, rank_sim with modelled xGMI, same box, two rounds each,
        # profiles/r05i-k_*): 8 ranks 0.92 / 0.90 / 0.82-0.86 ms per step with 1 / 2 / 3 buffers (96
        # preparation CUs), 0.82-0.85 with 3 buffers and 128 CUs, 1.06-1.18 with 4 (more write streams than
        # hardware queues: GPU_MAX_HW_QUEUES = 4); 4 ranks 1.38 (2) / 1.37-1.40 (3); 2 ranks 2.58 (2).
        # Default: 3 buffers from 8 ranks on, 2 at 2-4 ranks, 1 on one GPU
        ob = os.environ.get("QKNIT_OUT_BUFFERS", "")
        self.out_buffers = int(ob) if ob else (3 if world >= 8 else 2 if world >= 2 else 1)
        self._outs = None
        self._wstreams = None
        self._flip = 0
        self._write_cus = None
        self.events = []  # (start, end) events around the main contraction GEMM
        self.sweep_events = []  # (start, end) events around each step's sweep (all fragments)
        self.prep_events = []  # (sweep end, knit start): operand transforms + data-rank compression
        self.record_events = False
        self.row_jobs = ROW_JOBS
        self.row_prune = ROW_PRUNE
        self.out_alloc = None  # how the last output buffer was allocated (new_out)
        # slice mode: how a rank gets the operands of its slice (_choose_slice_prep, QKNIT_SLICE_PREP):
        # "replicated" — every rank sweeps every swept row and runs the whole preparation chain itself
        # (deterministic kernels on identical inputs: identical operands on every rank), checks its own
        # slice's rows and writes its slice; no collective in the step. "sharded" — rows dealt over the ranks, one
        # all_to_all / all_reduce / all_gather / MIN all_reduce per step (round 2-4's slice mode).
        self.slice_prep = None
        self.slice_costs = None  # the cost model's per-step estimates (ms) of both, when it chose
        self._plan()

    def _phase(self, name: str, since: float) -> float:
        """Record ``perf_counter() - since`` as planning phase ``name`` (ms); returns the new mark."""
        now = perf_counter()
        self.plan_ms[name] = self.plan_ms.get(name, 0.0) + (now - since) * 1e3
        return now

    def _stream_bits(self):
        """(clbits of the row side, of the column side) when two live fragments partition the output
        bits with clbit 0 on the column side (the streaming knit applies), else (None, None)."""
        live = [i for i, fs in enumerate(self.frags) if not fs.dropped]
        if len(live) != 2 or len(self.order) != 2:
            return None, None
        cA, cB = self.ops.clbits[self.order[0]], self.ops.clbits[self.order[-1]]
        return (cA, cB) if engine.stream_knit_ok(cA, cB, self.N) else (None, None)

    def slice_ok(self, world: int) -> bool:
        """Whether ``slice`` mode applies: each rank owns the contiguous output range
        ``[rank, rank + 1) * 2^N / world`` of the reference-ordered distribution (factored
        two-fragment knit written by the streaming kernel; world a power of two; >= 2^9 outputs and
        whole column blocks of both fragments per rank)."""
        cA, cB = self._stream_bits()
        # world 1: only when asked for (mode="slice": the collectives on a one-rank group, tests)
        if cA is None or world < 1 or world & (world - 1) or not self.factored:
            return False
        return (1 << self.N) // world >= 512 and min(len(cA), len(cB)) >= world.bit_length() - 1

    # ------------------------------------------------------------------ plan
    def _plan(self):
        T, be = self.T, self.be
        self.sweeps = []  # per fragment: device job tables and buffers, or None (dropped)
        # per fragment: source label of each swept row when rows are pruned (ROW_PRUNE) or labels split
        # (ROW_JOBS), else None; and the number of swept rows
        self.row_src, self.n_rows, self.plan_jobs = [], [], []  # plan_jobs: branch jobs swept (all ranks)
        L = self.ops.num_terms
        self.term_range = _shard(L, self.rank, self.world) if self.mode == "reduce" else (0, L)
        self.place = {}  # gather mode: fragment -> position of each swept row in the gathered rows
        tick = perf_counter()
        pruned = self._prune_rows()
        tick = self._phase("row_pruning", tick)
        swept = [self._swept_rows(i, fs, pruned.get(i)) for i, fs in enumerate(self.frags)]
        if self.mode == "slice":
            self.slice_prep, self.slice_costs = self._choose_slice_prep(swept)
        self.sharded = self.mode == "gather" or (self.mode == "slice" and self.slice_prep == "sharded")
        for i, fs in enumerate(self.frags):
            if fs.dropped:
                self.sweeps.append(None)
                self.row_src.append(None)
                self.n_rows.append(fs.n_rows)
                self.plan_jobs.append(0)
                continue
            src, jobs, nl = swept[i]
            self.row_src.append(src)
            self.n_rows.append(nl)
            self.plan_jobs.append(jobs.n_jobs)
            lo = 0
            if self.sharded:
                per = -(-nl // self.world)
                dealt = _deal_rows(jobs.label_jobs(), self.world)
                place = np.zeros(nl, dtype=np.int64)
                for r, rows_r in enumerate(dealt):
                    place[rows_r] = r * per + np.arange(len(rows_r))
                self.place[i] = place
                sub = jobs.take(dealt[self.rank])
            else:
                if self.mode == "reduce":
                    t0, t1 = self.term_range
                    rows = np.unique(self.ops.rows[i][t0:t1])
                    lo, hi = (int(rows.min()), int(rows.max()) + 1) if rows.size else (0, 0)
                else:
                    lo, hi = 0, nl
                sub = jobs.take(np.arange(lo, hi))
            n_local = len(sub.label_offsets) - 1
            slot_t, sign_t, off_t = be.upload_jobs(sub)
            n_jobs = sub.n_jobs
            width = be.device_width(fs)
            need = be.workspace_bytes(fs, n_jobs) if n_jobs else 0
            # gather / sharded slice mode: a rank's rows live in a zero-padded [per, width] buffer (the
            # unit of the collectives); padding rows stay zero
            sharded = self.sharded
            rows = -(-nl // self.world) if sharded else max(n_local, 1)
            alloc = be.zeros if sharded else be.empty
            branching = n_jobs != n_local
            # branching + compiled program: the FINAL pass writes the label rows (no pjob, no reduce)
            fused = branching and n_jobs > 0 and be.fuses_labels(fs)
            chunks = None
            if fused and self.chunk_jobs and n_jobs > self.chunk_jobs:
                offs = sub.label_offsets
                chunks = [(l0, l1, j0, j1, be.to_device(offs[l0:l1 + 1] - j0))
                          for l0, l1, j0, j1 in engine.label_chunks(offs, self.chunk_jobs)]
                need = be.workspace_bytes(fs, max(c[3] - c[2] for c in chunks))
            self.sweeps.append(dict(lo=lo, n_local=n_local, slot=slot_t, sign=sign_t, off=off_t, n_jobs=n_jobs,
                                    fused=fused, chunks=chunks, label_offsets=sub.label_offsets, jobs=sub,
                                    pjob=(None if fused else
                                          be.empty((max(n_jobs, 1), width), T.float64) if branching
                                          else alloc((max(rows, 1), width), T.float64)),
                                    q=alloc((max(rows, 1), width), T.float64) if branching else None,
                                    ws=be.empty((max(need, 1),), T.uint8)))
        tick = self._phase("job_tables", tick)
        self._plan_knit()
        if self.sharded:
            self._plan_exchange()
        tick = self._phase("knit_tables", tick)
        self._plan_multi()
        self._phase("sweep_launch_plan", tick)

    def _prune_rows(self) -> dict:
        """{fragment: kept swept rows} of the row pruning (ROW_PRUNE, PRUNE_TOL): two live fragments
        with factored transforms only; the bound of every output's change (``_prune_bound``) on the
        plan's own rows, swept once here, must be at most PRUNE_TOL. ``self.prune_bound`` keeps it."""
        self.prune_bound = None
        W = self.ops.transforms
        live = [i for i, fs in enumerate(self.frags) if not fs.dropped]
        if (self.row_prune <= 0 or len(live) != 2 or any(W[i] is None or not self.frags[i].jobs.n_jobs for i in live)
                or "sweep_rows" not in self.be.routes):
            return {}
        cms = {i: np.abs(np.asarray(W[i])).max(axis=0) for i in live}  # per swept row: largest entry
        qs, thr = None, self.row_prune
        while thr >= 1e-16:
            keep = {i: np.flatnonzero(cms[i] > thr * cms[i].max()) for i in live}
            pruned = {i: k for i, k in keep.items() if k.size < cms[i].size}
            if not pruned:  # nothing below this threshold, so nothing below any smaller one
                break
            if qs is None:
                qs = {i: self.be.sweep_rows(self.frags[i]) for i in live}
            bound = self._prune_bound(qs, keep)
            if bound <= PRUNE_TOL:
                self.prune_bound = bound
                self._prune_mq = None
                return pruned
            thr /= 10
        self._prune_mq = None
        return {}

    def _prune_bound(self, qs: dict, keep: dict) -> float:
        """Bound on max |R - R'| over every output when only the ``keep`` rows of each side are swept
        (the ROW_PRUNE comment): ``qs`` every swept row of both sides [rows, 2^m], exact. Only the rows'
        largest entries are read back (one device reduction per side, no GEMM: the plan does not wait
        for a BLAS library's first-use initialisation, ~0.2 s in a fresh process); with
        ``mq[j] = max_x |q[j, x]|`` the kept part of each operand row is bounded by the triangle
        inequality, ``max_x |X'_f[k, x]| <= sum_{j kept} |W_f[k, j]| mq[j]``, and
        ``d_f[k] = sum_{j pruned} |W_f[k, j]| mq[j]`` as before."""
        if self._prune_mq is None:
            self._prune_mq = {i: qs[i].abs().amax(dim=1).cpu().numpy() for i in sorted(keep)}
        m, d = [], []
        for i in sorted(keep):
            W = np.abs(np.asarray(self.ops.transforms[i]))
            mq = self._prune_mq[i]
            kept = np.zeros(W.shape[1], dtype=bool)
            kept[keep[i]] = True
            m.append(W[:, kept] @ mq[kept])
            d.append(W[:, ~kept] @ mq[~kept])
        return float((m[0] * d[1] + d[0] * m[1] + d[0] * d[1]).sum())

    def _swept_rows(self, i: int, fs, keep):
        """(source label of every swept row or None, job table, rows) of fragment i: the ``keep`` rows
        of the row pruning, labels of more than ROW_JOBS branch jobs split into several rows."""
        if fs.dropped:
            return None, None, fs.n_rows
        nl, jobs, src = fs.n_rows, fs.jobs, None
        if keep is not None:
            src, jobs, nl = keep, jobs.take(keep), keep.size
        if self.ops.transforms[i] is not None and self.row_jobs > 0 and jobs.n_jobs:
            piece_src, offs = _split_rows(jobs.label_offsets, self.row_jobs)
            if len(piece_src) > nl:
                jobs = JobTable(jobs.slot_mats, jobs.sign, offs, jobs.branch_bits)
                nl = len(piece_src)
                src = piece_src if src is None else src[piece_src]
        return src, jobs, nl

    # slice-mode cost model (_choose_slice_prep), per step on one rank. Rates measured on syc 32 5:
    # the sweep's modelled fp64 flops (_sweep_flops_per_job) ran at ~49 TF/s (2.79 GFLOP in 0.057 ms,
    # BENCH_r04), the preparation chain 0.14 ms for 2 x 65 rows x 2^16 columns x K = 64 (2.2 GFLOP of
    # transforms + Grams at ~27 TF/s, plus ~60 us of dependent small launches whatever the size);
    # collectives as rank_sim's xGMI model: 20 us per collective + received bytes / (min(world - 1, 7)
    # links x 50 GB/s), and the packing glue around them at a third of HBM speed (read + reorder +
    # write; ~200 us at 8 ranks on syc 32 5, profiles/r04s_rank_sim_8_timeline_split.txt)
    SWEEP_MODEL_TFS = 49.0
    PREP_FIXED_MS, PREP_GFS = 0.06, 27000.0  # MFMA GFLOP/s the transforms + Grams reach in the chain
    XGMI_GBS, COLL_LAT_MS = 50.0, 0.020

    def _choose_slice_prep(self, rows: list):
        """("replicated" | "sharded", {estimates}) for slice mode. ``QKNIT_SLICE_PREP`` forces one.
        Replicated: every rank runs the whole sweep and preparation (t_sweep + t_prep), no collective.
        Sharded: 1/world of each plus four collectives (all_to_all of the rows' column blocks, the
        Gram all_reduce, the compressed-operand all_gather, the MIN all_reduce) and, with the
        predicated exact fallback, the all_gather of the exact operands. The cheaper estimate wins."""
        P = self.world
        force = os.environ.get("QKNIT_SLICE_PREP", "auto")
        from . import sweep_plan

        flops, prep_flops, a2a, gat = 0, 0.0, 0, 0
        K = self.ops.num_terms
        for i, fs in enumerate(self.frags):
            src, jobs, nl = rows[i]
            if fs.dropped or jobs is None:
                continue
            enc = fs.dprog.enc if getattr(fs, "dprog", None) is not None else sweep_plan.encode(fs.prog)
            flops += jobs.n_jobs * _sweep_flops_per_job(enc)
            w = 1 << fs.prog.m
            prep_flops += 2.0 * K * nl * w + 2.0 * K * K * w
            a2a += 8 * nl * w * (P - 1) // (P * P)  # received: its column block of every peer's rows
            gat += 8 * K * w * (P - 1) // P  # the exact operands' column blocks (one side travels)
        t_sweep = flops / (self.SWEEP_MODEL_TFS * 1e9)
        t_prep = self.PREP_FIXED_MS + prep_flops / (self.PREP_GFS * 1e6)
        links = max(1, min(P - 1, 7))
        coll = lambda nbytes: self.COLL_LAT_MS + nbytes / (links * self.XGMI_GBS * 1e6)  # noqa: E731
        glue = 3 * (a2a + gat) / (8000 * 1e6) * 3
        t_rep = t_sweep + t_prep
        t_sh = (t_sweep + t_prep) / P + coll(a2a) + 3 * self.COLL_LAT_MS + coll(gat // 2) + glue
        costs = {"replicated_ms": round(t_rep, 4), "sharded_ms": round(t_sh, 4)}
        if force in ("replicated", "sharded"):
            return force, costs
        return ("replicated" if t_rep <= t_sh else "sharded"), costs

    def _plan_multi(self):
        """Single and gather mode: when every swept fragment runs compiled kernels of one tile
        width (2-4 fragments, not chunked), the whole sweep is one qk_sweep_compiled_multi call —
        pass round r of all fragments in one launch — instead of a launch sequence per fragment.
        In gather mode the collectives then start after the one sweep (a rank's shard is small:
        one launch beats overlapping the row side's all_to_all with a second sweep)."""
        self._multi = None
        if (self.mode == "reduce" or os.environ.get("QKNIT_SWEEP_MULTI", "1") == "0"
                or "plan_multi" not in self.be.routes):
            return
        idx = [i for i, sw in enumerate(self.sweeps) if sw is not None]
        ok = all(self.sweeps[i]["n_jobs"] and self.sweeps[i]["chunks"] is None
                 and getattr(self.frags[i], "dprog", None) is not None and self.frags[i].dprog.module is not None
                 for i in idx)
        encs = [self.frags[i].dprog.enc for i in idx] if ok else []
        rounds = max((len(e.passes) for e in encs), default=0)
        if not ok or not 2 <= len(idx) <= 4 or any(
                len({e.pass_tile_bits(r) for e in encs if len(e.passes) > r}) != 1 for r in range(rounds)):
            return
        self._multi = (idx, self.be.plan_multi([self.frags[i] for i in idx], [self.sweeps[i] for i in idx]))

    def _plan_exchange(self):
        """Collectives of gather mode. With two fragments the A side (output rows) only needs
        its column block of every instance row: one all_to_all of 1/world^2 of q_A per rank
        pair instead of an all_gather; the B side (output columns) is all-gathered. Buffers are
        allocated once."""
        be, T, P = self.be, self.T, self.world
        live = [i for i, fs in enumerate(self.frags) if not fs.dropped]
        a_side = self.order[0]
        width_a = 1 << len(self.ops.clbits[a_side])
        self.split_a = (len(self.order) == 2 and len(live) == 2 and width_a % P == 0)
        self.xbuf = {}
        for i in live:
            per = -(-self.n_rows[i] // P)
            width = 1 << self.frags[i].prog.m
            if self.mode == "slice" or (self.split_a and i == a_side):
                bw = width // P
                self.xbuf[i] = ("a2a", be.empty((P, per, bw), T.float64), be.empty((P * per, bw), T.float64))
            else:
                self.xbuf[i] = ("gather", None, be.empty((P * per, width), T.float64))

    def _plan_knit(self):
        be, ops = self.be, self.ops
        self.gather_idx, self.gather_coef, self.transforms = [], [], []
        t0, t1 = self.term_range
        for i, fs in enumerate(self.frags):
            place = self.place.get(i)
            if ops.transforms[i] is not None:
                Wt = ops.transforms[i].T  # [labels, terms]
                if self.row_src[i] is not None:  # pruned / split rows: every row takes its label's row
                    Wt = Wt[self.row_src[i]]
                if place is not None:  # rows as the collectives deliver them (rank-major, padded)
                    Wg = np.zeros((self.world * -(-self.n_rows[i] // self.world), Wt.shape[1]))
                    Wg[place] = Wt
                    Wt = Wg
                self.transforms.append(be.to_device(Wt))
                self.gather_idx.append(None)
                self.gather_coef.append(None)
            else:
                self.transforms.append(None)
                sw = self.sweeps[i]
                rows = ops.rows[i][t0:t1]
                if place is not None:
                    rows = place[rows]
                elif sw is not None and self.mode == "reduce":
                    rows = rows - sw["lo"]
                self.gather_idx.append(be.to_device(rows))
                self.gather_coef.append(be.to_device(ops.coefs[i][t0:t1]))
        self.row_block = None
        self.slice = None
        if self.mode == "slice":
            n_out = (1 << self.N) // self.world
            self.slice = (self.rank * n_out, n_out)
        if self.mode == "gather":
            width_a = 1
            for i in self.order[:-1]:
                width_a <<= len(ops.clbits[i])
            self.row_block = _shard(width_a, self.rank, self.world)
        self.out = None

    # ------------------------------------------------------------------ step
    def sweep(self) -> list:
        """Instance sweep of every fragment; returns the ``q_f`` tensors this rank needs (in
        gather mode: all rows, and only this rank's column block on a split A side)."""
        T, be = self.T, self.be
        qs = [None] * len(self.frags)
        pending = []
        if self._multi is not None and not self.fork:
            idx, plan = self._multi
            be.sweep_multi(plan)
            for i in sorted(range(len(self.frags)), key=lambda i: self.order.index(i)):
                fs, sw = self.frags[i], self.sweeps[i]
                if sw is None:
                    qs[i] = be.zeros((fs.n_rows, 1), T.float64) + 1.0
                    continue
                q = self._fold(fs, sw["q"] if sw["fused"] else sw["pjob"])
                if self.sharded:
                    work, qs[i] = self._exchange(i, q)
                    pending.append(work)
                else:
                    qs[i] = q[: sw["n_local"]]
            for work in pending:
                work.wait()
            return qs
        fork = self.fork and self.mode == "single"
        main = T.cuda.current_stream() if fork else None
        # the A side (output rows) first, so its exchange overlaps the other sweeps
        for k, i in enumerate(sorted(range(len(self.frags)), key=lambda i: self.order.index(i))):
            fs, sw = self.frags[i], self.sweeps[i]
            if sw is None:
                ones = be.zeros((fs.n_rows, 1), T.float64)
                ones += 1.0
                qs[i] = ones
                continue
            if fork:  # fragments are independent: one stream each, joined below
                while len(self._streams) <= k:
                    self._streams.append(T.cuda.Stream(device=main.device))
                s = self._streams[k]
                s.wait_stream(main)
                with T.cuda.stream(s):
                    be.bind()
                    q = self._fold(fs, self._sweep_fragment(fs, sw))
            else:
                q = self._fold(fs, self._sweep_fragment(fs, sw))
            if self.sharded:
                work, qs[i] = self._exchange(i, q)
                pending.append(work)
            else:
                qs[i] = q[: sw["n_local"]]
        if fork:
            for s in self._streams:
                main.wait_stream(s)
            be.bind()
        for work in pending:
            work.wait()
        return qs

    def _fold(self, fs, q):
        """Widened sweep rows -> the fragment's measured outcomes (engine.fold_traced)."""
        return self.be.fold_traced(q, fs.fold) if getattr(fs, "fold", 1) > 1 else q

    def _sweep_fragment(self, fs, sw):
        be = self.be
        if sw["fused"]:
            be.sweep_labels(fs, sw["slot"], sw["sign"], sw["n_jobs"], sw["off"], sw["n_local"], sw["q"], sw["ws"],
                            chunks=sw["chunks"])
            return sw["q"]
        if sw["n_jobs"]:
            be.sweep(fs, sw["slot"], sw["sign"], sw["n_jobs"], sw["pjob"], sw["ws"])
        if sw["q"] is not None:
            return be.reduce_labels(sw["pjob"], sw["off"], sw["n_local"], sw["q"])
        return sw["pjob"]

    def capture_sweep(self):
        """Record one step's sweep — every pass launch of every fragment, the fragments on forked
        streams — as one HIP graph (torch.cuda.CUDAGraph); :meth:`replay_sweep` re-issues it with
        a single launch call. Single mode only (gather mode's collectives stay eager)."""
        T = self.T
        if self.mode != "single":
            raise ValueError("sweep graphs are for single-GPU pipelines")
        self.fork = True
        self.sweep()  # outside the capture: streams, lazy allocations
        T.cuda.synchronize()
        g = T.cuda.CUDAGraph()
        with T.cuda.graph(g):
            self.be.bind()
            qs = self.sweep()
        self.be.bind()
        self._sweep_graph, self._graph_qs = g, qs
        return qs

    def replay_sweep(self) -> list:
        self._sweep_graph.replay()
        return self._graph_qs

    def _exchange(self, i, qpad):
        """Start fragment i's collective on its zero-padded shard ``qpad`` [per, width]."""
        import torch.distributed as dist

        kind, send, recv = self.xbuf[i]
        if kind == "a2a":  # chunk p = this rank's rows, column block p
            P, per, bw = send.shape
            send.copy_(qpad[:per].view(per, P, bw).transpose(0, 1))
            work = dist.all_to_all_single(recv, send, group=self.group, async_op=True)
        else:
            per = recv.shape[0] // self.world
            work = dist.all_gather_into_tensor(recv, qpad[:per], group=self.group, async_op=True)
        # rows arrive rank-major (self.place); the transforms / gather indices are laid out so
        return work, recv

    def operands(self, qs: list) -> list:
        T, be = self.T, self.be
        mats = []
        for i, q in enumerate(qs):
            q = q.contiguous()
            if self.transforms[i] is not None:
                W = self.transforms[i]
                a = be.empty((W.shape[1], q.shape[1]), T.float64)
                be.gemm_keyed(W, q, out=a, strideA=q.shape[1])
            else:
                a = be.gather_rows(q, self.gather_idx[i], self.gather_coef[i])
            mats.append(a)
        return mats

    N_PROBES = 16
    RANK_GIVE_UP = 3  # consecutive rejected host-path compressions after which a pipeline stops trying

    def _probes(self, n: int, device):
        """The fixed Gaussian probes, TRANSPOSED: [N_PROBES, n] (products with the wide operands go
        through _mm_nt: a plain [K, 2^16] @ [2^16, 16] GEMM runs on a handful of workgroups)."""
        if self._probe is None or self._probe.shape[1] != n:
            # the same fixed probes for every pipeline: drawn once per (n, device) in the process (the
            # 16 x 2^16 host draw and upload took ~10 ms of each new plan's first step)
            key = (n, str(device))
            with _PROBES_LOCK:
                hit = _PROBES.get(key)
                if hit is None:
                    T = self.T
                    g = T.Generator().manual_seed(1234)
                    hit = _PROBES[key] = T.randn((self.N_PROBES, n), generator=g, dtype=T.float64).to(device)
            self._probe = hit
        return self._probe

    def _prep_step(self, qs) -> PreparedStep:
        """The device data-rank preparation of one step: the sharded slice collectives, or the local
        chain (single mode, replicated slice mode)."""
        return self._prep_slice(qs) if self.mode == "slice" and self.sharded else self._prep_dev_rank(qs)

    def _launch_step(self, p: PreparedStep):
        return self._launch_slice(p) if self.mode == "slice" else self._launch_dev_rank(p)

    def knit(self, qs: list):
        if self.dev_rank and self.mode in ("single", "slice"):
            p = self._prep_step(qs)
            if self.out is None:
                self.out = self._alloc_out(None)
            return self._launch_step(p)
        mats = self.operands(qs)
        if self.out is None:
            self.out = self._alloc_out(mats)
        if self.mode == "slice":
            ia, ib = self.order[0], self.order[-1]
            return self._slice_exact(mats[ia], mats[ib], self.ops.clbits[ia], self.ops.clbits[ib])
        low = self._rank_compress(mats) if self.data_rank else None
        if self.record_events:
            start, end = self.be.event(), self.be.event()
            start.record()
        if low is not None:
            res = self._contract_lowrank(low[0])
        elif self.mode == "single" and len(self.order) == 2 and mats[self.order[0]].shape[0] <= 8:
            # already small-K (syc 32 1: one label, K = 1; a light-cone core of rank <= 8): the
            # write-bound kernels (blocked streaming knit when the fragments partition the output)
            res = self._contract_lowrank(mats)
        else:
            res = self._contract(mats)
        if self.record_events:
            end.record()
            self.events.append((start, end))
        if low is not None and not float(low[1]) <= max(self.rank_tol, self.rank_tol_rel * low[2]):
            # not numerically low-rank to the tolerance: exact contraction for this step; compression is
            # given up only after RANK_GIVE_UP consecutive rejections (a borderline step does not turn
            # the fast path off for the pipeline's life)
            self._rank_rejects += 1
            if self._rank_rejects >= self.RANK_GIVE_UP:
                self.data_rank = False
            self.rank_fallbacks += 1
            self.last_rank = None
            res = self._contract(mats)
        elif low is not None:
            self._rank_rejects = 0
        if self.mode == "reduce":
            import torch.distributed as dist

            dist.reduce(res, dst=0, group=self.group)
        return res

    def _fused_prep(self, qs) -> bool:
        """Whether the data-rank step takes the fused device preparation (qk_prep_operands ->
        qk_rank_factors -> qk_compress_operands -> qk_probe_errors): factored transforms on both sides, a backend
        with those kernels, and operand shapes they take."""
        ia, ib = self.order[0], self.order[-1]
        if "prep_operands" not in self.be.routes or self.transforms[ia] is None or self.transforms[ib] is None:
            return False
        K = self.transforms[ia].shape[1]
        return (self.transforms[ib].shape[1] == K and self.transforms[ia].shape[0] == qs[ia].shape[0]
                and self.transforms[ib].shape[0] == qs[ib].shape[0]
                and engine.prep_ok(K, qs[ia].shape[1], qs[ib].shape[1]))

    def _prep_fused(self, qs, probes):
        """(mats, G, U): light-cone operands of the two sides, their Grams [2, K, K] and the B side
        against the probes [K, 16], from one qk_prep_operands call."""
        ia, ib = self.order[0], self.order[-1]
        qa = qs[ia] if qs[ia].stride(1) == 1 else qs[ia].contiguous()
        qb = qs[ib] if qs[ib].stride(1) == 1 else qs[ib].contiguous()
        XA, XB, G, U = self.be.prep_operands(self.transforms[ia], qa, self.transforms[ib], qb, probes)
        mats = [None] * len(qs)
        mats[ia], mats[ib] = XA, XB
        self.last_prep = "fused"
        return mats, G, U

    def _accept(self, A, B, A2, B2, x, r, ref_rows=None, cmp_rows=None, reduce_err=None, note=True):
        """Device-side probe check of a compressed knit: ``(k_eff, err)``, ``k_eff`` = the rank when
        every probe's ``||(A^T B - A2^T B2) x||_2 <= rank_tol`` (see ``__init__``), else 0."""
        T = self.T
        if ref_rows is None:  # x: probes transposed, [N_PROBES, N]
            ref_rows = A.T @ _mm_nt(B, x)
            cmp_rows = A2.T @ _mm_nt(B2, x)
        e2 = T.cat([((ref_rows - cmp_rows) ** 2).sum(dim=0), (ref_rows ** 2).sum(dim=0)])
        if reduce_err is not None:
            e2 = reduce_err(e2)
        n = e2.numel() // 2
        err = e2[:n].max().sqrt()
        bound = T.clamp(self.rank_tol_rel * e2[n:].max().sqrt(), min=self.rank_tol)
        k_eff = T.where((err <= bound) & (r > 0), r, T.zeros_like(r))
        if note:
            self._note_rank(r, k_eff)
        return k_eff, err

    def _prep_dev_rank(self, qs) -> PreparedStep:
        """Single GPU, device data rank: operands + Grams + probe products (one fused launch where
        the shapes allow, else the transforms and torch products), qk_rank_factors with its
        acceptance check, compressed operands. Nothing waits for the host; ``sync_stats`` reads
        ranks / fallbacks later. The write (``_launch_dev_rank``) runs with the accepted rank and
        the exact contraction is predicated on it being 0."""
        ia, ib = self.order[0], self.order[-1]
        if self._fused_prep(qs):
            x = self._probes(qs[ib].shape[1], qs[ib].device)
            mats, G, U = self._prep_fused(qs, x)
            TA, TB, r = self.be.rank_factors(G[0], G[1])
            return self._compress_and_check(TA, TB, r, mats, U, x)
        mats = self.operands(qs)
        self.last_prep = "torch"
        A, B = mats[ia], mats[ib]
        G = self.T.stack([_mm_nt(A, A), _mm_nt(B, B)])
        TA, TB, r = self.be.rank_factors(G[0].contiguous(), G[1].contiguous())
        A2, B2 = (TA @ A).contiguous(), (TB @ B).contiguous()
        k_eff, _ = self._accept(A, B, A2, B2, self._probes(B.shape[1], B.device), r)
        return PreparedStep(A2, B2, k_eff, mats)

    def _compress_and_check(self, TA, TB, r, mats, U, x) -> PreparedStep:
        """The fused chain's compression and probe check: the compressed operands
        and the accepted rank of a prepared step. With the backend's fused form (compress_v) the check's V
        pass runs inside the compression. A replicated slice rank reads only A columns [base, base + n)
        (rows of R): it compresses those and checks those rows against every probe — its own slice's
        verdict, as each rank's rows in the sharded check; the Grams and factors stay whole, so its
        compressed values are the single-GPU ones bit for bit."""
        ia, ib = self.order[0], self.order[-1]
        a_cols = self._replicated_a_cols()
        kw = {"a_cols": a_cols} if a_cols is not None else {}
        cv = self.be.compress_v(TA, mats[ia], TB, mats[ib], x, **kw)
        check = {}
        if cv is not None:
            A2, B2, check["vpart"] = cv
        else:
            A2, B2 = self.be.compress(TA, mats[ia], TB, mats[ib], **kw)
        XA = mats[ia]
        if a_cols is not None:
            XA = XA[:, a_cols[0]:a_cols[0] + a_cols[1]]
            check["a2_cols"] = a_cols
        tally = self.be.fuses_tally  # the statistics in the accept kernel: one launch fewer
        if tally:
            check["tally"] = self._tally_for(r.device)
        _, k_eff, _ = self.be.probe_errors(XA, A2, U, B2, x, r=r, tol=self.rank_tol, rel_tol=self.rank_tol_rel,
                                           **check)
        if tally:
            self._pending += 1
        else:
            self._note_rank(r, k_eff)
        return PreparedStep(A2, B2, k_eff, mats)

    def _launch_dev_rank(self, p: PreparedStep):
        ia, ib = self.order[0], self.order[-1]
        cA, cB = self.ops.clbits[ia], self.ops.clbits[ib]
        if self.record_events:
            start, end = self.be.event(), self.be.event()
            start.record()
        self.last_kernel = self.be.outer_stream_kernel(p.A2.shape[0], cA, cB, self.N)
        self.be.knit_outer_stream(p.A2, p.B2, cA, cB, self.N, self.out, k_dev=p.k_eff)
        if self.record_events:
            end.record()
            self.events.append((start, end))
        return self._contract(p.mats, skip=p.k_eff)  # exact path: runs only if the check rejected

    def _broadcast_factors(self, TA, TB, r):
        """(TA, TB, r) of the first rank on every rank of the group: one broadcast of the three packed."""
        import torch.distributed as dist

        T = self.T
        R8, K = TA.shape
        fac = T.cat([TA.reshape(-1), TB.reshape(-1), r.to(T.float64)])
        dist.broadcast(fac, src=self._group_rank0(), group=self.group)
        return fac[:R8 * K].view(R8, K), fac[R8 * K:2 * R8 * K].view(R8, K), fac[-1:].to(T.int32)

    def _prep_slice(self, qs) -> PreparedStep:
        """Slice mode (multi-GPU), the preparation of this rank's write: ``qs`` hold every instance
        row of this rank's column block of each operand (the sweep's all_to_all). Collectives (fused
        preparation): one all_reduce of the two Grams + the B side against the probes, one
        all_gather of the compressed column blocks (rmax x 2^m per fragment), one MIN all_reduce of
        the ranks' accepted ranks (each checks its rows of R); every rank factors the identical
        all-reduced Grams with the same deterministic kernel (no broadcast unless QKNIT_SLICE_SYNC=1).
        The write itself is local. A rejected compression on any rank (read back after the write is
        queued) makes every rank take the exact contraction of its slice from all-gathered operands.
        The torch preparation broadcasts rank 0's factors instead."""
        import torch.distributed as dist

        T, be, P = self.T, self.be, self.world
        ia, ib = self.order[0], self.order[-1]
        bwA, bwB = qs[ia].shape[1], qs[ib].shape[1]
        x_full = self._probes(bwB * P, qs[ib].device)  # [N_PROBES, wB]
        if self._x_local is None or self._x_local.shape[1] != bwB:  # fixed probes: once
            self._x_local = x_full[:, self.rank * bwB:(self.rank + 1) * bwB].contiguous()
        x = self._x_local
        npr = self.N_PROBES
        fused = self._fused_prep(qs)
        if fused:
            mats, G, U = self._prep_fused(qs, x)
            XA, XB = mats[ia], mats[ib]
            K = XA.shape[0]
            red = _joined(T, G, U)
            dist.all_reduce(red, group=self.group)
            G = red[:2 * K * K].view(2, K, K)
            U = red[2 * K * K:].view(K, npr).contiguous()
            TA, TB, r = be.rank_factors(G[0].contiguous(), G[1].contiguous())
            if self.slice_sync:
                TA, TB, r = self._broadcast_factors(TA, TB, r)
            A2l, B2l = be.compress(TA.contiguous(), XA, TB.contiguous(), XB)
            loc = _joined(T, A2l, B2l)
        else:
            mats = self.operands(qs)
            self.last_prep = "torch"
            XA, XB = mats[ia], mats[ib]  # [K, wA / P], [K, wB / P]
            K = XA.shape[0]
            red = T.cat([_mm_nt(XA, XA).reshape(-1), _mm_nt(XB, XB).reshape(-1), _mm_nt(XB, x).reshape(-1)])
            dist.all_reduce(red, group=self.group)
            GA = red[:K * K].view(K, K).contiguous()
            GB = red[K * K:2 * K * K].view(K, K).contiguous()
            Bx = red[2 * K * K:].view(K, npr)
            TA, TB, r = self._broadcast_factors(*be.rank_factors(GA, GB))
            loc = T.cat([(TA @ XA).reshape(-1), (TB @ XB).reshape(-1)])
        R8 = TA.shape[0]
        gat = T.empty(P * loc.numel(), dtype=loc.dtype, device=loc.device)
        dist.all_gather_into_tensor(gat, loc, group=self.group)
        gat = gat.view(P, loc.numel())
        A2 = gat[:, :R8 * bwA].view(P, R8, bwA).permute(1, 0, 2).reshape(R8, P * bwA).contiguous()
        B2 = gat[:, R8 * bwA:].view(P, R8, bwB).permute(1, 0, 2).reshape(R8, P * bwB).contiguous()
        if fused:
            # this rank's A columns (its rows of R) against all probes (B2 / probes: every column)
            # (the accepted rank from the same launch chain: no separate accept kernel)
            _, k_eff, _ = be.probe_errors(XA, A2, U, B2, x_full.contiguous(), r=r, tol=self.rank_tol,
                                          a2_cols=(self.rank * bwA, bwA), rel_tol=self.rank_tol_rel)
        else:
            # rows of R in this rank's A column block, against all probes
            ref_rows = XA.T @ Bx
            cmp_rows = A2[:, self.rank * bwA:(self.rank + 1) * bwA].T @ _mm_nt(B2, x_full)
            k_eff, _ = self._accept(None, None, None, None, None, r, ref_rows, cmp_rows, note=False)
        # one decision for every rank: the accepted rank only if every rank's rows of R passed (the A
        # column blocks cover all of R; the ranks' factors are identical, so the local ranks are r or 0).
        # A rejection anywhere makes every rank take the exact slice, whose collectives then match.
        dist.all_reduce(k_eff, op=dist.ReduceOp.MIN, group=self.group)
        self._note_rank(r, k_eff)  # the decision every rank takes
        if self.slice_exact == "host":
            # round-3 form: the host reads the (MIN-reduced) verdict after queueing the write and
            # gathers the exact slice's operands only on a rejection (no per-step gather)
            on_gpu = k_eff.device.type == "cuda"
            pinned = T.empty(1, dtype=T.int32, pin_memory=on_gpu)
            pinned.copy_(k_eff, non_blocking=on_gpu)
            ready = T.cuda.Event() if on_gpu else None
            if on_gpu:
                ready.record()
            return PreparedStep(A2, B2, k_eff, mats, host_verdict=(pinned, ready))
        # the exact slice's operands, gathered every step (the same collectives on every rank whatever
        # the verdict; the contraction itself is predicated on the device, _launch_slice); started
        # asynchronously, so the write does not wait for them — only the predicated contraction does
        return PreparedStep(A2, B2, k_eff, mats, exact=self._slice_exact_operands(XA, XB, async_op=True))

    def _launch_slice(self, p: PreparedStep):
        be = self.be
        ia, ib = self.order[0], self.order[-1]
        cA, cB = self.ops.clbits[ia], self.ops.clbits[ib]
        o_begin, o_count = self.slice
        if self.record_events:
            start, end = be.event(), be.event()
            start.record()
        self.last_kernel = be.outer_stream_kernel(p.A2.shape[0], cA, cB, self.N, o_begin, o_count)
        be.knit_outer_stream(p.A2, p.B2, cA, cB, self.N, self.out, o_begin=o_begin, o_count=o_count, k_dev=p.k_eff)
        if self.record_events:
            end.record()
            self.events.append((start, end))
        if not self.sharded:
            # replicated preparation: every rank holds the whole transformed operands, so the exact
            # slice (predicated on this rank's own verdict over its slice's rows) reads its columns in
            # place — no collective. Pipelined steps queue it before the write (_step_overlapped)
            if p.exact_queued:
                return self.out
            A, kA, B, kB = self._slice_exact_operands(*self._exact_mats(p))
            be.gemm_keyed(A, B, keyA=kA, keyB=kB, out=self.out, skip=p.k_eff)
            return self.out
        if p.host_verdict is not None:  # slice_exact == "host"
            pinned, ready = p.host_verdict
            if ready is not None:
                ready.synchronize()  # the check only, not the knit queued behind it
            if int(pinned[0]) == 0:
                self._slice_exact(*self._exact_mats(p), cA, cB)
            return self.out
        # exact contraction of this slice, predicated on the device: runs only when the (MIN-reduced)
        # accepted rank is 0 — no host round trip, the verdict is read later by sync_stats
        A, kA, B, kB = p.exact()
        be.gemm_keyed(A, B, keyA=kA, keyB=kB, out=self.out, skip=p.k_eff)
        return self.out

    # ------------------------------------------------------------------ overlapped steps
    def overlap_ok(self) -> bool:
        """Whether steps can be software-pipelined (``step(overlap=True)``): the device data-rank
        path (single or slice mode) on a GPU backend, so everything before the write is stream work."""
        return bool(self.dev_rank and self.mode in ("single", "slice") and self.be.dev is not None
                    and self.be.dev.type == "cuda")

    # CUs of the preparation stream in a pipelined step (QKNIT_PREP_CUS; 0: no CU split). rank_sim, 8
    # ranks, modelled xGMI: 48 / 64 / 96 CUs -> 1.20 / 1.02 / 0.96 ms per step (the sweep on 32 CUs took
    # 0.7 ms); one GPU: 64 and 96 alike (6.27 / 6.28 ms), 128 slower (6.59: the write on 128 CUs)
    PREP_CUS = 96

    def _overlap_streams(self):
        """(prep stream, write stream) of pipelined steps. With ``QKNIT_PREP_CUS`` = c > 0 (default
        PREP_CUS) both are CU-masked HIP streams (qk_stream_create_cu_masked): the preparation runs
        on c CUs (c / 8 of every XCD), the write-bound knit on the rest, so neither waits for the other's workgroups to drain; c = 0: a plain side stream for the
        preparation and the caller's stream for the write."""
        if self._prep_stream is None:
            T = self.T
            dev = self.be.dev.index or 0
            # 4+ ranks: 128 preparation CUs (the replicated sweep + chain on 96 left the write waiting: 8
            # ranks 0.82-0.86 vs 0.82-0.85 ms per step with three buffers, profiles/r05j_*; 4 ranks
            # 1.319-1.322 vs 1.349-1.378 ms, r05az_*), 2 ranks PREP_CUS (2.533-2.546 vs 2.545-2.561 at 128,
            # r05ba_*)
            env = os.environ.get("QKNIT_PREP_CUS", str(128 if self.world >= 4 else self.PREP_CUS))
            total = engine.device_cu_count(dev)
            if env == "all":
                # no CU split: both streams may use every CU (their own hardware queues); the write's
                # grid (QKNIT_OB_WG_PER_CU) decides how many slots per CU it holds, the preparation
                # takes the others
                every = tuple(range(total))
                self._prep_stream = engine.cu_masked_stream(dev, every)
                self._write_stream = engine.cu_masked_stream(dev, every, tag=100)
                self._write_cus = every
                self.overlap_cus = (total, total)
                self._prep_stream.wait_stream(T.cuda.current_stream())
                return self._prep_stream, self._write_stream
            c = int(env)
            if 0 < c < total:
                # the top c logical CUs. The CU-mask bits of a stream are dealt over the XCDs (bit i ->
                # XCD i % 8, CU i // 8 of it; tools/cu_mask_probe.py): a contiguous block of bits is
                # the same few CUs of every XCD, while a mask leaving some XCD no CU leaves that XCD
                # unrestricted (every-8th-bit masks confined nothing)
                prep = tuple(range(total - c, total))
                write = tuple(i for i in range(total) if i not in set(prep))
                self._prep_stream = engine.cu_masked_stream(dev, prep)
                self._write_stream = engine.cu_masked_stream(dev, write)
                self._write_cus = write
                self.overlap_cus = (len(prep), len(write))
            else:  # no CU split: a plain side stream for the preparation, the write on the caller's stream
                self._prep_stream = T.cuda.Stream(device=self.be.dev)
                self.overlap_cus = (0, total)
            self._prep_stream.wait_stream(T.cuda.current_stream())  # plan uploads before the first step
        return self._prep_stream, self._write_stream

    def _step_overlapped(self):
        """One step with its sweep + operand transforms + data-rank compression (+ the slice
        collectives) on the preparation stream and the write on the write stream (``_overlap_streams``),
        so the preparation of this step runs while the previous step's write still streams: the write
        is HBM-bound, the sweep VALU-bound. Buffers the write reads are tensors of this step, handed to
        the write stream with record_stream; the sweep buffers are only touched on the preparation
        stream (in order). The caller's stream waits for the write before the step returns."""
        T, be = self.T, self.be
        main = T.cuda.current_stream()
        if main.cuda_stream == 0:
            # the CU-masked streams are blocking streams: anything queued on the legacy null stream
            # (here: the caller's wait for the write) would order the next step's preparation behind
            # this step's write and undo the overlap
            raise ValueError("pipelined steps need a non-default current stream (torch.cuda.stream(...))")
        if self.out is None:
            # the first step runs plain (it allocates the output); the pipelined steps after it write
            # into that buffer
            return self.knit(self.sweep())
        S, W = self._overlap_streams()
        W = W if W is not None else main
        # the caller's reads of an output buffer are queued on its stream after the step that wrote it
        # returned; the write that reuses the buffer (next step with one buffer, the one after with two)
        # waits for an event the caller's stream records at the start of step j - buffers + 1, which
        # follows every read queued before that call, and not for the other buffer's write (so step j's
        # write may still start under step j - 1's)
        started = T.cuda.Event()
        started.record(main)
        self._started = (self._started + [started])[-max(self.out_buffers, 1):]
        if self.out_buffers > 1:
            nb = self.out_buffers
            self._ensure_outs(W, main)
            k = self._flip
            self._flip = (self._flip + 1) % nb
            self.out, W = self._outs[k], self._wstreams[k]
        with T.cuda.stream(S):
            be.bind()
            if self.record_events:
                s0, s1 = be.event(), be.event()
                s0.record()
            qs = self.sweep()
            if self.record_events:
                s1.record()
                self.sweep_events.append((s0, s1))
            if self.out is None:
                self.out = self._alloc_out(None)
            p = self._prep_step(qs)
            if self._exact_before_write(W, main):
                # replicated slice: the predicated exact slice (a no-op unless the check rejected) on the
                # preparation stream ahead of the write, which then skips (device K = 0). Behind the write
                # on its own stream it waited ~100 us per step for CU slots under the other buffers'
                # writes and the buffer's next write waited for it (profiles/r05k_*); here it waits only
                # for the caller to release the buffer, as the write does
                if len(self._started) == max(self.out_buffers, 1):
                    S.wait_event(self._started[0])
                A, kA, B, kB = self._slice_exact_operands(*self._exact_mats(p))
                be.gemm_keyed(A, B, keyA=kA, keyB=kB, out=self.out, skip=p.k_eff)
                p.exact_queued = True
            done = T.cuda.Event(enable_timing=self.record_events)
            done.record(S)
        if self.record_events:
            self.prep_events.append((s1, done))
        with T.cuda.stream(W):
            W.wait_event(done)
            if W is not main and len(self._started) == max(self.out_buffers, 1):
                W.wait_event(self._started[0])
            be.bind()
            for t in (p.A2, p.B2, p.k_eff, *p.mats):
                if t is not None:
                    t.record_stream(W)
            out = self._launch_step(p)
        if W is not main:
            main.wait_stream(W)
        be.bind()
        return out

    def _replicated_a_cols(self):
        """(base, n): the A columns this rank's output slice reads in replicated slice mode, when that is
        fewer than all of them (syc 32 5 at 8 ranks: 2^13 of 2^16); else None. QKNIT_SLICE_A_COLS=0
        compresses and checks all columns (A/B)."""
        if self.mode != "slice" or self.sharded or os.environ.get("QKNIT_SLICE_A_COLS") == "0":
            return None
        base, n = self._slice_exact_plan()[0][:2]
        width = 1 << len(self.ops.clbits[self.order[0]])
        return (base, n) if n < width and n % 16 == 0 else None

    def _ensure_outs(self, W, main) -> None:
        """The output buffers pipelined steps rotate through (out_buffers > 1: the current one and
        out_buffers - 1 more, each made as _alloc_out makes it) and one write stream per buffer (W first),
        made once."""
        if self._outs is not None or self.out_buffers <= 1:
            return
        T, nb = self.T, self.out_buffers
        self._outs = [self.out] + [self._alloc_out(None) for _ in range(nb - 1)]
        dev = self.be.dev.index or 0
        self._wstreams = ([W] + [engine.cu_masked_stream(dev, self._write_cus, tag=t) for t in range(1, nb)]
                          if self._write_cus else [T.cuda.Stream(device=self.be.dev) for _ in range(nb)])
        for w in self._wstreams:
            w.wait_stream(main)

    def prepare_pipelined(self) -> None:
        """Make now what pipelined steps would make on their first runs — the rotating output buffers
        (each write-rate selected: mappings and probe writes) and their streams — so that later steps
        allocate nothing; bench.py calls it after its warmup steps, so a timed region never holds a buffer
        selection whatever the warmup count. Needs one step done (the first step runs plain and makes
        the first buffer); a no-op without ``overlap`` or before that step."""
        if (not self.overlap or not self.overlap_ok() or self.out is None or self.out_buffers <= 1
                or self._outs is not None):
            return
        main = self.T.cuda.current_stream()
        _, W = self._overlap_streams()
        self._ensure_outs(W if W is not None else main, main)

    def _exact_before_write(self, W, main) -> bool:
        """Whether a pipelined step queues its predicated exact contraction on the preparation stream
        before the write (replicated slice mode, the write on its own stream; QKNIT_EXACT_BEFORE_WRITE=0
        keeps it behind the write). Valid because the write kernels skip all work at device K = 0,
        the verdict on which the exact contraction runs."""
        return (self.mode == "slice" and not self.sharded and W is not main and self.dev_rank
                and os.environ.get("QKNIT_EXACT_BEFORE_WRITE", "1") != "0")

    def _group_rank0(self) -> int:
        import torch.distributed as dist

        return 0 if self.group is None else dist.get_global_rank(self.group, 0)

    def _slice_exact_plan(self):
        """Per side of the exact slice contraction: (the output bits' column range [base, base + n) of
        that side this rank's slice reads, whether it is the rank's own column block, device keys of
        those columns relative to the slice start). Built once."""
        if self._exact_plan is None:
            from .knit_plan import deposit_keys

            o_begin, o_count = self.slice
            plan = []
            for i in (self.order[0], self.order[-1]):
                cl = self.ops.clbits[i]
                m = sum(1 << c for c in cl)
                n = 1 << bin(m & (o_count - 1)).count("1")
                base = _pext(o_begin, m)
                w = 1 << len(cl)
                local = n == w // self.world and base == self.rank * n
                keys = deposit_keys(list(cl))[base:base + n] - (o_begin & m)
                plan.append((base, n, local, self.be.to_device(np.ascontiguousarray(keys))))
            self._exact_plan = plan
        return self._exact_plan

    def _slice_exact_operands(self, XA, XB, async_op: bool = False):
        """(A, keyA, B, keyB) of this rank's exact slice from the transformed column blocks ``XA`` /
        ``XB`` [K, w / P]: a side whose columns are this rank's own block is used as it is, the other
        side is all-gathered (syc 32 at 2-8 ranks: the slice's fixed output bits are A's top bits, so
        only B travels, K x 2^16 doubles per step). ``async_op``: the gathers are started and a
        finisher returned instead — called on the stream that needs the operands, it makes that
        stream wait for them (their column reorder runs on a helper stream that waits for the gather,
        so it overlaps whatever runs meanwhile, the write in pipelined steps)."""
        if not self.sharded:  # replicated preparation: whole operands on every rank, the slice's columns in place
            parts = []
            for X, (base, n, _, keys) in zip((XA, XB), self._slice_exact_plan()):
                parts += [X[:, base:base + n], keys]
            return tuple(parts)
        import torch.distributed as dist

        T, P = self.T, self.world
        parts, pend = [], []
        for X, (base, n, local, keys) in zip((XA, XB), self._slice_exact_plan()):
            if local:
                parts += [X, keys]
                continue
            K, bw = X.shape
            g = T.empty((P * K * bw,), dtype=X.dtype, device=X.device)
            work = dist.all_gather_into_tensor(g, X.contiguous().reshape(-1), group=self.group, async_op=async_op)
            pend.append((len(parts), g, work, K, bw, base, n))
            parts += [None, keys]

        def reorder(g, K, bw, base, n):
            return g.view(P, K, bw).permute(1, 0, 2).reshape(K, P * bw)[:, base:base + n].contiguous()

        if not async_op:
            for i, g, _, K, bw, base, n in pend:
                parts[i] = reorder(g, K, bw, base, n)
            return tuple(parts)
        on_gpu = XA.device.type == "cuda"
        if on_gpu:
            if self._exact_stream is None:
                self._exact_stream = T.cuda.Stream(device=XA.device)
            H = self._exact_stream
            H.wait_stream(T.cuda.current_stream())
            with T.cuda.stream(H):
                for i, g, work, K, bw, base, n in pend:
                    work.wait()  # H waits for the gather, the host does not
                    parts[i] = reorder(g, K, bw, base, n)
                    g.record_stream(H)
            done = T.cuda.Event()
            done.record(H)
        else:
            for i, g, work, K, bw, base, n in pend:
                work.wait()
                parts[i] = reorder(g, K, bw, base, n)

        def finish():
            if on_gpu:
                T.cuda.current_stream().wait_event(done)
                for t in parts:
                    if t is not None:
                        t.record_stream(T.cuda.current_stream())
            return tuple(parts)

        return finish

    def _exact_mats(self, p: PreparedStep):
        """(X_A, X_B): the transformed operands of a prepared step, row side first."""
        return p.mats[self.order[0]], p.mats[self.order[-1]]

    def _slice_exact(self, XA, XB, cA, cB):
        """Exact contraction of this rank's output slice (K terms) from the transformed column blocks
        (the slice path without data rank); collectives as :meth:`_slice_exact_operands`."""
        A, kA, B, kB = self._slice_exact_operands(XA, XB)
        self.last_kernel = None
        return self.be.gemm_keyed(A, B, keyA=kA, keyB=kB, out=self.out)

    def _tally_for(self, device):
        """The device tally of the data-rank statistics (_note_rank), created on first use."""
        if self._tally is None or self._tally.device != device:
            self._tally = self.T.zeros(4, dtype=self.T.int64, device=device)
        return self._tally

    def _note_rank(self, r, k_eff):
        """A device-rank step's verdict into the device-side tally (no host read: the loop of steps never
        waits for the device; round 4 read every 32 steps back, which drained the pipelined multi-GPU
        queue each time). In slice mode k_eff is MIN-all-reduced in place afterwards, so the tally is
        queued there after that reduction (_prep_slice)."""
        self.be.rank_tally(r, k_eff, self._tally_for(k_eff.device))
        self._pending += 1

    def sync_stats(self):
        """Read back the device tally of the steps since the last call (host sync): ``last_rank``
        (accepted rank, or None when the last step fell back), ``rank_fallbacks`` (probe check rejected),
        ``rank_incompressible`` (no factorisation of rank <= 8: the exact contraction)."""
        if self._pending and self._tally is not None:
            acc = self._tally.cpu().numpy()
            d = acc - self._tally_read
            self.rank_incompressible += int(d[0])
            self.rank_fallbacks += int(d[1])
            self.last_rank = int(acc[2]) if acc[2] > 0 else None
            self._tally_read = acc
        self._pending = 0
        return self.last_rank, self.rank_fallbacks

    def _rank_compress(self, mats):
        """Two-fragment knit R = A^T B ([K, M], [K, N] operands) rewritten as A''^T B'' with
        r = numerical rank of R rows (engine.data_rank_factors on the two K x K Gram matrices,
        read back once per step). Returns ``(mats'', err, ref)`` — err a device scalar: the largest
        ||(R - A''^T B'') x||_2 over the N_PROBES (16) fixed Gaussian probes x (an estimate of the Frobenius
        norm of the error, computed directly in fp64, no Gram squaring), ref the largest ||R x||_2 — or
        None when the compression would not shrink K."""
        T = self.T
        ia, ib = self.order[0], self.order[-1]
        A, B = mats[ia], mats[ib]
        if self.mode == "gather" and not self.split_a:  # this rank's block of output rows
            lo, hi = self.row_block
            A = A[:, lo:hi].contiguous()
        K = A.shape[0]
        xt = self._probes(B.shape[1], B.device)
        # Grams first, their readback started at once; the probe reference runs on the GPU while
        # the host factorises (no pageable copies: they would wait for the whole queue)
        G = T.stack([_mm_nt(A, A), _mm_nt(B, B)])
        on_gpu = G.device.type == "cuda"
        if self._pinned is None or self._pinned.shape != G.shape:
            self._pinned = T.empty(G.shape, dtype=G.dtype, pin_memory=on_gpu)
        self._pinned.copy_(G, non_blocking=on_gpu)
        ready = T.cuda.Event() if on_gpu else None
        if on_gpu:
            ready.record()
        ref = A.T @ _mm_nt(B, xt)
        if on_gpu:
            ready.synchronize()
        Gh = self._pinned.numpy()
        f = engine.data_rank_factors(Gh[0], Gh[1], rmax=K, rc_max=K)
        if f is None or f[0].shape[0] >= K:
            self.last_rank = K
            return None
        r = f[0].shape[0]
        tt = T.from_numpy(np.concatenate([f[0], f[1]]))
        if on_gpu:
            tt = tt.pin_memory()
        tt = tt.to(A.device, non_blocking=on_gpu)
        TA, TB = tt[:r], tt[r:]
        A2, B2 = (TA @ A).contiguous(), (TB @ B).contiguous()
        err = (A2.T @ _mm_nt(B2, xt) - ref).norm(dim=0).max()
        self.last_rank = A2.shape[0]
        out = list(mats)
        out[ia], out[ib] = A2, B2
        return out, err, float(ref.norm(dim=0).max())

    def _contract_lowrank(self, mats):
        """Contraction of the rank-compressed pair, r <= 8: the two fragments' clbits partition
        the output bits (clbit 0 on the N side) -> the streaming small-K knit (output order,
        contiguous stores); else the N side pairing adjacent outputs -> the keyed small-K outer
        product (both output-write bound); otherwise the operands are zero-padded to a multiple of 16 terms for the MFMA
        kernel."""
        T = self.T
        ia, ib = self.order[0], self.order[-1]
        A, B = mats[ia], mats[ib]
        r = A.shape[0]
        if self.mode == "gather":  # compact [rows, 2^m_B] block: affine keys, K <= 8 -> small-K kernel
            pad = (-r) % 16 if r > 8 else 0
            if pad:
                A = T.cat([A, A.new_zeros((pad, A.shape[1]))])
                B = T.cat([B, B.new_zeros((pad, B.shape[1]))])
            self.last_kernel = "qk_gemm_smallk_kernel" if r <= 8 else None
            return self.be.gemm_keyed(A.contiguous(), B.contiguous(), keyA=None, strideA=B.shape[1], keyB=None,
                                      strideB=1, out=self.out)
        cA, cB = self.ops.clbits[ia], self.ops.clbits[ib]
        stream = os.environ.get("QKNIT_OUTER", "stream") == "stream"  # "paired": keyed kernel (A/B timing)
        if stream and r <= 8 and engine.stream_knit_ok(cA, cB, self.N) and "knit_outer_stream" in self.be.routes:
            self.last_kernel = self.be.outer_stream_kernel(r, cA, cB, self.N)
            return self.be.knit_outer_stream(A, B, cA, cB, self.N, self.out)
        if r <= 8 and engine.paired_keys(cB) and "gemm_outer_paired" in self.be.routes:
            st = engine._affine_stride(cA)
            kA = None if st is not None else engine._device_keys(tuple(cA), None, None, A.device)
            kB = engine._device_keys(tuple(cB), None, None, B.device)
            self.last_kernel = "qk_gemm_smallk_kernel<true>"
            return self.be.gemm_outer_paired(A, B, kB, keyA=kA, strideA=st or 0, out=self.out)
        self.last_kernel = None
        pad = (-r) % 16
        if pad:
            A = T.cat([A, A.new_zeros((pad, A.shape[1]))])
            B = T.cat([B, B.new_zeros((pad, B.shape[1]))])
        out = list(mats)
        out[ia], out[ib] = A, B
        return self._contract(out)

    # The output buffer (round 4): the write kernel's rate depends on the 2^N buffer — 4.8-5.0 ms for
    # most 34 GB buffers, 5.2-5.9 ms for others, fixed per buffer, for hipMalloc blocks and 1-GiB-chunk
    # mappings alike and for every store order tried. Large outputs are mapped from 1-GiB
    # chunks (qk_out_alloc) and kept only if the knit's store order writes fast into them
    # (engine.out_buffer: at most OUT_TRIES candidates, the fastest kept); small ones come from torch.

    def _alloc_out(self, mats):
        """This rank's output buffer: 2^N entries (single / reduce), its slice (slice mode), or its block
        of output rows (gather mode, zeroed). Zero-filled unless every output is written by the knit."""
        if self.mode == "slice":
            n = self.slice[1]
        elif self.mode != "gather":
            n = 1 << self.N
        else:
            lo, hi = self.row_block
            n = max(hi - lo, 1) * mats[self.order[-1]].shape[1]
        return self.new_out(n, zero=self.mode == "gather" or not self.covers_outputs())

    def new_out(self, n: int, zero: bool = False, select: bool = True):
        """A fresh [n] fp64 device buffer for the knit output (engine.out_buffer: 1-GiB-mapped when
        large; a host backend's own allocation in the CPU tests). ``self.out_alloc`` records how.
        ``select=False``: a large mapping is not write-rate checked (take_out's first call)."""
        if "out_buffer" not in self.be.routes:  # a host backend's own allocation
            self.out_alloc = "backend"
            self._last_owner = None
            return self.be.zeros((n,), self.T.float64) if zero else self.be.empty((n,), self.T.float64)
        n_sel = len(engine.out_selections)
        out, owner = self.be.out_buffer(n, select=select)
        self.out_alloc = "qk_out_alloc (1-GiB mapped chunks)" if owner is not None else "torch"
        if len(engine.out_selections) > n_sel:  # candidates' write rates, the kept one first
            last = engine.out_selections[-1]
            self.out_alloc += f" ({last[0]})" if owner is None else f", write-rate selected: {last} GB/s"
        if owner is not None:
            st = engine.out_stats()
            self.out_alloc += (f"; process: {st['reserved']} reservations ({st['reserve_failed']} failed), "
                               f"{st['live']} live, {st['retired']} retired "
                               f"({st['retired_bytes'] / 2**30:.0f} GiB of address space)")
        self._last_owner = owner
        if zero:
            out.zero_()
        return out

    def take_out(self, defer_select: bool = False):
        """The output buffer of one drop-in call (run.run_virtual_circuit): the previous call's mapping
        again once the caller has dropped every tensor over it (the reference returns a fresh result
        per call, and mapping 34 GB costs milliseconds), else a new buffer. ``defer_select`` (one-GPU
        drop-in): the first buffer is not write-rate checked; the caller times the call's write and
        reports it (:meth:`note_call_write`), and a slow buffer is replaced at a later call."""
        n = self.slice[1] if self.mode == "slice" else 1 << self.N
        zero = not self.covers_outputs()
        own = self._call_owner
        if own is not None and own.n == n and not own.in_use():
            if getattr(own, "write_gbs", None) is None or own.write_gbs >= engine.OUT_FAST_GBS:
                out = own.tensor()
                if zero:
                    out.zero_()
                return out
            # the first call's own write into its un-timed mapping was slow (the buffer lottery, DESIGN
            # §4): this call takes a write-rate-selected mapping instead
            self._call_owner = own = None
            select = True
        else:
            # the first call maps one buffer without timing it (engine.out_buffer select=False) and
            # times its own write instead (note_call_write): the selection's extra mappings and probe
            # launches (~20 ms at 2^32 outputs) move to a later call, and only if that write was slow
            select = own is not None or not defer_select
        out = self.new_out(n, zero=zero, select=select)
        self._call_owner = self._last_owner
        if self._call_owner is not None and not select:
            self._call_owner.write_gbs = None
            self._time_call_write = True
        return out

    def note_call_write(self, events_before: int):
        """After a drop-in call whose output mapping was not write-rate checked (take_out): the rate of
        the call's own write (its HIP events) decides whether later calls keep the mapping."""
        if not self._time_call_write:
            return
        self._time_call_write = False
        own = self._call_owner
        ev = self.events[events_before:]
        if own is None or not ev:
            return
        ms = ev[-1][0].elapsed_time(ev[-1][1])
        M, N, _ = self.gemm_shape()
        own.write_gbs = 8.0 * M * N / (ms * 1e-3) / 1e9 if ms > 0 else float("inf")
        if own.write_gbs < engine.OUT_FAST_GBS:
            # a later call swaps it for a selected one (own.write_gbs stays below the stop)
            engine.out_selections.append([f"drop-in first call: un-timed mapping wrote at {own.write_gbs:.1f} GB/s, "
                                          "replaced on the next call"])

    def _contract(self, mats, skip=None):
        if self.mode != "gather":
            gemm = self.be.gemm_keyed if skip is None else (lambda A, B, **kw: self.be.gemm_keyed(A, B, skip=skip, **kw))
            return engine.contract(None, mats, self.ops.clbits, self.out, gemm=gemm, kr=self.be.khatri_rao)
        # output-sharded: compact [rows, 2^m_B] block in (x_A, x_B) order
        order = self.order
        A = mats[order[0]]
        for i in order[1:-1]:
            A = self.be.khatri_rao(A.contiguous(), mats[i].contiguous())
        B = mats[order[-1]]
        lo, hi = self.row_block
        if not self.split_a:  # split A side: the exchange delivered only this block
            A = A[:, lo:hi]
        A = A.contiguous()
        return self.be.gemm_keyed(A, B.contiguous(), keyA=None, strideA=B.shape[1], keyB=None, strideB=1,
                                  out=self.out)

    def plan_bytes(self) -> int:
        """Device bytes the plan holds between steps (job tables, sweep rows and workspaces, knit
        transforms); the output buffer is not counted (run_into: the caller's)."""
        seen, total = set(), 0
        for sw in self.sweeps:
            if sw is None:
                continue
            for k in ("slot", "sign", "off", "pjob", "q", "ws"):
                t = sw.get(k)
                if t is not None and hasattr(t, "data_ptr") and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    total += t.numel() * t.element_size()
        for W in self.transforms:
            if W is not None:
                total += W.numel() * W.element_size()
        return total

    def covers_outputs(self) -> bool:
        """Whether one knit writes every output this rank owns: the live fragments' clbits cover all
        N output bits (in single / slice mode every kernel of the knit then stores each output once,
        overwriting), so the caller may hand an uninitialised buffer to :meth:`run_into`."""
        bits = set()
        for i, fs in enumerate(self.frags):
            if not fs.dropped:
                bits |= set(self.ops.clbits[i])
        return self.mode in ("single", "slice") and bits == set(range(self.N))

    def run_into(self, out):
        """One step writing the distribution into the caller's ``out`` (2^N fp64, or this rank's slice);
        the pipeline keeps no reference to it afterwards (the drop-in ``run_virtual_circuit`` returns a
        fresh buffer per call, and the caching allocator hands the previous call's block back)."""
        self.out = out
        try:
            self.step()
        finally:
            self.out = None
        return out

    def _select_pair(self):
        """(row side, column side) fragment indices when the dict result can be selected straight
        from the two knit operands (qk_knit_select): two live fragments, ascending disjoint clbits."""
        live = [i for i, fs in enumerate(self.frags) if not fs.dropped]
        if self.mode != "single" or len(live) != 2 or len(self.order) != 2 or "knit_select" not in self.be.routes:
            return None
        ia, ib = self.order[0], self.order[-1]
        cA, cB = list(self.ops.clbits[ia]), list(self.ops.clbits[ib])
        if cA != sorted(cA) or cB != sorted(cB) or set(cA) & set(cB):
            return None
        return ia, ib

    def knit_dict(self, accuracy: float, qs=None):
        """The reference-shaped result of one step (``run.py:71``: ``QuasiDistr`` truncation at
        ``accuracy``, ``quasi_distr.py:7-10``, then ``nearest_probability_distribution``,
        ``:28-43``) as host ``(keys, values)`` ascending by value. Where the knit is small-K — the
        device data rank accepted a compression (syc 32), or the light-cone knit has K <= 8 terms
        (hwe, bv) — only the entries above ``accuracy`` are formed and kept (qk_knit_select) and
        NPD runs on those (qk_npd_pairs): the 2^N vector is never written. Otherwise (rejected
        compression, more than two fragments, K > 8) the dense knit into a scratch buffer, then
        qk_threshold_count + qk_npd."""
        if qs is None:
            qs = self.sweep()
        if self.mode == "slice":
            return self._knit_dict_slice(accuracy, qs)
        pair = self._select_pair()
        if pair is not None and self.dev_rank:
            p = self._prep_dev_rank(qs)
            ia, ib = pair
            keys, vals = self.be.knit_select(p.A2, p.B2, self.ops.clbits[ia], self.ops.clbits[ib], self.N,
                                             accuracy, k_dev=p.k_eff)
            self.last_kernel = "qk_knit_select_kernel"
            if int(p.k_eff.reshape(-1)[0]) > 0:
                return self.be.npd_pairs(keys, vals)
            mats = p.mats  # rejected compression: the exact contraction, dense
        else:
            mats = self.operands(qs)
            if pair is not None and mats[pair[0]].shape[0] <= 8:
                ia, ib = pair
                keys, vals = self.be.knit_select(mats[ia].contiguous(), mats[ib].contiguous(), self.ops.clbits[ia],
                                                 self.ops.clbits[ib], self.N, accuracy)
                self.last_kernel = "qk_knit_select_kernel"
                return self.be.npd_pairs(keys, vals)
        keep = self.out
        self.out = self.be.zeros((1 << self.N,), self.T.float64)
        try:
            dense = self._contract(mats)
            self.last_kernel = None
            return self.be.npd_dense(dense, accuracy)
        finally:
            self.out = keep

    def _knit_dict_slice(self, accuracy: float, qs):
        """knit_dict in slice mode (multi-GPU; every rank returns the whole result, ``run.py:71``): each
        rank selects the entries above ``accuracy`` of its own output slice — from the compressed
        operands (qk_knit_select on the slice's column ranges: its keys are the slice-local outputs'
        keys plus the slice start, since the slice's fixed bits and the ranges' own bits are disjoint)
        or, after a rejected compression, from its exact dense slice (qk_select_above) —, the kept
        pairs of all ranks are all-gathered, and every rank runs the NPD of the union (qk_npd_pairs:
        sorted by key, then by value, so the order of the union does not matter). The slices partition
        the outputs, so the union is exactly the single-GPU selection, bit for bit, whenever every
        rank's compression verdict matches the single-GPU one. Replicated preparation: each rank checks
        only its own slice's rows (against a bound scaled by the probes' ||R p|| over those rows), so
        a rank may accept where the single-GPU check rejects or the reverse; every kept entry is then
        still within the check's 10 tol of the exact knit, but not necessarily the
        single-GPU bits. (Sharded preparation takes the MIN verdict over the ranks.)"""
        import torch.distributed as dist

        T, be = self.T, self.be
        ia, ib = self.order[0], self.order[-1]
        o_begin, o_count = self.slice
        p = self._prep_step(qs) if self.dev_rank else None
        keys = vals = None
        if p is not None and int(p.k_eff.reshape(-1)[0]) > 0:
            (bA, nA, _, _), (bB, nB, _, _) = self._slice_exact_plan()
            cA, cB = list(self.ops.clbits[ia]), list(self.ops.clbits[ib])
            # the column ranges are the low log2(n) bits of each side's index (aligned blocks)
            keys, vals = be.knit_select(p.A2[:, bA:bA + nA], p.B2[:, bB:bB + nB], cA[:nA.bit_length() - 1],
                                        cB[:nB.bit_length() - 1], self.N, accuracy, k_dev=p.k_eff)
            keys = keys + o_begin
            self.last_kernel = "qk_knit_select_kernel"
        else:
            keep = self.out
            self.out = be.zeros((o_count,), T.float64)
            try:
                if p is not None:
                    self._launch_step(p)  # the write is skipped (k = 0), the exact slice runs
                else:
                    ia_, ib_ = self.order[0], self.order[-1]
                    mats = self.operands(qs)
                    self._slice_exact(mats[ia_], mats[ib_], self.ops.clbits[ia_], self.ops.clbits[ib_])
                keys, vals = be.select_above(self.out, accuracy, key_base=o_begin)
            finally:
                self.out = keep
            self.last_kernel = None
        if p is not None:
            self.sync_stats()
        # all-gather the ranks' kept pairs (counts first, then padded buffers)
        n = T.tensor([keys.numel()], dtype=T.int64, device=keys.device)
        counts = T.empty(self.world, dtype=T.int64, device=keys.device)
        dist.all_gather_into_tensor(counts, n, group=self.group)
        cnt = counts.cpu().tolist()
        top = max(max(cnt), 1)
        kp = T.zeros(top, dtype=T.int64, device=keys.device)
        vp = T.zeros(top, dtype=T.float64, device=keys.device)
        kp[:keys.numel()] = keys
        vp[:vals.numel()] = vals
        kall = T.empty(self.world * top, dtype=T.int64, device=keys.device)
        vall = T.empty(self.world * top, dtype=T.float64, device=keys.device)
        dist.all_gather_into_tensor(kall, kp, group=self.group)
        dist.all_gather_into_tensor(vall, vp, group=self.group)
        sel = [slice(r * top, r * top + c) for r, c in enumerate(cnt) if c]
        if not sel:
            return np.zeros(0, dtype=np.int64), np.zeros(0)
        ku = T.cat([kall[s] for s in sel]) if len(sel) > 1 else kall[sel[0]]
        vu = T.cat([vall[s] for s in sel]) if len(sel) > 1 else vall[sel[0]]
        return be.npd_pairs(ku, vu)

    def step(self):
        self.be.bind()  # the caller may have switched torch's current stream since the last step
        if self.overlap and self.overlap_ok():
            return self._step_overlapped()
        if not self.record_events:
            return self.knit(self.sweep())
        start, end = self.be.event(), self.be.event()
        start.record()
        qs = self.sweep()
        end.record()
        self.sweep_events.append((start, end))
        n = len(self.events)
        out = self.knit(qs)
        if len(self.events) > n:  # operand transforms + data-rank step: sweep end -> knit start
            self.prep_events.append((end, self.events[n][0]))
        return out

    # ------------------------------------------------------------------ accounting
    def row_transform(self, i: int):
        """Host transform ``[terms, swept rows]`` of fragment i's operand ``X = W q`` over the rows the
        sweep writes (``ops.transforms[i]`` restricted / repeated by ``row_src``), or None."""
        W = self.ops.transforms[i]
        if W is None or self.row_src[i] is None:
            return W
        return np.ascontiguousarray(np.asarray(W)[:, self.row_src[i]])

    def instance_counts(self) -> dict:
        """Reference instance count (``run.py:37-39``: sum of per-fragment label lists) and jobs."""
        return {
            "instances_ref": int(sum(len(fs.labels) for fs in self.frags)),
            "instances_unique": int(sum(len(fs.unique_labels) for fs in self.frags)),
            # instance labels the sweep simulates (pruned rows left out), and the rows it writes (split)
            "instances_swept": int(sum((fs.n_rows if src is None else np.unique(src).size)
                                       for fs, src in zip(self.frags, self.row_src))),
            "rows_swept": int(sum(self.n_rows)),
            "branch_jobs": int(sum(self.plan_jobs)),  # swept (pruned rows left out), all ranks
            "branch_jobs_all_rows": int(sum(fs.jobs.n_jobs for fs in self.frags if not fs.dropped)),
            "labels": int(self.ops.num_terms),
            "labels_ref": int(np.prod([v.operation.num_instantiations for v in self.virt.vgate_instructions])),
            "terms_factored": int(self.ops.factored_terms or self.ops.num_terms),
        }

    def sweep_traffic(self) -> dict:
        """Modelled bytes of one step's sweep on this rank.

        ``hbm``: what the kernels move: SPLIT programs write the |0..0> tile in the INIT
        pass, read it back and write the whole state in the next pass, read + write the state
        in every middle pass, read it and write ``2^m`` fp64 in the FINAL pass; the label
        reduction reads the jobs' rows and writes the labels'. ``algorithmic``: SURVEY.md §8d,
        one read + write of the complex128 state per (fused) gate per job. ``flops``: fp64
        arithmetic the kernel executes (``_sweep_flops_per_job``)."""
        from . import sweep_plan

        hbm = alg = flops = 0
        shared = dict(zip(self._multi[0], self.be.shared_init or [])) if self._multi is not None else {}
        for i, (fs, sw) in enumerate(zip(self.frags, self.sweeps)):
            if sw is None or not sw["n_jobs"]:
                continue
            enc = fs.dprog.enc if getattr(fs, "dprog", None) is not None else sweep_plan.encode(fs.prog)
            J, n, m, P = sw["n_jobs"], enc.n, enc.m, len(enc.passes)
            S, tile, out = 16 << n, 16 << enc.tile_bits, 8 << m
            if enc.packed or P == 1:
                per_job = out
            elif P == 2:
                # shared INIT prefixes: the INIT tiles are written once per prefix, each job's FINAL
                # pass reads its prefix's tile (L2 / MALL re-reads counted as HBM here)
                per_job = tile + out + (tile * shared[i] // J if shared.get(i) else tile)
            else:
                per_job = 2 * tile + S + (P - 3) * 2 * S + S + out
            if sw.get("fused"):  # FINAL pass sums a label's jobs: one row per label, no reduction
                hbm += J * (per_job - out) + sw["n_local"] * out
            else:
                hbm += J * per_job
                if sw["q"] is not None:
                    hbm += J * out + sw["n_local"] * out
            alg += J * len(fs.prog.ops) * 32 * (1 << fs.prog.n)
            flops += J * _sweep_flops_per_job(enc)
        return {"hbm": hbm, "algorithmic": alg, "flops": flops}

    def gemm_shape(self) -> tuple[int, int, int]:
        """(M, N, K) of the main contraction on this rank."""
        K = self.term_range[1] - self.term_range[0] if self.last_rank is None else self.last_rank
        widths = [1 << len(c) for c in self.ops.clbits]
        M = 1
        for i in self.order[:-1]:
            M *= widths[i]
        if self.row_block is not None:
            M = self.row_block[1] - self.row_block[0]
        if self.slice is not None:  # this rank's outputs: 1/world of the rows
            M //= self.world
        return M, widths[self.order[-1]], K
