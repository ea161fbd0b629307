"""Parametric cut circuits: one plan and one compile for every parameter set.

A variational loop evaluates the same cut circuit at many angle sets. The constant route
(:class:`~.observables.KnitReducer`) folds every angle into the fragment programs, so a new angle
set is a new program. :class:`ParametricKnit` instead keeps the angles symbolic down to the sweep
kernels (``fragment_program``: ``"param"`` ops; ``qk_sweep_bound``: the per-binding matrix table),
does everything that depends on the circuit's structure once, and answers each binding — or a
batch of them, swept together — with a complete ``KnitReducer``.
"""
from __future__ import annotations

import hashlib
import threading
from collections import OrderedDict

import numpy as np

from . import engine
from .backend import MI355XBackend
from .knit_plan import LabelSpace
from .observables import MAX_CLBITS, KnitReducer, cotangent_scatter_host, parse_masks, split_mask


def binding_values(parameters: list, values, *, batch: bool) -> np.ndarray:
    """float64 ``[B, P]`` of what a caller passes as parameter values. One binding (``batch=False``):
    a sequence in ``parameters`` order or a mapping ``Parameter -> float``. A batch: an array-like
    ``[B, P]`` or a sequence of such single bindings. A missing or surplus value is a ``ValueError``."""
    P = len(parameters)

    def one(v) -> np.ndarray:
        if isinstance(v, dict):
            known = set(parameters)
            surplus = [getattr(p, "name", p) for p in v if p not in known]
            missing = [p.name for p in parameters if p not in v]
            if surplus or missing:
                raise ValueError(f"binding: no value for {missing}, values for unknown parameters {surplus}")
            return np.array([float(v[p]) for p in parameters], dtype=np.float64)
        row = np.asarray(v, dtype=np.float64).reshape(-1)
        if row.size != P:
            raise ValueError(f"{P} parameters but {row.size} values")
        return row

    if not batch:
        return one(values).reshape(1, P)
    if isinstance(values, np.ndarray) or (len(values) and not isinstance(values[0], dict)):
        arr = np.asarray(values, dtype=np.float64)
        if arr.ndim != 2 or arr.shape[1] != P:
            raise ValueError(f"bindings must be [B, {P}], not {arr.shape}")
        return np.ascontiguousarray(arr)
    return np.stack([one(v) for v in values]) if len(values) else np.zeros((0, P))


class ParametricKnit:
    """The plan of a parametric cut circuit: fragments compiled with their parameters symbolic
    (``prepare_fragments(parametric=True)``), their sweep kernels, and the knit operands, all made
    once by the constructor. It holds no swept rows: :meth:`bind` / :meth:`bind_many` sweep the
    fragments for one binding or a batch (``engine.sweep_fragment_bound``: no compile, one launch
    sequence per fragment) and return reducers that share everything else with this plan.
    ``factored`` and ``jit`` as for ``KnitReducer`` / ``engine.prepare_fragments``."""

    def __init__(self, virt, *, device: int = 0, factored: bool | None = None, jit: bool | None = None):
        if not all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f)):
            raise ValueError("ParametricKnit needs every fragment on the MI355X backend")
        if virt.circuit.num_clbits > MAX_CLBITS:
            raise ValueError(f"{virt.circuit.num_clbits} clbits: keys are int64, at most {MAX_CLBITS}")
        self.parameters = list(virt.parameters)
        self.device = device
        self.ctx = ctx = engine.get_context(device)
        factored = (factored is None or bool(factored)) and engine.factored_ok(virt)
        frags = engine.prepare_fragments(virt, device, basis=factored, jit=jit, parametric=True)
        ops = engine.knit_operands(virt, frags, factored)
        # the reducer every binding's reducer is a sibling of (KnitReducer.with_channels builds its the
        # same way): everything but the rows
        t = object.__new__(KnitReducer)
        t.N, t.device, t.ctx, t.factored, t.frags, t.ops = virt.circuit.num_clbits, device, ctx, factored, frags, ops
        t.clbits = [list(c) for c in ops.clbits]
        t.qs = None
        t._spectrum = t._transposed = t._moment_specs = t._spectrum_t = None
        if not frags:
            vg = [v.operation for v in virt.vgate_instructions]
            t._scalar = float(LabelSpace([g.num_instantiations for g in vg],
                                         [g.knit_coefficients() for g in vg]).coefficients().sum())
        self._template = t

    @property
    def num_parameters(self) -> int:
        return len(self.parameters)

    @property
    def frags(self) -> list:
        return self._template.frags

    # -- sweeps ---------------------------------------------------------------------------------
    def sweep(self, values: np.ndarray, workspace_budget: int | None = None) -> list:
        """Per fragment the device rows ``[B, rows_f, 2^m_f]`` of the bindings ``values [B, P]``."""
        self.ctx.bind_stream()
        return [engine.sweep_fragment_bound(self.ctx, fs, fs.prog.bind_matrices(values), workspace_budget)
                for fs in self.frags]

    def _reducer(self, qs: list) -> KnitReducer:
        new = object.__new__(KnitReducer)
        new.__dict__.update(self._template.__dict__)
        new.qs = qs
        return new

    def bind(self, values) -> KnitReducer:
        """The reducer of the circuit at one binding (a sequence in :attr:`parameters` order or a
        mapping ``Parameter -> float``): one bound sweep per fragment, no compile."""
        vals = binding_values(self.parameters, values, batch=False)
        return self._reducer([q[0] for q in self.sweep(vals)])

    def bind_many(self, values, *, workspace_budget: int | None = None) -> list:
        """One reducer per row of ``values [B, P]``, from one batched sweep per fragment; each holds a
        contiguous copy of its rows. ``workspace_budget``: bytes of sweep state per launch
        (``engine.BOUND_WORKSPACE_BYTES``); more bindings go in chunks, with the same rows."""
        vals = binding_values(self.parameters, values, batch=True)
        if not len(vals):
            return []
        qs = self.sweep(vals, workspace_budget)
        return [self._reducer([q[b].clone() for q in qs]) for b in range(len(vals))]

    def expectation(self, values, masks, weights=None) -> np.ndarray:
        """float64 ``[B, M]``: the Z-string expectation values ``masks`` (``observables.parse_masks``)
        of the exact knit at every binding of ``values [B, P]``; with ``weights [M]`` the weighted
        sums ``[B]``. The batch is swept once and ``qk_reduce_bits`` runs over all ``B * rows`` rows
        of a fragment at once per batch of masks; the transform and the product over fragments are
        taken per binding."""
        vals = binding_values(self.parameters, values, batch=True)
        return self.expectation_of_rows(self.sweep(vals) if len(vals) else [], len(vals), masks, weights)

    def expectation_of_rows(self, qs: list, B: int, masks, weights=None) -> np.ndarray:
        """:meth:`expectation` of rows already swept (:meth:`sweep` of ``B`` bindings)."""
        t = self._template
        self.ctx.bind_stream()
        zs = parse_masks(masks, t.N)
        M = len(zs)
        w = None
        if weights is not None:
            w = np.asarray(weights.cpu() if hasattr(weights, "cpu") else weights, dtype=np.float64)
            if w.ndim != 1 or len(w) != M:
                raise ValueError(f"{M} masks but weights of shape {w.shape}")
        out = np.zeros((B, M))
        if B and M and not t.frags:
            out[:] = t._scalar
        elif B and M:
            local = [list(col) for col in zip(*(split_mask(z, t.clbits) for z in zs))]  # per fragment, per mask
            reds = []
            for q, fcl, fl in zip(qs, t.clbits, local):
                rows, width = q.shape[1], q.shape[2]
                reds.append(engine.reduce_bits(self.ctx, q.view(B * rows, width), len(fcl), 0, fl).view(B, rows, M))
            for b in range(B):
                mats = engine.fragment_operands(self.ctx, t.ops, [r[b] for r in reds])  # [terms, M] each
                prod = mats[0]
                for a in mats[1:]:
                    prod = prod * a
                out[b] = prod.sum(0).cpu().numpy()
        return out if w is None else out @ w

    # -- gradients ------------------------------------------------------------------------------
    def _weights(self, weights, M: int):
        if weights is None:
            return None
        w = np.asarray(weights.cpu() if hasattr(weights, "cpu") else weights, dtype=np.float64)
        if w.ndim != 1 or len(w) != M:
            raise ValueError(f"{M} masks but weights of shape {w.shape}")
        return w

    def _columns(self, parameters) -> list:
        """Columns of ``self.parameters`` for ``parameters`` (None: all, in order); an unknown parameter or one
        named twice is a ``ValueError``."""
        if parameters is None:
            return list(range(len(self.parameters)))
        index = {p: i for i, p in enumerate(self.parameters)}
        unknown = [getattr(p, "name", p) for p in parameters if p not in index]
        if unknown or len(set(parameters)) != len(parameters):
            raise ValueError(f"parameters: unknown {unknown}" if unknown else "parameters: one parameter named twice")
        return [index[p] for p in parameters]

    def _transform(self, i: int) -> np.ndarray:
        """``W_f`` ``[swept rows, terms]`` of fragment ``i``: ``X_f = W_f^T red_f`` (``engine.plan_transforms``)."""
        ops, fs = self._template.ops, self.frags[i]
        if ops.transforms[i] is not None:
            return np.ascontiguousarray(ops.transforms[i].T)
        W = np.zeros((fs.n_rows, ops.num_terms))
        np.add.at(W, (ops.rows[i], np.arange(ops.num_terms)), ops.coefs[i])
        return W

    def _base(self, qs: list, B: int, zs: list):
        """From the swept rows of ``B`` bindings: per fragment the local masks and ``X_f [B, terms, M]`` on the
        device (``engine.fragment_operands`` per binding, as :meth:`expectation_of_rows` takes them), and the
        unweighted values ``[B, M]`` in that method's own order of operations."""
        T = engine.torch()
        t = self._template
        M = len(zs)
        local = [list(col) for col in zip(*(split_mask(z, t.clbits) for z in zs))]
        reds = []
        for q, fcl, fl in zip(qs, t.clbits, local):
            rows, width = q.shape[1], q.shape[2]
            reds.append(engine.reduce_bits(self.ctx, q.reshape(B * rows, width), len(fcl), 0, fl).view(B, rows, M))
        per_b = [engine.fragment_operands(self.ctx, t.ops, [r[b] for r in reds]) for b in range(B)]
        X = [T.stack([per_b[b][f] for b in range(B)]) for f in range(len(qs))]
        out = np.zeros((B, M))
        for b in range(B):
            prod = per_b[b][0]
            for a in per_b[b][1:]:
                prod = prod * a
            out[b] = prod.sum(0).cpu().numpy()
        return local, X, out

    @staticmethod
    def _others(X: list, f: int):
        """``prod over f' != f of X_f'`` in fragment order (all ones for a single fragment)."""
        prod = None
        for g, x in enumerate(X):
            if g != f:
                prod = x if prod is None else prod * x
        return X[f] * 0.0 + 1.0 if prod is None else prod

    def _cotangent(self, f: int, q_shape: tuple, Xh: list, local_f: list, w: np.ndarray):
        """``D_f [B, rows_f, 2^m_f]`` on the device from the host copies ``Xh`` of every ``X_f'``: ``C_f = W_f (prod of
        the others * w)`` on the host (numpy, one fixed order), masks that coincide on this fragment combined by a
        0/1 matrix, the result scattered to the distinct masks' columns and transformed by one ``qk_wht_rows``."""
        T = engine.torch()
        B, rows, width = q_shape
        C = np.matmul(self._transform(f)[None], self._others(Xh, f) * w[None, None, :])  # [B, rows, M]
        uniq, Cu = cotangent_scatter_host(C, local_f)
        dev = T.device("cuda", self.device)
        Cu = T.from_numpy(np.ascontiguousarray(Cu).reshape(B * rows, len(uniq))).to(dev)
        D = T.zeros((B * rows, width), dtype=T.float64, device=dev)
        D[:, T.tensor(uniq, dtype=T.int64, device=dev)] = Cu  # distinct columns: no accumulation
        engine.wht_rows(self.ctx, D, out=D)
        return D.view(B, rows, width)

    def cotangent_rows(self, qs_b: list, masks, weights) -> list:
        """Per fragment the device tensor ``D_f [rows_f, 2^m_f]`` with ``<D_f, q_f> = E_w``: the cotangent of the
        weighted sum ``E_w = sum_m weights[m] <Z_masks[m]>`` with respect to fragment ``f``'s swept rows, at the one
        binding whose rows ``qs_b`` (:meth:`sweep`, one binding) are. ``E_w`` is linear in each fragment's rows, so
        ``D_f`` does not depend on ``q_f`` itself."""
        self.ctx.bind_stream()
        zs = parse_masks(masks, self._template.N)
        w = self._weights(weights, len(zs))
        if w is None:
            raise ValueError("cotangent_rows needs weights (one-hot weights give a single mask's)")
        if not self.frags or not zs:
            return [engine.torch().zeros_like(q) for q in qs_b]
        qs = [q.unsqueeze(0) for q in qs_b]
        local, X, _ = self._base(qs, 1, zs)
        Xh = [x.cpu().numpy() for x in X]
        return [self._cotangent(f, tuple(q.shape), Xh, local[f], w)[0] for f, q in enumerate(qs)]

    @staticmethod
    def shift_chunks(B: int, n_occ: int, unit_bytes: int, budget: int) -> list:
        """``[(b0, b1, o0, o1), ...]``: (bindings x occurrences) blocks whose ``2 * (b1 - b0) * (o1 - o0)`` shifted
        units of ``unit_bytes`` each stay within ``budget`` (at least one pair per block): whole bindings while
        one fits, else slices of one binding's occurrences."""
        pairs = max(1, int(budget) // max(2 * int(unit_bytes), 1))
        if pairs >= n_occ:
            nb = pairs // n_occ
            return [(b, min(b + nb, B), 0, n_occ) for b in range(0, B, nb)]
        return [(b, b + 1, o, min(o + pairs, n_occ)) for b in range(B) for o in range(0, n_occ, pairs)]

    def value_and_gradient(self, values, masks, weights=None, *, parameters=None, row_budget: int | None = None) -> tuple:
        """The Z-string expectation values of :meth:`expectation` and their exact parameter-shift gradient.

        With ``weights [M]``: ``(E_w [B], grad [B, P'])`` of the weighted sum, by the cotangent route: one batched
        base sweep gives the value and, per fragment, the cotangent ``D_f`` of ``E_w`` with respect to its rows;
        each angle occurrence of a fragment is then swept at ``+-pi/2`` (that fragment alone, as ordinary bindings
        of the bound sweep with one matrix of the table changed) and ``qk_rows_dot`` takes ``<D_f, Q>`` of the
        shifted rows: ``d E_w / d angle = (dot+ - dot-) / 2``, whatever ``M`` is. Without ``weights``:
        ``(E [B, M], grad [B, M, P'])`` per mask, by the reduce route (``qk_reduce_bits`` on the shifted rows,
        knitted against the other fragments' base operands). ``grad[..., j]`` is the derivative with respect to
        ``parameters[j]`` (a list of this circuit's ``Parameter``; default all, in :attr:`parameters` order): the
        sum over the occurrences of ``coefficient * occurrence derivative``, in program order on the host, so a
        parameter that occurs several times or inside an affine expression is differentiated correctly.
        ``row_budget``: bytes of shifted rows held at a time (``engine.GRADIENT_ROW_BYTES``); more go in chunks,
        with the same bits on the cotangent route."""
        T = engine.torch()
        t = self._template
        vals = binding_values(self.parameters, values, batch=True)
        zs = parse_masks(masks, t.N)
        B, M = len(vals), len(zs)
        w = self._weights(weights, M)
        cols = self._columns(parameters)
        where = {c: j for j, c in enumerate(cols)}
        budget = engine.GRADIENT_ROW_BYTES if row_budget is None else int(row_budget)
        if budget < 1:
            raise ValueError("row_budget must be positive")
        grad = np.zeros((B, len(cols)) if w is not None else (B, M, len(cols)))
        if not B or not M or not t.frags:
            E = np.zeros((B, M))
            if B and M:
                E[:] = t._scalar
            return (E if w is None else E @ w), grad
        self.ctx.bind_stream()
        qs = self.sweep(vals)
        local, X, E = self._base(qs, B, zs)
        Xh = [x.cpu().numpy() for x in X] if w is not None else None
        for f, fs in enumerate(self.frags):
            if fs.dropped or not fs.prog.num_params:
                continue
            occs = [o for o in fs.prog.shift_occurrences() if any(c in where for c in o.coefs)]
            if not occs:
                continue
            _, rows, width = qs[f].shape
            n = rows * width
            if w is not None:
                D = self._cotangent(f, (B, rows, width), Xh, local[f], w).view(B, n)
                d_occ = np.zeros((B, len(occs)))
            else:
                Wt = T.from_numpy(np.ascontiguousarray(self._transform(f).T)).to(qs[f].device)  # [terms, rows]
                Y = self._others(X, f)  # [B, terms, M]
                d_occ = np.zeros((B, len(occs), M))
            for b0, b1, o0, o1 in self.shift_chunks(B, len(occs), n * 8, budget):
                nb, no = b1 - b0, o1 - o0
                mats = fs.prog.bind_matrices_shifted(vals[b0:b1], occs[o0:o1])
                Q = engine.sweep_fragment_bound(self.ctx, fs, mats.reshape(nb * no * 2, fs.prog.num_params, 2, 2))
                if w is not None:
                    dots = engine.rows_dot(self.ctx, Q.view(nb * no * 2, n), D[b0:b1], per=2 * no)
                    dots = dots.cpu().numpy().reshape(nb, no, 2)
                else:
                    red = engine.reduce_bits(self.ctx, Q.view(nb * no * 2 * rows, width), len(t.clbits[f]), 0, local[f])
                    Xs = T.matmul(Wt, red.view(nb, no * 2, rows, M))  # [nb, 2 no, terms, M]
                    dots = (Xs * Y[b0:b1, None]).sum(2).cpu().numpy().reshape(nb, no, 2, M)
                del Q
                d_occ[b0:b1, o0:o1] = 0.5 * (dots[:, :, 0] - dots[:, :, 1])
            for o, occ in enumerate(occs):  # host, in occurrence order
                for c, coef in occ.coefs.items():
                    if c in where:
                        grad[..., where[c]] += coef * d_occ[:, o]
        return (E if w is None else E @ w), grad

    def gradient(self, values, masks, weights=None, **kw) -> np.ndarray:
        """The gradient of :meth:`value_and_gradient` alone."""
        return self.value_and_gradient(values, masks, weights, **kw)[1]


# ---------------------------------------------------------------------------- cached plans
KNIT_CACHE_SIZE = 4  # ParametricKnit objects kept (LRU), per (structural fingerprint, device, thread)
_KNITS: OrderedDict = OrderedDict()
_KNITS_LOCK = threading.Lock()
knits_built = [0]  # ParametricKnit objects cached_knit has built (tests count it)


def structural_fingerprint(virt) -> str:
    """``run.circuit_fingerprint`` with every parameter expression in place of its value: each
    parameter enters as its position in ``virt.parameters``, so two circuits built alike from
    different ``Parameter`` objects share the hash, whatever values they are later bound to."""
    from .run import _param_key

    index = {p: i for i, p in enumerate(virt.parameters)}

    def key(p):
        return p.structure(index) if hasattr(p, "structure") else _param_key(p)

    h = hashlib.sha1()
    circ = virt.circuit
    h.update(repr((circ.num_qubits, circ.num_clbits, len(virt.vgate_instructions), len(index))).encode())
    for frag, fcirc in virt.fragment_circuits.items():
        h.update(repr(("frag", frag.name, len(frag))).encode())
        for instr in fcirc:
            op = instr.operation
            item = [op.name, tuple(key(p) for p in getattr(op, "params", ())),
                    tuple(fcirc.find_qubit(q) for q in instr.qubits), tuple(fcirc.find_clbit(c) for c in instr.clbits)]
            vg = getattr(op, "_virtual_gate", None)
            if vg is not None:
                item += [op.vgate_idx, op.qubit_idx, type(vg).__name__,
                         tuple(_param_key(p) for p in getattr(vg, "_params", getattr(vg, "params", ())))]
            h.update(repr(item).encode())
    return h.hexdigest()


def cached_knit(virt, device: int = 0, factored: bool | None = None) -> ParametricKnit:
    """The :class:`ParametricKnit` of ``virt`` for the calling thread, built on the first call and
    reused for every circuit of the same structure (:func:`structural_fingerprint`)."""
    key = (structural_fingerprint(virt), device, factored, threading.get_ident())
    with _KNITS_LOCK:
        knit = _KNITS.get(key)
        if knit is not None:
            _KNITS.move_to_end(key)
            return knit
    knit = ParametricKnit(virt, device=device, factored=factored)
    knits_built[0] += 1
    with _KNITS_LOCK:
        _KNITS[key] = knit
        while len(_KNITS) > KNIT_CACHE_SIZE:
            _KNITS.popitem(last=False)
    return knit


def clear_knit_cache() -> None:
    with _KNITS_LOCK:
        _KNITS.clear()
