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
from .observables import MAX_CLBITS, KnitReducer, parse_masks, split_mask


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
