"""``run_virtual_circuit``: the knitting hot path, MI355X-native.

Drop-in for ``third_party/qvm/qvm/run.py:23-71``: same name, same arguments,
same return shape ``(dict[int, float], RunTimeInfo)``. Differences, by design:

* by default instances are simulated exactly (fp64 statevector, HIP) instead of
  being sampled with ``shots`` (``run.py:42``); ``sample=True`` draws ``shots``
  outcomes per instance label from the exact distributions on the GPU
  (``engine.sample_fragment``: counter-based stream, ``seed``) and applies
  ``from_counts``' truncation, as the reference's Aer path does; fragments whose
  backend was replaced by a foreign (e.g. qiskit-aer) backend are run through the
  reference's own counts path;
* the knit is one dense fp64 MFMA contraction; ``QuasiDistr``'s ``ACCURACY``
  truncation is applied once to the final distribution instead of after every
  intermediate dict operation, then ``nearest_probability_distribution``
  (``quasi_distr.py:28-43``) as the reference does at ``run.py:71``;
* ``dense=True`` returns the full distribution as a device tensor (needed for
  32-bit outputs: 2^32 fp64 = 34.4 GB cannot be a Python dict).

Timing split (``RunTimeInfo``) follows ``run.py:35,60,65-67``: ``run_time``
covers instance preparation + simulation, ``knit_time`` the contraction.
"""
from __future__ import annotations

import hashlib
import logging
import threading
from collections import OrderedDict
from dataclasses import dataclass
from time import perf_counter

import numpy as np

from . import engine
from . import quasi_distr as _qd
from .backend import MI355XBackend
from .quasi_distr import QuasiDistr
from .virtual_circuit import VirtualCircuit, generate_instantiations

log = logging.getLogger(__name__)


@dataclass
class RunTimeInfo:
    run_time: float
    knit_time: float
    # multi-GPU runs: (first output, outputs) of this rank's contiguous share of the distribution
    shard: tuple | None = None


def _sync(device: int) -> None:
    engine.torch().cuda.synchronize(device)


def _foreign_fragment(virt: VirtualCircuit, fs: engine.FragmentState, backend, shots: int, device: int):
    """Reference counts path for a fragment bound to a non-MI355X backend (run.py:36-58)."""
    T = engine.torch()
    N = virt.circuit.num_clbits
    circuits = generate_instantiations(virt.fragment_circuits[fs.fragment], fs.labels)
    counts = backend.run(circuits, shots=shots).result().get_counts()
    counts = [counts] if isinstance(counts, dict) else counts
    pos = {c: i for i, c in enumerate(fs.prog.clbits)}
    q = np.zeros((len(fs.labels), 1 << len(pos)), dtype=np.float64)
    for li, c in enumerate(counts):
        for key, val in QuasiDistr.from_counts(c).items():
            data, cfg = key & ((1 << N) - 1), key >> N
            x = 0
            while data:
                low = data & -data
                x |= 1 << pos[low.bit_length() - 1]
                data ^= low
            q[li, x] += (-1.0) ** bin(cfg).count("1") * val
    return T.from_numpy(q).to(T.device("cuda", device))


def _direct_dense(virt: VirtualCircuit, shots: int, device: int, factored: bool, out, sample: bool, seed: int):
    """Sweep (or shot-sample) + knit without a cached plan: sampled runs, foreign backends and the
    explicit ``factored=True/False`` knits of ``engine.knit_dense``."""
    ctx = engine.get_context(device)
    # The factored knit folds labels whose side programs coincide into one operand row; sampled
    # labels differ in their shots even then, so sampling knits directly over the labels.
    factored = factored and not sample and engine.factored_ok(virt)
    now = perf_counter()
    native = all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f))
    frags = engine.prepare_fragments(virt, device, basis=factored and native and not sample)
    qs = []
    for i, fs in enumerate(frags):
        backend = virt.get_backend(fs.fragment)
        if isinstance(backend, MI355XBackend) and not sample:
            qs.append(engine.sweep_fragment(ctx, fs))
            continue
        if isinstance(backend, MI355XBackend):
            qs.append(engine.sample_fragment(ctx, fs, shots, engine.fragment_seed(seed, i), _qd.ACCURACY))
        else:
            qs.append(_foreign_fragment(virt, fs, backend, shots, device))
        frags[i] = engine.label_rows(fs)  # one q row per reference label
    _sync(device)
    run_time = perf_counter() - now
    now = perf_counter()
    dense = engine.knit_dense(ctx, virt, frags, qs, out=out, factored=factored)
    _sync(device)
    knit_time = perf_counter() - now
    return dense, RunTimeInfo(run_time, knit_time)


# ---------------------------------------------------------------------------- plan cache
PLAN_CACHE_SIZE = 4  # compiled plans kept (LRU), per (circuit fingerprint, device, thread)
PLAN_CACHE_MAX_BYTES = 16 << 30  # plans holding more device memory (a 32-qubit uncut sweep: 100 GB) are not kept
PLAN_CACHE_TOTAL_BYTES = 32 << 30  # device bytes all cached plans may hold together (LRU eviction beyond)
_PLANS: OrderedDict = OrderedDict()
_PLANS_LOCK = threading.Lock()


def _param_key(p):
    """A parameter as hashed by circuit_fingerprint: arrays by dtype, shape and bytes (their repr
    rounds to 8 digits and elides long arrays), everything else by repr."""
    if isinstance(p, np.ndarray):
        return ("nd", p.dtype.str, p.shape, hashlib.sha1(np.ascontiguousarray(p).tobytes()).hexdigest())
    return repr(p)


def circuit_fingerprint(virt: VirtualCircuit) -> str:
    """Content hash of a cut circuit as the sweep and knit see it: every fragment circuit's
    operations (name, parameters, qubit and global clbit positions; for virtual-gate endpoints the
    gate type, its parameters and the endpoint side) and the output width. Two ``VirtualCircuit``
    objects built from the same cut share it, so a repeated ``run_virtual_circuit`` reuses the
    compiled plan. Cached on the ``VirtualCircuit`` per mutation generation (``_generation``) only:
    the caller's circuit can be edited in place between calls (``cut.data[i] = ...`` keeps the list
    and its length), so every new ``VirtualCircuit`` hashes its fragments again — when it is built
    (``VirtualCircuit.__init__``; syc 32 5: ~1.3 ms of the ~6 ms construction in the build container),
    as the reference builds one per call (``Utilities.py:74-79``)."""
    gen = getattr(virt, "_generation", 0)
    cached = getattr(virt, "_qk_fingerprint", None)
    if cached is not None and cached[0] == gen:
        return cached[1]
    h = hashlib.sha1()
    circ = virt.circuit
    h.update(repr((circ.num_qubits, circ.num_clbits, len(virt.vgate_instructions))).encode())
    for frag, fcirc in virt.fragment_circuits.items():
        h.update(repr(("frag", frag.name, len(frag))).encode())
        for instr in fcirc:
            op = instr.operation
            item = [op.name, tuple(_param_key(p) for p in getattr(op, "params", ())),
                    tuple(fcirc.find_qubit(q) for q in instr.qubits), tuple(fcirc.find_clbit(c) for c in instr.clbits)]
            vg = getattr(op, "_virtual_gate", None)
            if vg is not None:
                item += [op.vgate_idx, op.qubit_idx, type(vg).__name__,
                         tuple(_param_key(p) for p in getattr(vg, "_params", getattr(vg, "params", ())))]
            h.update(repr(item).encode())
    fp = h.hexdigest()
    virt._qk_fingerprint = (gen, fp)
    return fp


def _build_plan(virt: VirtualCircuit, device: int):
    """The benchmarked engine (bench.py): factored knit with light-cone basis + rank-compressed core
    and the per-step device data rank (``pipeline.KnitPipeline``). A circuit the
    factored planner refuses (a virtual gate with both endpoints in one fragment) gets the direct
    knit over all global labels through the same pipeline (``engine.factored_ok``)."""
    from .pipeline import KnitPipeline

    if not engine.factored_ok(virt):
        log.info("a virtual gate with both endpoints in one fragment: direct knit")
        return KnitPipeline(virt, device=device, factored=False)
    return KnitPipeline(virt, device=device, factored=True)


def cached_plan(virt: VirtualCircuit, device: int = 0, group=None, backend=None):
    """The compiled plan (``KnitPipeline``) of ``virt`` on ``device`` for the calling thread: built on
    the first call, reused while the circuit's fingerprint is unchanged (LRU of PLAN_CACHE_SIZE;
    plans above PLAN_CACHE_MAX_BYTES of device buffers are rebuilt per call instead).
    Plans are per thread: a plan owns its sweep buffers, and the reference calls
    ``run_virtual_circuit`` from concurrent threads (``Utilities.py:85-89``). ``group`` (a
    ``torch.distributed`` process group, or ``"WORLD"``): this rank's plan of the multi-GPU run
    (:func:`_build_sharded_plan`), keyed by the group as well. ``backend``: a pipeline backend other
    than the HIP one (CPU tests), part of the key."""
    key = (circuit_fingerprint(virt), device, threading.get_ident())
    if group is not None:
        import torch.distributed as dist

        g = None if group == "WORLD" else group
        gid = "WORLD" if g is None else (getattr(g, "group_name", None) or id(g))
        key += ("sharded", gid, dist.get_rank(g), dist.get_world_size(g))
    if backend is not None:
        key += ("backend", id(backend))
    with _PLANS_LOCK:
        pipe = _PLANS.get(key)
        if pipe is not None:
            _PLANS.move_to_end(key)
            pipe.plan_reused = True
            return pipe
    if group is None:
        pipe = _build_plan(virt, device)
    else:
        pipe = _build_sharded_plan(virt, device, None if group == "WORLD" else group, backend)
    pipe.plan_reused = False
    if pipe.plan_bytes() > PLAN_CACHE_MAX_BYTES:
        return pipe
    with _PLANS_LOCK:
        _PLANS[key] = pipe
        _PLANS.move_to_end(key)
        while len(_PLANS) > 1 and (len(_PLANS) > PLAN_CACHE_SIZE
                                   or sum(_plan_held_bytes(p) for p in _PLANS.values()) > PLAN_CACHE_TOTAL_BYTES):
            _PLANS.popitem(last=False)
    return pipe


def _plan_held_bytes(pipe) -> int:
    """Device bytes a cached plan holds: its buffers, the output mapping it keeps for reuse (the mapped
    bytes: whole 1-GiB chunks) and the output buffers of pipelined steps, if any."""
    total = pipe.plan_bytes()
    own = pipe._call_owner
    if own is not None:
        total += own.mapped_bytes() if hasattr(own, "mapped_bytes") else 8 * own.n
    for t in pipe._outs or []:
        total += t.numel() * t.element_size()
    return total


def clear_plan_cache() -> None:
    """Drop every cached plan (and the output mappings they keep): the device memory returns once
    no result tensor of theirs is alive."""
    with _PLANS_LOCK:
        _PLANS.clear()


def _is_oom(e: Exception) -> bool:
    T = engine.torch()
    msg = str(e)
    return (isinstance(e, T.cuda.OutOfMemoryError) or "out of memory" in msg.lower()
            or "hipErrorOutOfMemory" in msg)


def _planned_dense(virt: VirtualCircuit, device: int, out):
    """One step of the cached plan into a fresh (or the caller's) output buffer. ``run_time`` = host
    planning (first call) + the sweep (HIP events), ``knit_time`` = the rest of the wall time: the
    same split as run.py:35,60,65-67 without a host synchronisation between the two."""
    T = engine.torch()
    now = perf_counter()
    pipe = cached_plan(virt, device)
    t_plan = perf_counter()
    pipe.be.bind()
    if out is None:  # 1-GiB-mapped when large; the previous call's mapping once the caller dropped it
        out = pipe.take_out(defer_select=True)
    t_out = perf_counter()
    e0, e1 = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
    host = perf_counter() - now
    timed = pipe._time_call_write and not pipe.record_events
    n_ev = len(pipe.events)
    e0.record()
    pipe.out = out
    try:
        if timed:  # the call's own write times its un-checked output mapping (KnitPipeline.take_out)
            pipe.record_events = True
        qs = pipe.sweep()
        e1.record()
        t_sweep = perf_counter()
        pipe.knit(qs)
        t_knit = perf_counter()
        out = pipe.out
    finally:
        pipe.out = None
        if timed:
            pipe.record_events = False
    _sync(device)
    wall = perf_counter() - now
    if timed:
        pipe.note_call_write(n_ev)
        del pipe.events[n_ev:]
    if not pipe.plan_reused and not hasattr(pipe, "first_call_ms"):
        # where the first call's time goes: the plan's phases (KnitPipeline.plan_ms), the output buffer
        # (mapping + write-rate selection), the step itself (launches + device time to the sync)
        pipe.first_call_ms = {"plan": (t_plan - now) * 1e3, **{f"plan.{k}": v for k, v in pipe.plan_ms.items()},
                              "output_buffer": (t_out - t_plan) * 1e3, "step": (now + wall - t_out) * 1e3,
                              "step.sweep_launch": (t_sweep - t_out) * 1e3, "step.knit_launch": (t_knit - t_sweep) * 1e3,
                              "step.device_wait": (now + wall - t_knit) * 1e3, "total": wall * 1e3}
    pipe.sync_stats()
    run_time = host + e0.elapsed_time(e1) * 1e-3
    return out, RunTimeInfo(run_time, max(wall - run_time, 0.0)), pipe


def _planned_dict(virt: VirtualCircuit, device: int, accuracy: float):
    """The reference-shaped result from the cached plan (``KnitPipeline.knit_dict``): the
    thresholded knit where it applies, never the dense 2^N vector."""
    T = engine.torch()
    now = perf_counter()
    pipe = cached_plan(virt, device)
    pipe.be.bind()
    e0, e1 = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
    host = perf_counter() - now
    e0.record()
    qs = pipe.sweep()
    e1.record()
    keys, vals = pipe.knit_dict(accuracy, qs)
    wall = perf_counter() - now
    pipe.sync_stats()
    run_time = host + e0.elapsed_time(e1) * 1e-3
    return keys, vals, RunTimeInfo(run_time, max(wall - run_time, 0.0))


def run_virtual_circuit_dense(virt: VirtualCircuit, shots: int = 20000, *, device: int = 0,
                              factored: bool | None = None, out=None, sample: bool = False, seed: int = 0):
    """Sweep (or shot-sample, ``sample=True``) + knit; returns ``(dense fp64 tensor [2^N] on
    device, RunTimeInfo)``.

    Default (``factored=None``, every fragment on the MI355X backend, exact instances): the cached
    plan (:func:`cached_plan`) — the engine ``bench.py`` times: factored light-cone knit, per-step
    device data rank, the write-bound blocked knit. ``factored=True/False`` force the uncached
    factored / direct ``engine.knit_dense``; sampling and foreign backends take the direct path."""
    log.info("Running virtualizer with %d %s fragments and %d vgates...",
             len(virt.fragment_circuits),
             tuple(len(f) for f in virt.fragment_circuits), len(virt.vgate_instructions))
    native = all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f))
    if factored is None and native and not sample:
        try:
            dense, info, _ = _planned_dense(virt, device, out)
        except Exception as e:  # out of device memory: drop the cached plans (and their outputs), retry once
            if not _is_oom(e):
                raise
            log.warning("out of device memory (%s): clearing the plan cache and retrying", e)
            clear_plan_cache()
            engine.torch().cuda.empty_cache()
            dense, info, _ = _planned_dense(virt, device, out)
    else:
        dense, info = _direct_dense(virt, shots, device, bool(factored), out, sample, seed)
    log.info("Knitted in %.2fs.", info.knit_time)
    return dense, info


def run_virtual_circuit_sharded(virt: VirtualCircuit, group=None, *, device: int | None = None, backend=None):
    """Multi-GPU ``run_virtual_circuit`` (one process per GPU, ``torch.distributed`` initialised;
    ``group``: the process group, None = WORLD). The instance sweep is sharded over the ranks and
    the distribution assembled by the pipeline's collectives:

    * wide outputs (syc 32: 2^32 fp64 = 34 GB) in ``slice`` mode: rank r returns the contiguous
      outputs ``[r, r + 1) * 2^N / world`` of the reference-ordered distribution (concatenating the
      ranks' shards in rank order gives the whole array);
    * narrow outputs (bv / hwe / qft: at most the instance tensors' size) in ``reduce`` mode: one
      RCCL reduce; rank 0 holds the whole distribution, the others ``None``.

    Returns ``(tensor or None, RunTimeInfo)`` with ``info.shard = (first output, outputs)`` of the
    returned tensor. Exact instances only (the reference's ``shots`` sampling: single-GPU
    ``run_virtual_circuit(sample=True)``)."""
    import torch.distributed as dist

    T = engine.torch()
    rank = dist.get_rank(group)
    if device is None:
        device = T.cuda.current_device() if backend is None else 0
    log.info("Running virtualizer with %d %s fragments and %d vgates on %d ranks...",
             len(virt.fragment_circuits), tuple(len(f) for f in virt.fragment_circuits),
             len(virt.vgate_instructions), dist.get_world_size(group))
    on_gpu = backend is None
    now = perf_counter()
    pipe = cached_plan(virt, device, group="WORLD" if group is None else group, backend=backend)
    pipe.be.bind()
    # slice mode: the previous call's output mapping again once the caller dropped it (take_out);
    # reduce mode: a fresh (small) buffer per call, as the reference returns a new result per call
    pipe.out = pipe.take_out() if pipe.mode == "slice" else None
    try:
        qs = pipe.sweep()
        if on_gpu:
            _sync(device)
        run_time = perf_counter() - now
        now = perf_counter()
        out = pipe.knit(qs)
        if on_gpu:
            _sync(device)
    finally:
        pipe.out = None
    pipe.sync_stats()
    knit_time = perf_counter() - now
    log.info("Knitted in %.2fs.", knit_time)
    if pipe.mode == "slice":
        return out, RunTimeInfo(run_time, knit_time, tuple(pipe.slice))
    n = 1 << pipe.N
    return (out if rank == 0 else None), RunTimeInfo(run_time, knit_time, (0, n) if rank == 0 else (0, 0))


def _build_sharded_plan(virt: VirtualCircuit, device: int, group, backend):
    """This rank's plan of a multi-GPU run: slice mode for a factored two-fragment knit
    whose fragments partition the output bits, else the direct knit in reduce mode (one RCCL reduce)."""
    import torch.distributed as dist

    from .pipeline import KnitPipeline

    world, rank = dist.get_world_size(group), dist.get_rank(group)
    kw = {"backend": backend} if backend is not None else {}
    if engine.factored_ok(virt):  # else (both endpoints of a gate in one fragment): direct knit, reduce mode
        pipe = KnitPipeline(virt, device=device, factored=True, rank=rank, world=world, group=group, **kw)
        if pipe.mode == "slice":
            return pipe
        del pipe
    return KnitPipeline(virt, device=device, factored=False, rank=rank, world=world, group=group, mode="reduce", **kw)


def _sharded_dict(virt: VirtualCircuit, group, device: int, accuracy: float):
    """The reference-shaped dict of a multi-GPU run, every rank the whole of it (``run.py:71``): slice
    mode selects the entries above ``accuracy`` per rank and runs the NPD of the gathered union
    (``KnitPipeline.knit_dict``, any output width); reduce mode's distribution (at most the instance
    tensors' size) is all-reduced and truncated as on one GPU."""
    T = engine.torch()
    now = perf_counter()
    pipe = cached_plan(virt, device, group="WORLD" if group is None else group)
    pipe.be.bind()
    if pipe.mode == "slice":
        e0, e1 = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        host = perf_counter() - now
        e0.record()
        qs = pipe.sweep()
        e1.record()
        keys, vals = pipe.knit_dict(accuracy, qs)
        wall = perf_counter() - now
        run_time = host + e0.elapsed_time(e1) * 1e-3
        return keys, vals, RunTimeInfo(run_time, max(wall - run_time, 0.0), tuple(pipe.slice))
    import torch.distributed as dist

    out, info = run_virtual_circuit_sharded(virt, group, device=device)
    full = T.zeros(1 << virt.circuit.num_clbits, dtype=T.float64, device=T.device("cuda", device))
    lo, cnt = info.shard
    if out is not None and cnt:
        full[lo:lo + cnt] = out[:cnt]
    dist.all_reduce(full, group=group)  # shards are disjoint: the sum assembles the distribution
    keys, vals = engine.nearest_probability_distribution(engine.get_context(device), full, accuracy)
    return keys, vals, info


def _run_reference_truncated(virt: VirtualCircuit, device: int, dense: bool):
    """``truncation="reference"``: the reference's knit with ``ACCURACY`` applied after every
    operation (truncated.knit_reference_truncated), then nearest_probability_distribution."""
    from .truncated import knit_reference_truncated

    if not all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f)):
        raise ValueError("truncation='reference' needs every fragment on the MI355X backend")
    log.info("Running virtualizer with %d %s fragments and %d vgates (reference truncation)...",
             len(virt.fragment_circuits), tuple(len(f) for f in virt.fragment_circuits), len(virt.vgate_instructions))
    now = perf_counter()
    out = knit_reference_truncated(virt, device, _qd.ACCURACY)
    _sync(device)
    info = RunTimeInfo(0.0, perf_counter() - now)
    log.info("Knitted in %.2fs.", info.knit_time)
    if dense:
        return out, info
    keys, vals = engine.nearest_probability_distribution(engine.get_context(device), out, _qd.ACCURACY)
    return dict(zip(keys.tolist(), vals.tolist())), info


def run_virtual_circuit(virt: VirtualCircuit, shots: int = 20000, *, device: int = 0,
                        dense: bool = False, factored: bool | None = None, sample: bool = False, seed: int = 0,
                        group=None, truncation: str = "final"):
    """Reference-compatible entry point (``run.py:23-71``). ``group`` (a ``torch.distributed``
    process group, e.g. ``dist.group.WORLD``) runs it on every rank of the group
    (:func:`run_virtual_circuit_sharded`, the plan cached per group like the single-GPU one):
    ``dense=True`` returns the rank's shard, otherwise every rank returns the whole reference-shaped
    dict (slice mode: the entries above ``ACCURACY`` selected per rank, gathered, then the NPD — any
    output width, syc 32 included).

    ``truncation``: ``"final"`` (default) knits exactly and applies ``ACCURACY`` once, to the result;
    ``"reference"`` applies it after every operation as the reference's ``QuasiDistr`` dicts do
    (``quasi_distr.py:7-10``: from_counts, every merge, every per-gate ``+ - *``), on exact instance
    distributions, single GPU, at most 24 clbits (``dense=True``: the knit before NPD)."""
    if truncation not in ("final", "reference"):
        raise ValueError(f"truncation must be 'final' or 'reference', not {truncation!r}")
    if truncation == "reference":
        if group is not None or sample or factored is not None:
            raise ValueError("truncation='reference': single GPU, exact instances, the direct knit")
        if virt.circuit.num_clbits > 24:
            raise ValueError("truncation='reference' is for outputs of at most 24 clbits")
        return _run_reference_truncated(virt, device, dense)
    if group is not None:
        if sample:
            raise ValueError("multi-GPU runs sweep exact instances (sample=True: single GPU)")
        if dense:
            return run_virtual_circuit_sharded(virt, group, device=device)
        keys, vals, info = _sharded_dict(virt, group, device, _qd.ACCURACY)
        log.info("Knitted in %.2fs.", info.knit_time)
        return dict(zip(keys.tolist(), vals.tolist())), info
    else:
        native = all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f))
        if not dense and factored is None and native and not sample:
            # reference-shaped result straight from the plan: entries above ACCURACY only
            log.info("Running virtualizer with %d %s fragments and %d vgates...",
                     len(virt.fragment_circuits), tuple(len(f) for f in virt.fragment_circuits),
                     len(virt.vgate_instructions))
            keys, vals, info = _planned_dict(virt, device, _qd.ACCURACY)
            log.info("Knitted in %.2fs.", info.knit_time)
            return dict(zip(keys.tolist(), vals.tolist())), info
        out, info = run_virtual_circuit_dense(virt, shots, device=device, factored=factored, sample=sample,
                                              seed=seed)
    if dense:
        return out, info
    keys, vals = engine.nearest_probability_distribution(engine.get_context(device), out, _qd.ACCURACY)
    return dict(zip(keys.tolist(), vals.tolist())), info


# ---------------------------------------------------------------------------- reductions of the knit
def _reducer(virt: VirtualCircuit, device: int, factored, group, sample: bool, *, readout=None, mitigate: bool = False):
    """Sweep for the marginal / expectation entry points: ``(KnitReducer, run_time)``. ``readout``: per-clbit
    confusion matrices (``observables.bit_channels``): the reducer then answers for the knit under that readout
    error (``KnitReducer.with_readout_error``) or, with ``mitigate``, under its inverse
    (``with_readout_mitigation``); the transform of the swept rows counts into ``run_time``."""
    from .observables import KnitReducer

    if group is not None:
        raise ValueError("marginals and expectation values run on one GPU (group must be None)")
    if sample:
        raise ValueError("marginals and expectation values are of the exact knit (sample=True is not supported)")
    if not all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f)):
        raise ValueError("marginals and expectation values need every fragment on the MI355X backend")
    if mitigate and readout is None:
        raise ValueError("mitigate=True needs the confusion matrices (readout)")
    log.info("Running virtualizer with %d %s fragments and %d vgates...", len(virt.fragment_circuits),
             tuple(len(f) for f in virt.fragment_circuits), len(virt.vgate_instructions))
    now = perf_counter()
    red = KnitReducer(virt, device=device, factored=factored)
    if readout is not None:
        red = red.with_readout_mitigation(readout) if mitigate else red.with_readout_error(readout)
    _sync(device)
    return red, perf_counter() - now


def run_virtual_circuit_marginal(virt: VirtualCircuit, clbits, *, device: int = 0, dense: bool = False,
                                 factored: bool | None = None, group=None, sample: bool = False,
                                 readout=None, mitigate: bool = False, npd: bool = False, accuracy: float = 0.0):
    """The knit's distribution of the clbits ``clbits`` alone (bit ``i`` of a key = ``clbits[i]``), all
    others summed out, without the 2^N output: the swept rows are reduced per fragment
    (``qk_reduce_bits``) and knitted narrow (:class:`observables.KnitReducer`). Returns
    ``(result, RunTimeInfo)``; the sweep is ``run_time``, reduce + combine ``knit_time``.

    ``dense=True``: the exact marginal as a float64 device tensor ``[2^k]``, not projected.
    ``dense=False``: its ``ACCURACY`` truncation and ``nearest_probability_distribution`` as a dict, the
    shape of :func:`run_virtual_circuit`'s result. Note that the projection does not commute with
    summing: the NPD of a marginal is not the marginal of the NPD of the full distribution.

    ``readout``: per-clbit confusion matrices (an ``[N, 2, 2]`` array, a dict ``{clbit: 2x2}`` or one 2x2 matrix for
    every measured clbit; ``observables.readout_matrix``): the answer is then that of the knit under this readout
    error, or with ``mitigate=True`` under its inverse, the readout-mitigated quasi-distribution
    (``KnitReducer.with_readout_error`` / ``with_readout_mitigation``; the swept rows are transformed once, inside
    ``run_time``). The other single-circuit entry points below take the same two keywords.

    ``npd=True``: the marginal of the nearest probability distribution of the full knit instead (``KnitReducer.project``
    over all clbits with the truncation ``accuracy``, then ``projected_marginal``): ``dense=True`` the tensor,
    ``dense=False`` the dict ``{key: value}`` of its positive entries.

    One GPU, exact instances, every fragment on the MI355X backend (``ValueError`` otherwise)."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    if npd:
        out = red.projected_marginal(clbits, red.project(accuracy=accuracy))
        _sync(device)
        info = RunTimeInfo(run_time, perf_counter() - now)
        if dense:
            return out, info
        keys = engine.torch().nonzero(out > 0).reshape(-1)
        return dict(zip(keys.tolist(), out[keys].tolist())), info
    out = red.marginal(clbits)
    if dense:
        _sync(device)
        return out, RunTimeInfo(run_time, perf_counter() - now)
    keys, vals = engine.nearest_probability_distribution(red.ctx, out, _qd.ACCURACY)
    info = RunTimeInfo(run_time, perf_counter() - now)
    log.info("Knitted in %.2fs.", info.knit_time)
    return dict(zip(keys.tolist(), vals.tolist())), info


def run_virtual_circuit_expectation(virt: VirtualCircuit, observables, *, device: int = 0,
                                    factored: bool | None = None, group=None, sample: bool = False,
                                    weights=None, method: str = "reduce", readout=None, mitigate: bool = False,
                                    npd: bool = False, accuracy: float = 0.0, bindings=None):
    """Expectation values of Pauli-Z strings on the exact knit (the quasi-distribution itself, no
    projection): ``sum_key (-1)^popcount(key & mask) R[key]`` per observable, without the 2^N output.
    ``observables``: int masks over the clbits, or ``'ZIIZ'`` strings (rightmost character = clbit 0,
    one character per clbit). Returns ``(float64 [M], RunTimeInfo)``; the sweep is ``run_time``,
    reduce + combine ``knit_time``. Same restrictions as :func:`run_virtual_circuit_marginal`.

    ``method="spectrum"`` answers from the fragments' Walsh-Hadamard spectra
    (:meth:`observables.KnitReducer.z_spectrum`): one transform, then a gather per mask, the route for
    thousands of strings and more; the masks may then be an integer numpy array or an int64 tensor.
    ``method="fused"`` reads the same spectra with the lookup kernel (``qk_knit_at``), one launch for all masks.
    ``weights`` (one per observable): the result is the float ``sum_j weights[j] <Z_j>`` instead, always
    by the spectrum route.

    ``npd=True``: of the nearest probability distribution of the knit instead (``KnitReducer.project`` over all clbits
    with the truncation ``accuracy``, then ``projected_expectation``: passes over all outcomes, eight masks each);
    the values then lie in [-mass, mass]. ``weights`` gives the weighted sum, formed on the host; ``method`` must be
    left at its default.

    ``bindings`` (float ``[B, P]``, columns in ``virt.parameters`` order, or a sequence of ``Parameter -> float``
    mappings): the circuit may hold run-time parameters, and the result gains a leading binding axis (``[B, M]``, or
    ``[B]`` with ``weights``). The batch is swept once by the :class:`parametric.ParametricKnit` of the circuit's
    structure (``parametric.cached_knit``: built on the first call, so from the second call on ``run_time`` is the
    bound sweep alone, without a compile). Exact knit by the ``"reduce"`` route only: no ``readout``, ``npd`` or other
    ``method``."""
    if bindings is not None:
        return _bound_expectation(virt, observables, bindings, device, factored, weights,
                                  plain=group is None and not sample and readout is None and not mitigate
                                  and not npd and method == "reduce")
    if npd and method != "reduce":
        raise ValueError(f"npd=True has one route: method must be left at its default, not {method!r}")
    if method not in ("reduce", "spectrum", "fused"):
        raise ValueError(f"method must be 'reduce', 'spectrum' or 'fused', not {method!r}")
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    if npd:
        vals = red.projected_expectation(observables, red.project(accuracy=accuracy))
        if weights is not None:
            w = np.asarray(weights.cpu() if hasattr(weights, "cpu") else weights, dtype=np.float64)
            if w.ndim != 1 or len(w) != len(vals):
                raise ValueError(f"{len(vals)} masks but weights of shape {w.shape}")
            vals = float(np.dot(vals, w))
    elif weights is None:
        vals = red.expectation(observables, method=method)
    else:
        vals = red.expectation_sum(observables, weights)
    info = RunTimeInfo(run_time, perf_counter() - now)
    log.info("Knitted in %.2fs.", info.knit_time)
    return vals, info


def _bound_expectation(virt: VirtualCircuit, observables, bindings, device: int, factored, weights, plain: bool):
    from . import parametric

    if not plain:
        raise ValueError("bindings: one GPU, the exact knit and method='reduce' only (no group, sample, readout, "
                         "mitigate or npd)")
    vals = parametric.binding_values(virt.parameters, bindings, batch=True)
    now = perf_counter()
    knit = parametric.cached_knit(virt, device, factored)
    qs = knit.sweep(vals) if len(vals) else []
    _sync(device)
    run_time = perf_counter() - now
    now = perf_counter()
    out = knit.expectation_of_rows(qs, len(vals), observables, weights)
    info = RunTimeInfo(run_time, perf_counter() - now)
    log.info("Knitted in %.2fs.", info.knit_time)
    return out, info


def run_virtual_circuit_gradient(virt: VirtualCircuit, observables, bindings, *, weights=None, parameters=None,
                                 device: int = 0, factored: bool | None = None):
    """Z-string expectation values of a parametric cut circuit and their exact parameter-shift gradient at every
    binding (``bindings`` as for :func:`run_virtual_circuit_expectation`): ``((values, grads), RunTimeInfo)``. With
    ``weights [M]`` the weighted sum, ``values [B]`` and ``grads [B, P']``, by the cotangent route of
    :meth:`parametric.ParametricKnit.value_and_gradient`; without, ``values [B, M]`` and ``grads [B, M, P']`` per
    observable. ``parameters``: the ``Parameter`` s to differentiate by (default ``virt.parameters``, in order). The
    plan is the cached :class:`parametric.ParametricKnit` of the circuit's structure, so a second call compiles
    nothing; ``run_time`` is the whole evaluation (sweeps, dots and the knit's small algebra are interleaved).
    One GPU, the exact knit, as ``bindings=`` there."""
    from . import parametric

    vals = parametric.binding_values(virt.parameters, bindings, batch=True)
    now = perf_counter()
    knit = parametric.cached_knit(virt, device, factored)
    if parameters is not None:  # the caller's Parameter objects, by position, as the cached plan knows them
        index = {p: i for i, p in enumerate(virt.parameters)}
        unknown = [getattr(p, "name", p) for p in parameters if p not in index]
        if unknown:
            raise ValueError(f"parameters: unknown {unknown}")
        parameters = [knit.parameters[index[p]] for p in parameters]
    out = knit.value_and_gradient(vals, observables, weights, parameters=parameters)
    _sync(device)
    info = RunTimeInfo(perf_counter() - now, 0.0)
    return out, info


def run_virtual_circuit_shots(virt: VirtualCircuit, shots: int = 20000, *, seed: int = 0, clbits=None,
                              memory: bool = False, device: int = 0, factored: bool | None = None, group=None,
                              sample: bool = False, readout=None, mitigate: bool = False, npd: bool = False,
                              accuracy: float = 0.0):
    """``shots`` measurement outcomes distributed as the exact knit, i.e. as the uncut circuit's output,
    without the 2^N distribution: drawn fragment by fragment from the swept rows
    (:meth:`observables.KnitReducer.sample`, ``qk_sample_rows``). Not ``run_virtual_circuit(sample=True)``,
    which samples the fragment instances and knits the noisy rows. Returns ``(result, RunTimeInfo)``; the
    sweep is ``run_time``, the chain of draws ``knit_time``.

    ``memory=False``: counts ``{key: count}`` (Python ints); ``memory=True``: the device int64 tensor
    ``[shots]`` of keys in draw order. ``clbits``: the measured clbits (bit ``i`` of a key = ``clbits[i]``),
    ``None`` = all. A pure function of (circuit, ``seed``, ``shots``); the first ``n`` shots of a longer
    run are an ``n``-shot run. Same restrictions as :func:`run_virtual_circuit_marginal`.

    ``npd=True``: drawn from the nearest probability distribution of the knit instead (``KnitReducer.project`` over
    ``clbits`` with the truncation ``accuracy``, then ``projected_sample``): what the shots of a knit with negative
    entries, a readout-mitigated one say, should follow. The fragment-by-fragment chain draws from clipped
    conditionals, which is exact only for a non-negative knit."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    if npd:
        keys = red.projected_sample(shots, red.project(clbits, accuracy=accuracy), seed)
    else:
        keys = red.sample(shots, seed, clbits)
    if memory:
        _sync(device)
        return keys, RunTimeInfo(run_time, perf_counter() - now)
    uniq, counts = engine.torch().unique(keys, return_counts=True)
    info = RunTimeInfo(run_time, perf_counter() - now)
    log.info("Knitted in %.2fs.", info.knit_time)
    return dict(zip(uniq.tolist(), counts.tolist())), info


def run_virtual_circuit_probabilities(virt: VirtualCircuit, keys, *, clbits=None, device: int = 0,
                                      factored: bool | None = None, group=None, sample: bool = False,
                                      readout=None, mitigate: bool = False):
    """The exact knit at the given outcome keys, i.e. the probabilities of chosen bitstrings (the
    quasi-distribution itself, no projection), without the 2^N output: one gathered row per fragment and key
    (:meth:`observables.KnitReducer.probabilities`, ``qk_knit_at``). ``keys``: ints, a list, an integer numpy
    array or an int64 tensor, e.g. the keys of :func:`run_virtual_circuit_shots`; ``clbits``: the clbits the
    keys are over (bit ``i`` of a key = ``clbits[i]``), ``None`` = all. Returns ``(float64 numpy [M],
    RunTimeInfo)``; the sweep is ``run_time``, the lookup ``knit_time``. Same restrictions as
    :func:`run_virtual_circuit_marginal`."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    vals = red.probabilities(keys, clbits).cpu().numpy()
    return vals, RunTimeInfo(run_time, perf_counter() - now)


def run_virtual_circuit_xeb(virt: VirtualCircuit, keys, *, clbits=None, device: int = 0,
                            factored: bool | None = None, group=None, sample: bool = False,
                            readout=None, mitigate: bool = False):
    """Linear cross-entropy benchmarking score of sampled ``keys`` against the exact knit:
    ``2^k * mean_j R[key_j] - 1`` over the ``k`` measured clbits (:meth:`observables.KnitReducer.linear_xeb`).
    Returns ``(float, RunTimeInfo)``; arguments, timing and restrictions as
    :func:`run_virtual_circuit_probabilities`."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    score = red.linear_xeb(keys, clbits)
    return score, RunTimeInfo(run_time, perf_counter() - now)


def run_virtual_circuit_collision(virt: VirtualCircuit, clbits=None, *, device: int = 0, factored: bool | None = None,
                                  group=None, sample: bool = False, readout=None, mitigate: bool = False):
    """The collision probability ``sum_y R_S[y]^2`` of the exact knit's marginal onto ``clbits`` (``None`` =
    all clbits), without the 2^N output: per fragment the Gram matrix of its swept rows (``qk_gram_rows``),
    then sums over pairs of terms (:meth:`observables.KnitReducer.collision_probability`). Returns
    ``(float, RunTimeInfo)``; the sweep is ``run_time``, Grams + combine ``knit_time``. Same restrictions as
    :func:`run_virtual_circuit_marginal`."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    value = red.collision_probability(clbits)
    return value, RunTimeInfo(run_time, perf_counter() - now)


def run_virtual_circuit_overlap(virt_a: VirtualCircuit, virt_b: VirtualCircuit, clbits=None, *, device: int = 0,
                                factored: bool | None = None, group=None, sample: bool = False):
    """The overlap ``sum_y R_S[y] R'_S[y]`` of the exact knits of two cut circuits, marginalised onto
    ``clbits`` (``None`` = all), without either 2^N output (:meth:`observables.KnitReducer.overlap`). The two
    circuits must have the same number of clbits and, on ``clbits``, fragments that measure the same sets.
    Returns ``(float, RunTimeInfo)``; both sweeps are ``run_time``. Same restrictions as
    :func:`run_virtual_circuit_marginal`."""
    red_a, time_a = _reducer(virt_a, device, factored, group, sample)
    red_b, time_b = _reducer(virt_b, device, factored, group, sample)
    now = perf_counter()
    value = red_a.overlap(red_b, clbits)
    return value, RunTimeInfo(time_a + time_b, perf_counter() - now)


def run_virtual_circuit_scan(virt: VirtualCircuit, clbits=None, *, threshold: float = 0.0, device: int = 0,
                             factored: bool | None = None, group=None, sample: bool = False,
                             readout=None, mitigate: bool = False):
    """Statistics of the exact knit that do not factorise over the fragments (mass, L1 norm and negativity, Shannon
    entropy, extrema and their keys, counts, a histogram of binades), of its marginal onto ``clbits`` (``None`` = all
    clbits), without the 2^N output: the knit is formed tile by tile on the matrix cores and consumed in registers
    (:meth:`observables.KnitReducer.scan`, ``qk_knit_scan``). Returns ``(observables.KnitScan, RunTimeInfo)``; the
    sweep is ``run_time``, the scan ``knit_time``. Same restrictions as :func:`run_virtual_circuit_marginal`."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    value = red.scan(clbits, threshold=threshold)
    return value, RunTimeInfo(run_time, perf_counter() - now)


def run_virtual_circuit_top_k(virt: VirtualCircuit, k: int, clbits=None, *, capacity: int = 1 << 24, device: int = 0,
                              factored: bool | None = None, group=None, sample: bool = False,
                              readout=None, mitigate: bool = False):
    """The ``k`` most probable outcomes of the exact knit (of its marginal onto ``clbits``) without the 2^N output
    (:meth:`observables.KnitReducer.top_k`: a scan with a histogram, then ``qk_knit_collect``). Returns
    ``({key: value} in descending order of value, RunTimeInfo)``. Same restrictions as
    :func:`run_virtual_circuit_marginal`."""
    red, run_time = _reducer(virt, device, factored, group, sample, readout=readout, mitigate=mitigate)
    now = perf_counter()
    keys, vals = red.top_k(k, clbits, capacity)
    return dict(zip(keys.tolist(), vals.tolist())), RunTimeInfo(run_time, perf_counter() - now)


def run_virtual_circuit_fidelity(virt_a: VirtualCircuit, virt_b: VirtualCircuit, clbits=None, *, device: int = 0,
                                 factored: bool | None = None, group=None, sample: bool = False, npd: bool = False,
                                 accuracy: float = 0.0):
    """The Hellinger fidelity of the exact knits of two cut circuits, marginalised onto ``clbits`` (``None`` = all),
    without either 2^N output (:meth:`observables.KnitReducer.hellinger_fidelity`). The circuits must have the same
    number of clbits and, on ``clbits``, fragments that measure the same sets. Returns ``(float, RunTimeInfo)``; both
    sweeps are ``run_time``. Same restrictions as :func:`run_virtual_circuit_marginal`.

    ``npd=True``: the fidelity of the two knits' nearest probability distributions, each of its entries with
    ``|R| > accuracy`` (:meth:`observables.KnitReducer.project`, then
    :meth:`~observables.KnitReducer.projected_hellinger_fidelity`): what the reference's ``cutVsUncutFidelity``
    compares. The default compares the knits clipped at zero, and ``accuracy`` is then not used."""
    red_a, time_a = _reducer(virt_a, device, factored, group, sample)
    red_b, time_b = _reducer(virt_b, device, factored, group, sample)
    now = perf_counter()
    if npd:
        pa, pb = red_a.project(clbits, accuracy=accuracy), red_b.project(clbits, accuracy=accuracy)
        value = red_a.projected_hellinger_fidelity(red_b, pa, pb)
    else:
        value = red_a.hellinger_fidelity(red_b, clbits)
    return value, RunTimeInfo(time_a + time_b, perf_counter() - now)


def run_virtual_circuit_npd(virt: VirtualCircuit, *, accuracy: float = _qd.ACCURACY, clbits=None,
                            capacity: int = 1 << 24, readout=None, mitigate: bool = False, device: int = 0,
                            factored: bool | None = None):
    """The reference-shaped result at any output width: ``({key: value}, RunTimeInfo)``, the
    ``nearest_probability_distribution`` of the knit's entries with ``|R| > accuracy`` (of its marginal onto
    ``clbits``; of the knit under ``readout`` / ``mitigate`` as in :func:`run_virtual_circuit_marginal`), in ascending
    order of value, equal values by key: the order of the reference's dict. The 2^N output is never formed: the
    threshold takes a few passes of ``qk_knit_project_scan`` (:meth:`observables.KnitReducer.project`), the kept
    entries are collected above it. ``accuracy=0`` projects the whole knit. More than ``capacity`` kept entries
    raise ``ValueError`` naming the count.

    An entry exactly at the threshold projects to 0.0: the reference lists it with the value 0.0, here it is not
    listed. One GPU, exact instances, every fragment on the MI355X backend."""
    red, run_time = _reducer(virt, device, factored, None, False, readout=readout, mitigate=mitigate)
    now = perf_counter()
    T = engine.torch()
    projection = red.project(clbits, accuracy=accuracy)
    if projection.kept > capacity:
        raise ValueError(f"{projection.kept} entries in the projection, more than capacity = {capacity}")
    keys, vals = red.projected_heavy_outputs(projection, capacity=capacity)
    keys, by_key = T.sort(keys)
    vals, by_val = T.sort(vals[by_key], stable=True)  # ascending; equal values stay in key order
    info = RunTimeInfo(run_time, perf_counter() - now)
    return dict(zip(keys[by_val].tolist(), vals.tolist())), info
