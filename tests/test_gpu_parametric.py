"""Run-time circuit parameters on the GPU: the bound sweep (``qk_sweep_bound``: PACKED and SPLIT interpreter,
per-program kernels) and ``parametric.ParametricKnit`` against the constant route on the bound circuit — the oracle's
knit, the uncut statevector and ``KnitReducer(VirtualCircuit(cut.bind(v)))``."""
import ctypes
import functools
import random

import numpy as np
import pytest

import parametric_cases as pc
from oracle import dense
from test_observables import np_expectation

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (VirtualCircuit, _lib, engine, parametric,
                                                                      run_virtual_circuit, run_virtual_circuit_expectation)
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.cutting import cut_circuit
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.parametric import ParametricKnit

pytestmark = pytest.mark.gpu
TOL = 1e-12  # the project's GPU-against-oracle tolerance per entry (tests/test_gpu_observables.py)


@pytest.fixture(scope="module")
def T(require_gpu):
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def packed():
    qc, spec = pc.packed_two_fragment()
    return qc, cut_circuit(qc, spec)


@functools.lru_cache(maxsize=None)
def packed_refs(B: int):
    """``(V, [oracle knit of the bound cut circuit], [uncut distribution of the bound circuit])``, read-only."""
    qc, cut = packed()
    V = pc.bindings(len(qc.parameters), B)
    knit = [dense.run_dense(cut.bind(v)) for v in V]
    unc = [dense.uncut_distribution(qc.bind(v)) for v in V]
    for a in knit + unc + [V]:
        a.setflags(write=False)
    return V, knit, unc


# ----------------------------------------------------------------------------- PACKED interpreter
@pytest.mark.parametrize("B", [5, 70])
def test_packed_bindings_share_tiles(T, B):
    """Fragments of 3 and 2 qubits, one cx cut, every u layer parametric. A tile holds 256 units and a binding
    has 5 or 6 branch jobs, so bindings share tiles (B = 5: one partial tile) and B = 70 spills into a second
    tile. Every binding's full marginal against the oracle knit and the uncut distribution."""
    qc, cut = packed()
    V, knit, unc = packed_refs(B)
    pk = ParametricKnit(VirtualCircuit(cut))
    assert pk.parameters == qc.parameters and pk.num_parameters == 30
    for fs in pk.frags:
        assert fs.dprog.enc.packed and fs.dprog.module is None and fs.prog.num_params > 0
        assert 256 % fs.jobs.n_jobs != 0 and (B == 5 or B * fs.jobs.n_jobs > 256)
    reds = pk.bind_many(V)
    assert len(reds) == B
    worst = 0.0
    for red, k, u in zip(reds, knit, unc):
        got = red.marginal(list(range(5))).cpu().numpy()
        worst = max(worst, float(np.abs(got - k).max()), float(np.abs(got - u).max()))
    print(f"packed B={B}: max|gpu - oracle| = {worst:.3e}")
    assert worst <= TOL
    # the dict and the sequence form of one binding, and the constant route's reducer on the bound circuit
    for b in (0, 1, B - 1):
        one = pk.bind(dict(zip(qc.parameters, V[b])))
        assert all(T.equal(x, y) for x, y in zip(one.qs, pk.bind(V[b]).qs))
        ref = KnitReducer(VirtualCircuit(cut.bind(V[b])))
        assert float((one.marginal([4, 0, 2]) - ref.marginal([4, 0, 2])).abs().max()) <= TOL
        np.testing.assert_allclose(one.expectation([0b10011, 0b11111]), ref.expectation([0b10011, 0b11111]), atol=TOL, rtol=0)


def test_bound_reducer_is_a_complete_reducer(T):
    """What ``bind`` returns is a ``KnitReducer`` like any other: spectrum, shots, probabilities, scan, channels and
    the projection answer as the constant route's reducer does."""
    qc, cut = packed()
    v = pc.bindings(len(qc.parameters), 3)[1]
    red = ParametricKnit(VirtualCircuit(cut)).bind(v)
    ref = KnitReducer(VirtualCircuit(cut.bind(v)))
    assert isinstance(red, KnitReducer)
    masks = list(range(32))
    np.testing.assert_allclose(red.expectation(masks, method="spectrum"), ref.expectation(masks, method="spectrum"), atol=TOL, rtol=0)
    keys = [0, 5, 17, 31]
    assert float((red.probabilities(keys) - ref.probabilities(keys)).abs().max()) <= TOL
    assert abs(red.collision_probability() - ref.collision_probability()) <= TOL
    assert abs(red.scan().mass - ref.scan().mass) <= TOL and abs(red.scan().max - ref.scan().max) <= TOL
    noisy, noisy_ref = red.with_readout_error(np.array([[0.97, 0.05], [0.03, 0.95]])), ref.with_readout_error(
        np.array([[0.97, 0.05], [0.03, 0.95]]))
    assert float((noisy.marginal([0, 1, 2, 3, 4]) - noisy_ref.marginal([0, 1, 2, 3, 4])).abs().max()) <= TOL
    pr, pr_ref = red.project(), ref.project()
    assert float((red.projected_marginal([0, 3], pr) - ref.projected_marginal([0, 3], pr_ref)).abs().max()) <= 1e-11
    shots = red.sample(4000, seed=3).cpu().numpy()
    assert shots.shape == (4000,) and shots.min() >= 0 and shots.max() < 32
    exact = dense.uncut_distribution(qc.bind(v))
    assert 0.5 * np.abs(np.bincount(shots, minlength=32) / 4000 - exact).sum() < 0.1  # 4000 draws of 32 outcomes


# ----------------------------------------------------------------------------- SPLIT: interpreter and compiled
SPLIT_B = 3


@functools.lru_cache(maxsize=None)
def split_refs(kind: str):
    """``(V, [OracleRows of cut.bind(v)], marginal clbits, 32 Z masks)`` of a SPLIT case, computed once."""
    qc, spec, cut = pc.split_built(kind)
    V = pc.bindings(len(qc.parameters), SPLIT_B, seed=11)
    V.setflags(write=False)
    refs = [pc.OracleRows(cut.bind(v)) for v in V]
    per_frag = refs[0].clbits
    rng = random.Random(8)
    # the marginal: 5 measured clbits of each fragment (all of a fragment that measures fewer), shuffled
    keep = [c for cl in per_frag for c in (cl if len(cl) <= 5 else rng.sample(cl, 5))]
    rng.shuffle(keep)
    measured = refs[0].measured()
    masks = [sum(1 << c for c in measured if rng.random() < 0.5) for _ in range(30)] + [sum(1 << c for c in measured), 0]
    marg = [r.marginal(keep) for r in refs]
    expv = [np.array([r.expectation(m) for m in masks]) for r in refs]
    return V, keep, masks, marg, expv


SPLIT_MODES = {"interpreter": ("0", None), "jit10": ("1", "10"), "jit13": ("1", "13")}


@pytest.mark.parametrize("mode", sorted(SPLIT_MODES))
@pytest.mark.parametrize("kind", pc.SPLIT_KINDS)
def test_split_bound_sweep_matches_oracle(T, monkeypatch, kind, mode):
    """Fragments of 13 and 14 qubits on the SPLIT interpreter (QKNIT_SWEEP_JIT=0) and on the per-program kernels at
    tile widths 10 (two passes, sparse INIT; the traced case's 14-qubit fragment runs three passes on the 12-bit
    tiles its 7 traced qubits need) and 13 (the ``rzz`` case's 14-qubit fragment: ONE pass), three distinct
    bindings swept together: a marginal onto five measured clbits of each fragment and 32 Z strings over all
    measured clbits against the oracle's knit of the bound circuit. Neither side forms the 2^27 output."""
    jit_env, tb = SPLIT_MODES[mode]
    monkeypatch.setenv("QKNIT_SWEEP_JIT", jit_env)
    if tb:
        monkeypatch.setenv("QKNIT_JIT_TILE_BITS", tb)
    qc, spec, cut = pc.split_built(kind)
    V, keep, masks, marg, expv = split_refs(kind)
    pk = ParametricKnit(VirtualCircuit(cut), jit=True if tb else None)
    for fs in pk.frags:
        enc = fs.dprog.enc
        assert not enc.packed and sorted(f.prog.n for f in pk.frags) == [13, 14] and len(fs.prog.ops) <= 40
        assert (fs.dprog.module is not None) == bool(tb) and fs.prog.num_params > 0
        if tb == "10":
            assert len(enc.passes) >= 2 and enc.tile_bits == (12 if (kind == "traced") else 10)
        if tb == "13" and kind == "rzz" and fs.prog.n == 14:
            assert len(enc.passes) == 1 and enc.tile_bits == 13
    if kind == "cx_cut":
        assert all(fs.jobs.n_jobs > fs.n_rows for fs in pk.frags)  # branch jobs: the label-summing FINAL pass
    if kind == "traced":
        assert sorted(fs.fold for fs in pk.frags) == [1, 16] and min(fs.prog.m for fs in pk.frags) == 3
    reds = pk.bind_many(V)
    worst_m = worst_e = 0.0
    for red, m_ref, e_ref in zip(reds, marg, expv):
        worst_m = max(worst_m, float(np.abs(red.marginal(keep).cpu().numpy() - m_ref).max()))
        worst_e = max(worst_e, float(np.abs(red.expectation(masks) - e_ref).max()))
    print(f"split {kind} {mode}: max|gpu - oracle| marginal {worst_m:.3e}, Z strings {worst_e:.3e}")
    assert worst_m <= TOL and worst_e <= TOL
    # the bindings differ, and so do their answers: a sweep that read another binding's table cannot pass the above
    assert float(np.abs(marg[0] - marg[1]).max()) > 1e-3


# ----------------------------------------------------------------------------- batch == singles
@pytest.mark.parametrize("case", ["packed", "cx_cut:interpreter", "wire_cut:jit", "traced:jit"])
def test_batch_equals_singles_bit_for_bit(T, monkeypatch, case):
    """``bind_many(V)[i].qs`` against ``bind(V[i]).qs`` for B = 5, in one launch sequence and with the workspace
    budget forced so that the batch runs in 3 chunks: a unit's arithmetic does not depend on its neighbours, so
    anything but equality is an indexing error."""
    name, _, mode = case.partition(":")
    monkeypatch.setenv("QKNIT_SWEEP_JIT", "0" if mode == "interpreter" else "1")
    cut = packed()[1] if name == "packed" else pc.split_built(name)[2]
    pk = ParametricKnit(VirtualCircuit(cut), jit=(mode == "jit") or None)
    V = pc.bindings(pk.num_parameters, 5, seed=21)
    singles = [pk.bind(v).qs for v in V]
    whole = pk.bind_many(V)
    # two bindings' worth of sweep state per launch: chunks of 2, 2 and 1 bindings for every fragment
    budgets = {fs.jobs.n_jobs * (16 << fs.dprog.enc.n_eff) for fs in pk.frags}
    chunked = [None] * 5
    rows = [[] for _ in range(5)]
    for fs in pk.frags:
        budget = 2 * fs.jobs.n_jobs * (16 << fs.dprog.enc.n_eff)
        assert engine.binding_chunks(5, budget // 2, budget) == [(0, 2), (2, 4), (4, 5)]
        q = engine.sweep_fragment_bound(pk.ctx, fs, fs.prog.bind_matrices(V), budget)
        for b in range(5):
            rows[b].append(q[b])
    assert budgets
    for b in range(5):
        assert len(whole[b].qs) == len(singles[b]) == len(rows[b])
        for one, many, ch in zip(singles[b], whole[b].qs, rows[b]):
            assert many.is_contiguous() and T.equal(one, many) and T.equal(one, ch)
    assert not T.equal(singles[1][0], singles[2][0])


# ----------------------------------------------------------------------------- no recompile
def test_bind_never_compiles(T, monkeypatch):
    """Calls into ``qk_module_compile`` / ``qk_module_load`` after the constructor and after three further binds."""
    lib = _lib.lib()
    calls = []
    for fn in ("qk_module_compile", "qk_module_load"):
        real = getattr(lib, fn)
        monkeypatch.setattr(lib, fn, lambda *a, _real=real, _fn=fn: (calls.append(_fn), _real(*a))[1])
    monkeypatch.setenv("QKNIT_SWEEP_JIT", "1")
    monkeypatch.setenv("QKNIT_JIT_TILE_BITS", "11")  # a width no other test compiles these programs at
    pk = ParametricKnit(VirtualCircuit(pc.split_built("wire_cut")[2]), jit=True)
    assert all(fs.dprog.module is not None for fs in pk.frags)
    built = len(calls)
    assert built >= 2  # one module per fragment went through the library
    rng = np.random.default_rng(2)
    answers = [pk.bind(rng.uniform(-3, 3, pk.num_parameters)).expectation([1, 2]) for _ in range(3)]
    assert len(calls) == built
    assert not np.allclose(answers[0], answers[1])


def test_expectation_entry_builds_one_knit_per_structure(T):
    """Three ``run_virtual_circuit_expectation(..., bindings=...)`` calls on circuits built alike from different
    ``Parameter`` objects share one ``ParametricKnit``; the values are those of the oracle."""
    parametric.clear_knit_cache()
    before = parametric.knits_built[0]
    V, knit, _ = packed_refs(5)
    masks = [0b00001, 0b10110, 0b11111]
    ref = np.array([[np_expectation(k, m) for m in masks] for k in knit])
    for call in range(3):
        qc, spec = pc.packed_two_fragment()  # fresh parameters, same structure
        virt = VirtualCircuit(cut_circuit(qc, spec))
        bind = V[call:call + 3] if call < 2 else [dict(zip(qc.parameters, v)) for v in V[2:5]]
        got, info = run_virtual_circuit_expectation(virt, masks, bindings=bind)
        assert got.shape == (3, 3) and info.run_time > 0
        np.testing.assert_allclose(got, ref[call:call + 3] if call < 2 else ref[2:5], atol=TOL, rtol=0)
    assert parametric.knits_built[0] == before + 1
    with pytest.raises(ValueError, match="bindings"):
        run_virtual_circuit_expectation(virt, masks, bindings=V[:1], method="spectrum")


# ----------------------------------------------------------------------------- batched expectation
def test_batched_expectation(T):
    qc, cut = packed()
    B = 5
    V, knit, _ = packed_refs(B)
    pk = ParametricKnit(VirtualCircuit(cut))
    rng = random.Random(4)
    masks = [rng.getrandbits(5) for _ in range(engine.REDUCE_BITS_BATCH + 3)] + [0, 31]
    got = pk.expectation(V, masks)
    assert got.shape == (B, len(masks)) and got.dtype == np.float64
    ref = np.array([[np_expectation(k, m) for m in masks] for k in knit])
    singles = np.stack([pk.bind(v).expectation(masks) for v in V])
    print(f"batched expectation: max|gpu - oracle| = {np.abs(got - ref).max():.3e}, "
          f"max|batch - singles| = {np.abs(got - singles).max():.3e}")
    assert np.abs(got - ref).max() <= TOL
    assert np.abs(got - singles).max() <= TOL
    w = np.array([rng.uniform(-1, 1) for _ in masks])
    weighted = pk.expectation(V, masks, weights=w)
    assert weighted.shape == (B,)
    assert np.abs(weighted - ref @ w).max() <= TOL and np.abs(weighted - got @ w).max() <= TOL
    assert pk.expectation(V[:0], masks).shape == (0, len(masks))
    with pytest.raises(ValueError):
        pk.expectation(V, masks, weights=w[:-1])
    with pytest.raises(ValueError):
        pk.expectation(V[:, :-1], masks)


def test_batched_expectation_split(T, monkeypatch):
    """The same on SPLIT fragments (compiled, label rows): ``qk_reduce_bits`` over all B * rows rows at once."""
    monkeypatch.setenv("QKNIT_SWEEP_JIT", "1")
    monkeypatch.setenv("QKNIT_JIT_TILE_BITS", "10")
    V, keep, masks, marg, expv = split_refs("cx_cut")
    pk = ParametricKnit(VirtualCircuit(pc.split_built("cx_cut")[2]), jit=True)
    got = pk.expectation(V, masks)
    assert got.shape == (SPLIT_B, 32)
    assert np.abs(got - np.stack(expv)).max() <= TOL


# ----------------------------------------------------------------------------- refusals
def test_constant_routes_and_unbound_entries_refuse_parametric_programs(T):
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.pipeline import KnitPipeline

    qc, cut = packed()
    virt = VirtualCircuit(cut)
    with pytest.raises(ValueError, match="ParametricKnit"):
        run_virtual_circuit(virt, dense=True)
    with pytest.raises(ValueError, match="ParametricKnit"):
        KnitPipeline(virt)
    with pytest.raises(ValueError, match="ParametricKnit"):
        KnitReducer(virt)
    ctx = engine.get_context(0)
    for cut_ in (cut, pc.split_built("cx_cut")[2]):
        pk = ParametricKnit(VirtualCircuit(cut_), jit=True)
        for fs in pk.frags:
            slot_t, sign_t, off_t = engine.jobs_to_device(fs.jobs, 0)
            with pytest.raises(_lib.QknitError, match="run-time parameters"):  # refused on the host, before any launch
                engine.sweep_jobs(ctx, fs.dprog, slot_t, sign_t, fs.jobs.n_jobs)
            with pytest.raises(ValueError, match="sweep_fragment_bound"):
                engine.sweep_fragment(ctx, fs)
            with pytest.raises(ValueError, match="binding matrices"):
                engine.sweep_fragment_bound(ctx, fs, np.zeros((2, fs.prog.num_params + 1, 2, 2)))
            # the bound entry itself: a table too short for the program's param indices
            enc = fs.dprog.enc
            mats = T.zeros(8 * enc.n_params, dtype=T.float64, device="cuda")
            out = T.zeros((fs.jobs.n_jobs, 1 << enc.m), dtype=T.float64, device="cuda")
            ws = T.zeros(max(fs.jobs.n_jobs * (16 << enc.n) * (not enc.packed), 8), dtype=T.uint8, device="cuda")
            for n_bind, n_params, table in ((0, enc.n_params, mats), (1, enc.n_params - 1, mats), (1, enc.n_params, None)):
                st = ctx.lib.qk_sweep_bound(ctx.handle, fs.dprog.module, ctypes.byref(fs.dprog.struct), enc.ops.ctypes.data, len(enc.ops),
                                            n_bind, n_params, table.data_ptr() if table is not None else None,
                                            fs.jobs.n_jobs, slot_t.data_ptr(), sign_t.data_ptr(), 0, None,
                                            ws.data_ptr(), ws.numel(), out.data_ptr())
                assert st != 0
            st = ctx.lib.qk_sweep_bound(ctx.handle, fs.dprog.module, ctypes.byref(fs.dprog.struct), enc.ops.ctypes.data, len(enc.ops), 1,
                                        enc.n_params, mats.data_ptr(), fs.jobs.n_jobs, slot_t.data_ptr(),
                                        sign_t.data_ptr(), 0, None, ws.data_ptr(), ws.numel() - 9 if not enc.packed else 0,
                                        out.data_ptr())
            assert (st != 0) == (not enc.packed)  # SPLIT: a workspace below n_bind * n_jobs states
    T.cuda.synchronize()
