"""Parameter-shift gradients on the GPU: ``qk_rows_dot`` against ``math.fsum`` and against itself (bits), the cotangent
identity, ``ParametricKnit.value_and_gradient`` against shifts and central differences of the separately pinned
``ParametricKnit.expectation``, chunking, the edge cases and the entry point."""
import ctypes
import functools
import math
import random

import numpy as np
import pytest

import gradient_cases as gc
import parametric_cases as pc

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (VirtualCircuit, _lib, engine, parametric,
                                                                      run_virtual_circuit_expectation,
                                                                      run_virtual_circuit_gradient)
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import observables as obs
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.cutting import cut_circuit
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.parametric import ParametricKnit

pytestmark = pytest.mark.gpu
TOL = 1e-12  # the project's GPU-against-oracle tolerance per entry (tests/test_gpu_observables.py)
SEG = obs.ROWS_DOT_SEGMENT
QK_EARG = 1


@pytest.fixture(scope="module")
def T(require_gpu):
    import torch

    return torch


# ----------------------------------------------------------------------------- qk_rows_dot
def _placed(T, host: np.ndarray, ld: int, offset: int):
    """``host [rows, n]`` on the device with row stride ``ld`` doubles, the first row ``offset`` doubles into a fresh
    (256-byte aligned) buffer whose other elements are NaN: a read outside the rows poisons the result."""
    rows, n = host.shape
    buf = T.full((offset + rows * ld + 2,), float("nan"), dtype=T.float64, device="cuda")
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :n]
    view.copy_(T.from_numpy(host))
    assert view.data_ptr() % 256 == 8 * offset % 256
    return view


DOT_N = [1, 2, 3, 255, 256, 257, SEG - 1, SEG, SEG + 1, 3 * SEG + 5, 1 << 17]
DOT_UNITS = [(1, 1), (3, 1), (3, 3), (8, 1), (8, 2), (8, 8)]  # (units, per): per in {1, 2, units} where it divides


@pytest.mark.parametrize("n", DOT_N)
def test_rows_dot_shapes(T, n):
    """Every (units, per) at one ``n``: inputs of mixed signs over 20 binades, ``ldq > n`` and ``ldd > n``. The
    aligned placement (16-byte aligned base, even leading dimensions: 16-byte loads) against ``math.fsum`` of the
    products within ``(L + 1) 2^-53 sum |Q_i D_i|``, ``L = observables.rows_dot_chain(n)`` being the longest chain of
    additions in the kernel's association (qknit_dot.hip: 16 fma + 1 + 6 + 3 per segment, then ceil(segments / 64)
    + 6). Bit for bit the same: a second launch; the misaligned placement (odd leading dimensions, base 8 bytes off:
    8-byte loads), and Q aligned with D misaligned and the reverse; every unit launched alone with ``per = 1``."""
    ctx = engine.get_context(0)
    ctx.bind_stream()
    rng = np.random.default_rng(n)
    L = obs.rows_dot_chain(n)
    even = n + 2 + (n & 1)
    worst = 0.0
    for units, per in DOT_UNITS:
        Q, D = gc.signed_values(rng, (units, n)), gc.signed_values(rng, (units // per, n))
        Qa, Da = _placed(T, Q, even, 0), _placed(T, D, even + 2, 2)
        Qm, Dm = _placed(T, Q, even + 1, 1), _placed(T, D, even + 3, 3)
        got = engine.rows_dot(ctx, Qa, Da, per)
        again = engine.rows_dot(ctx, Qa, Da, per)
        host = got.cpu().numpy()
        assert host.shape == (units,) and np.isfinite(host).all()
        for u in range(units):
            ref, mag = gc.fsum_dot(Q[u], D[u // per])
            err = abs(host[u] - ref) / ((L + 1) * 2.0 ** -53 * mag)
            worst = max(worst, err)
            assert err <= 1.0, (units, per, u, host[u], ref)
        assert T.equal(got, again)
        for q, d in ((Qm, Dm), (Qa, Dm), (Qm, Da)):
            assert T.equal(got, engine.rows_dot(ctx, q, d, per)), (units, per)
        for u in range(units):
            for q, d in ((Qa, Da), (Qm, Dm)):
                alone = engine.rows_dot(ctx, q[u:u + 1], d[u // per:u // per + 1], 1)
                assert T.equal(alone, got[u:u + 1]), (units, per, u)
    print(f"qk_rows_dot n={n}: L = {L}, worst error / bound = {worst:.3f}")


def test_rows_dot_refusals(T):
    """Each refusal is QK_EARG with a message and leaves ``out`` as it was; ``units == 0`` is QK_OK and a no-op; the
    wrapper turns wrong shapes into ``ValueError`` before the library is called."""
    ctx = engine.get_context(0)
    ctx.bind_stream()
    lib = ctx.lib
    units, per, n = 4, 2, 300
    Q = T.ones((units, n), dtype=T.float64, device="cuda")
    D = T.ones((units // per, n), dtype=T.float64, device="cuda")
    out = T.full((units,), -7.0, dtype=T.float64, device="cuda")
    need = ctypes.c_int64()
    assert lib.qk_rows_dot_workspace_bytes(units, n, ctypes.byref(need)) == 0 and need.value == units * 8
    assert lib.qk_rows_dot_workspace_bytes(units, 2 * SEG + 1, ctypes.byref(need)) == 0 and need.value == units * 3 * 8
    assert lib.qk_rows_dot_workspace_bytes(-1, n, ctypes.byref(need)) == QK_EARG
    assert lib.qk_rows_dot_workspace_bytes(units, 0, ctypes.byref(need)) == QK_EARG
    ws = T.zeros(units, dtype=T.float64, device="cuda")
    good = dict(units=units, per=per, n=n, Q=Q.data_ptr(), ldq=n, D=D.data_ptr(), ldd=n, out=out.data_ptr(),
                ws=ws.data_ptr(), ws_bytes=units * 8)

    def call(**change):
        a = {**good, **change}
        return lib.qk_rows_dot(ctx.handle, a["units"], a["per"], a["n"], a["Q"], a["ldq"], a["D"], a["ldd"], a["out"],
                               a["ws"], a["ws_bytes"])

    bad = [dict(units=-2), dict(per=0), dict(per=3), dict(n=0), dict(ldq=n - 1), dict(ldd=n - 1), dict(Q=None),
           dict(D=None), dict(out=None), dict(ws=None), dict(ws_bytes=units * 8 - 1)]
    for change in bad:
        assert call(**change) == QK_EARG, change
        assert b"qk_rows_dot" in lib.qk_last_error(ctx.handle), change
    assert call(units=0, ws=None, ws_bytes=0) == 0
    T.cuda.synchronize()
    assert T.equal(out, T.full_like(out, -7.0))
    assert call() == 0
    assert T.equal(out, T.full_like(out, float(n)))
    assert engine.rows_dot(ctx, Q[:0], D[:0], per).shape == (0,)
    for q, d, p in ((Q, D, 3), (Q, D, 0), (Q, D[:, :-1], per), (Q.float(), D, per), (Q.cpu(), D.cpu(), per),
                    (Q.t(), D.t(), per), (Q[0], D[0], 1)):
        with pytest.raises(ValueError):
            engine.rows_dot(ctx, q, d, p)


# ----------------------------------------------------------------------------- plans under test
@functools.lru_cache(maxsize=None)
def packed():
    qc, spec = pc.packed_two_fragment()
    return qc, cut_circuit(qc, spec)


SPLIT_MODES = {"interpreter": ("0", None), "jit10": ("1", "10"), "jit13": ("1", "13")}  # as test_gpu_parametric.py
SPLIT_MODE_OF = {"cx_cut": "jit10", "wire_cut": "interpreter", "traced": "jit10", "rzz": "jit13"}


def _split_knit(monkeypatch, kind: str):
    jit_env, tb = SPLIT_MODES[SPLIT_MODE_OF[kind]]
    monkeypatch.setenv("QKNIT_SWEEP_JIT", jit_env)
    if tb:
        monkeypatch.setenv("QKNIT_JIT_TILE_BITS", tb)
    qc, spec, cut = pc.split_built(kind)
    pk = ParametricKnit(VirtualCircuit(cut), jit=True if tb else None)
    assert all((fs.dprog.module is not None) == bool(tb) for fs in pk.frags)
    return qc, pk


def _masks_and_weights(n_clbits: int, M: int, seed: int):
    rng = random.Random(seed)
    masks = [rng.getrandbits(n_clbits) for _ in range(M)]
    return masks, np.array([rng.uniform(-1, 1) for _ in masks])


def _omega(pk: ParametricKnit, column: int) -> float:
    return sum(gc.omega_of(fs.prog.shift_occurrences(), column) for fs in pk.frags)


# ----------------------------------------------------------------------------- cotangent identity
@pytest.mark.parametrize("case", ["packed", "cx_cut"])
def test_cotangent_identity_on_the_device(T, monkeypatch, case):
    """``<cotangent_rows_f, q_f> = E_w`` of ``ParametricKnit.expectation`` for every fragment (``E_w`` is linear in each
    fragment's rows), on the packed 3 + 2 circuit and on fragments of 13 + 14 qubits; two of the masks coincide on
    the first fragment and two on the second. Bound: the per-entry tolerance times ``max(1, |w|_1)``."""
    if case == "packed":
        pk = ParametricKnit(VirtualCircuit(packed()[1]))
    else:
        _, pk = _split_knit(monkeypatch, case)
    N = pk._template.N
    masks, w = _masks_and_weights(N, 7, seed=3)
    first = sum(1 << c for c in pk._template.clbits[0])
    masks[2] = (masks[0] & first) | (masks[1] & ~first)  # equals masks[0] on fragment 0, masks[1] on fragment 1
    v = pc.bindings(pk.num_parameters, 3, seed=9)[1]
    qs_b = [q[0] for q in pk.sweep(v[None])]
    E = float(pk.expectation(v[None], masks, w)[0])
    Ds = pk.cotangent_rows(qs_b, masks, w)
    assert len(Ds) == len(qs_b)
    bound = TOL * max(1.0, float(np.abs(w).sum()))
    for D, q in zip(Ds, qs_b):
        assert D.shape == q.shape and D.is_cuda
        dot = float(engine.rows_dot(pk.ctx, q.reshape(1, -1), D.reshape(1, -1))[0])
        print(f"cotangent {case}: <D, q> - E = {dot - E:.3e} (E = {E:.6f}, bound {bound:.2e})")
        assert abs(dot - E) <= bound
    assert abs(E) > 1e-6
    with pytest.raises(ValueError):
        pk.cotangent_rows(qs_b, masks, None)


# ----------------------------------------------------------------------------- exact reference: every parameter once
@functools.lru_cache(maxsize=None)
def packed_shift_reference():
    """``(V [3, 30], masks, w, E [3, 5], dE [3, 5, 30])`` of the packed circuit, where every parameter is one angle of
    one ``u``: ``dE/dp = (E(V + pi/2 e_p) - E(V - pi/2 e_p)) / 2`` from the existing ``expectation``. Read-only."""
    qc, cut = packed()
    pk = ParametricKnit(VirtualCircuit(cut))
    P = pk.num_parameters
    V = pc.bindings(P, 3)
    masks, w = _masks_and_weights(5, 5, seed=12)
    shifted = V[:, None, None, :] + (math.pi / 2) * np.array([1.0, -1.0])[None, None, :, None] * np.eye(P)[None, :, None, :]
    Es = pk.expectation(shifted.reshape(-1, P), masks).reshape(3, P, 2, len(masks))
    dE = 0.5 * (Es[:, :, 0] - Es[:, :, 1]).transpose(0, 2, 1)
    out = (V, tuple(masks), w, pk.expectation(V, masks), dE)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def test_gradient_where_every_parameter_occurs_once(T):
    """Bindings all zeros, random and all pi/2, 5 masks with weights: the cotangent route ``[B, P]``, the reduce route
    ``[B, M, P]`` per mask and the cotangent route at one-hot weights, each within ``1e-12 max(1, |w|_1)`` per entry of
    the whole-circuit shifts of ``expectation``."""
    V, masks, w, E, dE = packed_shift_reference()
    masks = list(masks)
    pk = ParametricKnit(VirtualCircuit(packed()[1]))
    bound = TOL * max(1.0, float(np.abs(w).sum()))
    val, grad = pk.value_and_gradient(V, masks, w)
    assert val.shape == (3,) and grad.shape == (3, 30)
    print(f"cotangent route: max|grad - shifts| = {np.abs(grad - np.einsum('bmp,m->bp', dE, w)).max():.3e}")
    assert np.array_equal(val, pk.expectation(V, masks, w))
    assert np.abs(grad - np.einsum("bmp,m->bp", dE, w)).max() <= bound
    vals, grads = pk.value_and_gradient(V, masks)
    assert vals.shape == (3, 5) and grads.shape == (3, 5, 30)
    print(f"reduce route: max|grad - shifts| = {np.abs(grads - dE).max():.3e}")
    assert np.array_equal(vals, E) and np.abs(grads - dE).max() <= TOL
    for m in range(5):
        hot = np.zeros(5)
        hot[m] = 1.0
        g1 = pk.gradient(V, masks, hot)
        assert np.abs(g1 - grads[:, m]).max() <= TOL and np.abs(g1 - dE[:, m]).max() <= TOL
    assert np.abs(dE[1]).max() > 1e-2 and np.abs(dE[0]).max() <= TOL  # all angles zero: every Z string at an extremum


# ----------------------------------------------------------------------------- shared and affine parameters
def _chosen(qc, kind: str) -> list:
    """``shared``, one ``ry`` angle, the ``rzz`` and ``cp`` angles (the ``rzz`` case) and one ``u`` angle of a SPLIT case,
    found in the circuit's own instructions."""
    shared = {p.name: p for p in qc.parameters}["t0"]
    first = {}
    for instr in qc:
        op = instr.operation
        for a in getattr(op, "params", ()):
            first.setdefault(op.name, []).extend(p for p in getattr(a, "terms", {}) if p is not shared)
    picked = [shared, first["ry"][0]]
    if kind == "rzz":
        picked += [first["rzz"][0], first["rzz"][1], first["cp"][0]]  # rzz(t - shared), rzz(t) and cp(0.5 t)
    return picked + [first["u"][0]]


@pytest.mark.parametrize("kind", pc.SPLIT_KINDS)
def test_shared_and_affine_parameters_against_central_differences(T, monkeypatch, kind):
    """Fragments of 13 and 14 qubits whose parameter ``shared`` sits in some twenty angles of both fragments, halved
    in ``rz(0.5 shared + t - 0.25)``, negated in ``rzz(t - shared)``: the gradient by ``shared``, an ``ry`` angle, the
    ``rzz`` and ``cp`` angles and a ``u`` angle against the central difference of ``expectation`` at h = 1e-5, within
    ``gradient_cases.difference_bound`` of ``Omega`` (the sum of the parameter's |coefficients| over the occurrences
    of both fragments) and values in ``[-|w|_1, |w|_1]``."""
    qc, pk = _split_knit(monkeypatch, kind)
    chosen = _chosen(qc, kind)
    cols = [pk.parameters.index(p) for p in chosen]
    N = pk._template.N
    masks, w = _masks_and_weights(N, 6, seed=5)
    v = pc.bindings(pk.num_parameters, 3, seed=17)[1]
    val, grad = pk.value_and_gradient(v[None], masks, w, parameters=chosen)
    assert grad.shape == (1, len(chosen))
    steps = np.repeat(v[None], 2 * len(cols), axis=0)
    for j, c in enumerate(cols):
        steps[2 * j, c] += gc.H_STEP
        steps[2 * j + 1, c] -= gc.H_STEP
    Es = pk.expectation(steps, masks, w).reshape(len(cols), 2)
    ref = (Es[:, 0] - Es[:, 1]) / (2 * gc.H_STEP)
    scale = float(np.abs(w).sum())
    for j, c in enumerate(cols):
        omega = _omega(pk, c)
        bound = gc.difference_bound(omega, scale)
        print(f"{kind} d/d{chosen[j].name}: gradient {grad[0, j]:+.9f}, difference {ref[j]:+.9f}, "
              f"|diff| {abs(grad[0, j] - ref[j]):.3e}, Omega {omega:g}, bound {bound:.3e}")
    assert _omega(pk, cols[0]) > 5.0  # shared: many occurrences in both fragments
    for j, c in enumerate(cols):
        assert abs(grad[0, j] - ref[j]) <= gc.difference_bound(_omega(pk, c), scale)
    assert np.abs(ref).max() > 1e-3


def test_shared_parameter_against_the_chain_rule_of_the_deshared_circuit(T):
    """One small circuit built twice: with ``s`` and ``a`` inside eight angles (``gradient_cases.chain_rule_case``),
    and with a fresh parameter in each of those angles. There every parameter is one rotation angle, so its
    derivative is the exact two-term shift of the existing ``expectation``; the chain rule over them in numpy must
    give the shared circuit's gradient within ``1e-12 max(1, |w|_1) sum |coef|``."""
    qc, spec, slots = gc.chain_rule_case(shared=True)
    qf, spec_f, slots_f = gc.chain_rule_case(shared=False)
    assert slots == slots_f
    pk, pf = ParametricKnit(VirtualCircuit(cut_circuit(qc, spec))), ParametricKnit(VirtualCircuit(cut_circuit(qf, spec_f)))
    masks, w = _masks_and_weights(5, 6, seed=2)
    S = np.array([[0.3, -1.1], [0.0, 0.0], [2.0, 0.7]])
    coef = np.array([[cs, ca] for cs, ca, _ in slots])  # [slots, 2]
    F = S @ coef.T + np.array([k for _, _, k in slots])[None, :]  # the fresh parameters' values [B, slots]
    n = len(slots)
    shifted = F[:, None, None, :] + (math.pi / 2) * np.array([1.0, -1.0])[None, None, :, None] * np.eye(n)[None, :, None, :]
    Es = pf.expectation(shifted.reshape(-1, n), masks, w).reshape(len(S), n, 2)
    ref = (0.5 * (Es[:, :, 0] - Es[:, :, 1])) @ coef
    val, grad = pk.value_and_gradient(S, masks, w)
    assert np.abs(val - pf.expectation(F, masks, w)).max() <= TOL * max(1.0, np.abs(w).sum())
    bound = TOL * max(1.0, float(np.abs(w).sum())) * np.abs(coef).sum(0)
    print(f"chain rule: max|grad - ref| = {np.abs(grad - ref).max(0)}, bound {bound}")
    assert (np.abs(grad - ref) <= bound[None, :]).all()
    assert np.abs(ref).max(0).min() > 1e-3


# ----------------------------------------------------------------------------- chunking
@pytest.mark.parametrize("case", ["packed", "cx_cut"])
def test_chunked_gradient_has_the_same_bits(T, monkeypatch, case):
    """``row_budget = 1`` byte: every chunk is one occurrence pair of one binding. Sweep rows and ``qk_rows_dot`` units
    do not depend on their neighbours and the host sums in occurrence order, so the cotangent route's gradient is
    the same bit for bit; so it is at a budget of three pairs. The reduce route goes through batched matrix
    products whose kernels depend on the batch: it is held to the per-entry tolerance."""
    if case == "packed":
        pk = ParametricKnit(VirtualCircuit(packed()[1]))
        chosen = None
    else:
        qc, pk = _split_knit(monkeypatch, case)
        chosen = _chosen(qc, case)
    masks, w = _masks_and_weights(pk._template.N, 4, seed=8)
    V = pc.bindings(pk.num_parameters, 3, seed=4)[1:]  # a random binding and all pi/2
    val, grad = pk.value_and_gradient(V, masks, w, parameters=chosen)
    unit = max(q.shape[1] * q.shape[2] * 8 for q in pk.sweep(V[:1]))
    for budget in (1, 6 * unit):
        val_c, grad_c = pk.value_and_gradient(V, masks, w, parameters=chosen, row_budget=budget)
        assert np.array_equal(val, val_c) and np.array_equal(grad, grad_c), budget
    vals, grads = pk.value_and_gradient(V, masks, parameters=chosen)
    vals_c, grads_c = pk.value_and_gradient(V, masks, parameters=chosen, row_budget=1)
    assert np.array_equal(vals, vals_c) and np.abs(grads - grads_c).max() <= TOL
    assert np.abs(grad).max() > 1e-3
    with pytest.raises(ValueError):
        pk.value_and_gradient(V, masks, w, row_budget=0)


# ----------------------------------------------------------------------------- edges
def test_gradient_edges(T):
    """A parameter subset in another order; a fragment without parameters; a parameter no mask can see; B = 0; no
    masks; unknown and repeated parameters."""
    qc, spec = gc.edge_case()
    t0, t1 = qc.parameters
    pk = ParametricKnit(VirtualCircuit(cut_circuit(qc, spec)))
    assert sorted(fs.prog.num_params > 0 for fs in pk.frags) == [False, True]
    masks, w = [0b0101, 0b0111, 0b0010, 0b0100], np.array([0.7, -0.4, 1.1, 0.3])  # clbit 3 (t1's qubit) in none
    V = np.array([[0.4, 1.3], [-2.0, 0.2]])
    val, grad = pk.value_and_gradient(V, masks, w)
    bound = TOL * max(1.0, float(np.abs(w).sum()))
    assert grad.shape == (2, 2) and np.abs(grad[:, 1]).max() <= bound and np.abs(grad[:, 0]).max() > 1e-3
    assert np.abs(pk.gradient(V, masks + [0b1000], np.append(w, 0.5))[:, 1]).max() > 1e-3  # and clbit 3 sees t1
    # t0 occurs twice (ry, and doubled inside u): against the central difference of expectation
    steps = np.array([V[0] + [gc.H_STEP, 0], V[0] - [gc.H_STEP, 0]])
    Es = pk.expectation(steps, masks, w)
    assert abs(grad[0, 0] - (Es[0] - Es[1]) / (2 * gc.H_STEP)) <= gc.difference_bound(3.0, float(np.abs(w).sum()))
    swapped = pk.gradient(V, masks, w, parameters=[t1, t0])
    assert np.array_equal(swapped, grad[:, ::-1])
    only = pk.gradient(V, masks, w, parameters=[t0])
    assert only.shape == (2, 1) and np.array_equal(only[:, 0], grad[:, 0])
    assert pk.gradient(V, masks, w, parameters=[]).shape == (2, 0)
    per_mask = pk.gradient(V, masks, parameters=[t0])
    assert per_mask.shape == (2, 4, 1) and np.abs(per_mask[:, :, 0] @ w - grad[:, 0]).max() <= bound
    v0, g0 = pk.value_and_gradient(V[:0], masks, w)
    assert v0.shape == (0,) and g0.shape == (0, 2)
    v0, g0 = pk.value_and_gradient(V[:0], masks)
    assert v0.shape == (0, 4) and g0.shape == (0, 4, 2)
    v0, g0 = pk.value_and_gradient(V, [])
    assert v0.shape == (2, 0) and g0.shape == (2, 0, 2)
    other = gc.edge_case()[0].parameters[0]
    for wrong in ([other], [t0, t0], [t0, t1, other]):
        with pytest.raises(ValueError):
            pk.value_and_gradient(V, masks, w, parameters=wrong)
    with pytest.raises(ValueError):
        pk.value_and_gradient(V, masks, w[:-1])


def test_gradient_of_an_uncut_circuit(T):
    """One fragment: the product over the other fragments is empty. ``t`` sits in an ``ry`` and, halved, in an ``rz``."""
    qc, spec = gc.one_fragment_case()
    pk = ParametricKnit(VirtualCircuit(cut_circuit(qc, spec)))
    assert len(pk.frags) == 1
    masks, w = [0b001, 0b110, 0b111, 0b010], np.array([0.5, -1.0, 0.25, 0.8])
    V = np.array([[0.9, -0.6]])
    val, grad = pk.value_and_gradient(V, masks, w)
    vals, grads = pk.value_and_gradient(V, masks)
    scale = float(np.abs(w).sum())
    assert np.array_equal(val, pk.expectation(V, masks, w)) and np.abs(grads.transpose(0, 2, 1) @ w - grad).max() <= TOL * scale
    for j, omega in enumerate((1.5, 1.0)):
        e = np.zeros(2)
        e[j] = gc.H_STEP
        Es = pk.expectation(np.array([V[0] + e, V[0] - e]), masks, w)
        assert abs(grad[0, j] - (Es[0] - Es[1]) / (2 * gc.H_STEP)) <= gc.difference_bound(omega, scale)
    assert np.abs(grad).max(0).min() > 1e-3


# ----------------------------------------------------------------------------- entry point
def test_gradient_entry_builds_one_knit_and_never_compiles_again(T, monkeypatch):
    """Two ``run_virtual_circuit_gradient`` calls on circuits built alike from different ``Parameter`` objects share one
    ``ParametricKnit``; the second reaches neither ``qk_module_compile`` nor ``qk_module_load``; the values are those of
    ``run_virtual_circuit_expectation(..., bindings=V, weights=w)``."""
    lib = _lib.lib()
    calls = []
    for fn in ("qk_module_compile", "qk_module_load"):
        real = getattr(lib, fn)
        monkeypatch.setattr(lib, fn, lambda *a, _real=real, _fn=fn: (calls.append(_fn), _real(*a))[1])
    monkeypatch.setenv("QKNIT_SWEEP_JIT", "1")
    monkeypatch.setenv("QKNIT_JIT_TILE_BITS", "12")  # a width no other test compiles these programs at
    parametric.clear_knit_cache()
    before = parametric.knits_built[0]
    masks, w = _masks_and_weights(27, 5, seed=6)
    results = []
    for call in range(2):
        qc, spec = pc.split_case("cx_cut")  # fresh parameters, same structure
        virt = VirtualCircuit(cut_circuit(qc, spec))
        V = pc.bindings(len(qc.parameters), 3, seed=30 + call)[1:]  # a random binding (per call) and all pi/2
        chosen = _chosen(qc, "cx_cut")
        if call == 1:
            built = len(calls)
        (val, grad), info = run_virtual_circuit_gradient(virt, masks, V, weights=w, parameters=chosen)
        assert val.shape == (2,) and grad.shape == (2, len(chosen)) and info.run_time > 0
        ref, _ = run_virtual_circuit_expectation(virt, masks, bindings=V, weights=w)
        assert np.array_equal(val, ref)
        results.append(grad)
    assert parametric.knits_built[0] == before + 1
    assert len(calls) == built
    assert not np.allclose(results[0], results[1])
    (vals, grads), _ = run_virtual_circuit_gradient(virt, masks, V, parameters=chosen[:2])
    assert vals.shape == (2, 5) and grads.shape == (2, 5, 2)
    assert np.abs(np.einsum("bmp,m->bp", grads, w) - results[1][:, :2]).max() <= TOL * max(1.0, np.abs(w).sum())
    with pytest.raises(ValueError):
        run_virtual_circuit_gradient(virt, masks, V, parameters=[pc.split_case("cx_cut")[0].parameters[0]])
    parametric.clear_knit_cache()
