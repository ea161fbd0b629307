"""Shots from the knit without the 2^N distribution, host side: the chain sampler as a numpy model
(shared with tests/test_gpu_shots.py), the key deposit, argument handling and the C entries' checks
that need no device."""
import ctypes
import types

import numpy as np
import pytest

import circuits
from oracle.sampling import uniforms

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, _lib, observables as ob
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer


# ----------------------------------------------------------------------------- numpy models
def np_sample_rows(X, C, draw_off, u):
    """numpy model of qk_sample_rows: ``(x, w, row_total, cdf, raw)`` with ``raw = C @ X``,
    ``cdf = cumsum(max(raw, 0))`` per row and, per draw, the first x with ``cdf > u * total``."""
    raw = C @ X
    w = np.maximum(raw, 0.0)
    cdf = np.cumsum(w, axis=1)
    x = np.full(len(u), -1, dtype=np.int64)
    for r in range(C.shape[0]):
        d = slice(draw_off[r], draw_off[r + 1])
        if cdf[r, -1] > 0:
            x[d] = np.minimum(np.searchsorted(cdf[r], u[d] * cdf[r, -1], side="right"), X.shape[1] - 1)
    return x, w, cdf[:, -1], cdf, raw


def np_chain_sample(Xs, us):
    """The chain of the issue on the host. ``Xs``: per fragment ``[K, 2^m_f]`` with the coefficients
    folded in; ``us[f]``: the uniforms ``[shots]`` of step f. Returns the outcomes ``[F, shots]``."""
    sums = [X.sum(axis=1) for X in Xs]
    shots, K = len(us[0]), Xs[0].shape[0]
    c = np.ones((shots, K))
    out = []
    for f, X in enumerate(Xs):
        tail = np.ones(K)
        for s in sums[f + 1:]:
            tail = tail * s
        w = np.maximum((c * tail) @ X, 0.0)
        cdf = np.cumsum(w, axis=1)
        x = (cdf > (us[f] * cdf[:, -1])[:, None]).argmax(axis=1)
        c = c * X[:, x].T
        out.append(x)
    return np.array(out)


def test_chain_sampler_agrees_with_inverse_cdf_sampling_of_the_dense_product():
    """R[x_0, x_1, x_2] = sum_k prod_f X_f[k][x_f] with fragment 0 in the highest bits: one inverse-CDF
    draw of R with u fixes x_0 as the chain's first step does with the same u, and the position of the
    target inside the chosen block is the uniform of the next step. Feeding the chain those uniforms
    must give the dense draw, outcome by outcome."""
    rng = np.random.default_rng(5)
    K, ms, shots = 3, (3, 2, 4), 4000
    Xs = [rng.uniform(1.0, 1.5, size=(K, 1 << m)) for m in ms]
    Xs[0][K - 1] *= -0.1  # a negative term: R stays positive (|term| < 0.1 * 1.5^3 / 1 of a positive one)
    R = np.einsum("ka,kb,kc->abc", *Xs)
    assert R.min() > 0
    u0 = uniforms(11, 0, shots)
    cdf = np.cumsum(R.reshape(-1))
    target = u0 * cdf[-1]
    key = np.searchsorted(cdf, target, side="right")
    want = np.array(np.unravel_index(key, R.shape))
    # residual uniforms: where the target lies inside the block of the outcomes drawn so far
    us = [u0]
    for f in (1, 2):
        block = R.reshape(int(np.prod(R.shape[:f])), -1)
        start = np.concatenate([[0.0], np.cumsum(block.sum(axis=1))[:-1]])
        idx = np.ravel_multi_index(tuple(want[:f]), R.shape[:f])
        us.append((target - start[idx]) / block.sum(axis=1)[idx])
        assert np.all((us[-1] >= 0) & (us[-1] < 1))
    got = np_chain_sample(Xs, us)
    assert np.array_equal(got, want)
    # and its outcome frequencies follow R (5 sigma per outcome of fragment 0)
    freq = np.bincount(got[0], minlength=8) / shots
    p0 = R.sum(axis=(1, 2)) / R.sum()
    assert np.all(np.abs(freq - p0) <= 5 * np.sqrt(p0 * (1 - p0) / shots))


def test_np_sample_rows_model_is_an_inverse_cdf():
    X = np.array([[1.0, 0.0, 2.0, 1.0], [0.0, 1.0, -5.0, 0.0]])
    C = np.array([[1.0, 1.0], [0.0, 0.0], [2.0, 0.0]])
    off = np.array([0, 3, 4, 6])
    u = np.array([0.0, 0.5, 1 - 2.0 ** -53, 0.3, 0.49, 0.5])
    x, w, total, _, _ = np_sample_rows(X, C, off, u)
    assert w[0].tolist() == [1.0, 1.0, 0.0, 1.0] and total.tolist() == [3.0, 0.0, 8.0]
    assert x.tolist() == [0, 1, 3, -1, 2, 2]


# ----------------------------------------------------------------------------- keys
def test_key_deposit_of_interleaved_fragment_clbits():
    fcl = [[0, 2], [1, 3]]
    keep, where = ob.key_positions([0, 1, 2, 3], fcl)
    assert keep == [0b11, 0b11] and where == [[0, 2], [1, 3]]
    x0, x1 = np.array([0b01, 0b10, 0b11]), np.array([0b11, 0b01, 0b10])
    keys = ob.deposit_bits(ob.deposit_bits(np.zeros(3, dtype=np.int64), x0, where[0]), x1, where[1])
    assert keys.tolist() == [0b1011, 0b0110, 0b1101]
    # a subset in another order: bit i of the key is clbits[i]; fragment bits that are not kept vanish
    keep, where = ob.key_positions([3, 0, 2], fcl)
    assert keep == [0b11, 0b10] and where == [[1, 2], [0]]
    keys = ob.deposit_bits(ob.deposit_bits(np.zeros(3, dtype=np.int64), x0, where[0]), x1 >> 1, where[1])
    assert keys.tolist() == [0b011, 0b100, 0b111]
    # a clbit nobody measures has no position: it stays 0
    keep, where = ob.key_positions([0, 1, 2, 3, 4], [[0], [2, 4]])
    assert keep == [1, 3] and where == [[0], [2, 4]]
    # torch tensors take the same path
    import torch

    t = ob.deposit_bits(torch.zeros(3, dtype=torch.int64), torch.from_numpy(x0), [0, 2])
    assert t.tolist() == [0b001, 0b100, 0b101]


def test_sample_checks_clbits_and_shots_before_touching_the_device():
    red = object.__new__(KnitReducer)
    red.N, red.device, red.ctx = 4, 0, types.SimpleNamespace(bind_stream=lambda: None)
    with pytest.raises(ValueError, match="duplicate"):
        red.sample(10, 0, [0, 1, 0])
    with pytest.raises(ValueError, match="outside"):
        red.sample(10, 0, [4])
    with pytest.raises(ValueError, match="negative"):
        red.sample(-1)


def test_shots_entry_point_refuses_what_is_out_of_scope():
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import run_virtual_circuit_shots

    virt = VirtualCircuit(circuits.two_fragment("cx")[1])
    with pytest.raises(ValueError, match="one GPU"):
        run_virtual_circuit_shots(virt, 10, group="WORLD")
    with pytest.raises(ValueError, match="exact"):
        run_virtual_circuit_shots(virt, 10, sample=True)


# ----------------------------------------------------------------------------- C entries, no device
def test_sample_rows_workspace_is_one_double_per_row_and_tile():
    lib = _lib.lib()
    need = ctypes.c_int64(-1)
    for rows, m, want in ((1, 0, 8), (5, 10, 40), (5, 11, 80), (3, 13, 3 * 8 * 8), (20000, 18, 20000 * 256 * 8),
                          (0, 4, 0), (2, 30, 2 * (1 << 20) * 8)):
        assert lib.qk_sample_rows_workspace_bytes(rows, m, ctypes.byref(need)) == 0
        assert need.value == want, (rows, m)
    assert lib.qk_sample_rows_workspace_bytes(1, 31, ctypes.byref(need)) != 0
    assert lib.qk_sample_rows_workspace_bytes(1, -1, ctypes.byref(need)) != 0
    assert lib.qk_sample_rows_workspace_bytes(-1, 4, ctypes.byref(need)) != 0
    assert lib.qk_sample_rows_workspace_bytes(1, 4, None) != 0


def test_shots_entries_reject_a_null_context():
    lib = _lib.lib()
    assert lib.qk_uniforms(None, 0, 0, 0, 4, None) != 0
    assert lib.qk_sample_rows(None, 1, 0, None, 1, 1, None, 1, None, 0, None, None, None, None, None, 0) != 0
