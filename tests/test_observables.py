"""Marginals and Z-string expectation values without the 2^N output: the host side (no GPU).

The index mathematics of ``qk_reduce_bits`` (``observables.reduce_bits_host`` mirrors the kernel's
tile walk), the splitting of global clbit sets and masks over fragments, the ``QuasiDistr`` helpers
and argument validation."""
import math
import random

import numpy as np
import pytest

import circuits
import obs_cases
from oracle import dense, qvm

import hardwareawareoptimalquantumcircuitcuttingandknitting_amd.quasi_distr as pqd
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (QuasiDistr, VirtualCircuit, _lib, engine,
                                                                      observables as ob)

TOL = 1e-12


def brute_reduce(src, m, keep, flips):
    k = bin(keep).count("1")
    out = np.zeros((src.shape[0], len(flips) << k))
    for r in range(src.shape[0]):
        for j, f in enumerate(flips):
            for x in range(1 << m):
                out[r, (j << k) + ob.pext(x, keep)] += (-1.0) ** bin(x & f).count("1") * src[r, x]
    return out


def np_marginal(vec, clbits):
    """Marginal of a dense vector over 2^N keys onto ``clbits`` (bit i of the result = clbits[i])."""
    idx = np.arange(vec.size)
    y = np.zeros(vec.size, dtype=np.int64)
    for i, c in enumerate(clbits):
        y |= ((idx >> c) & 1) << i
    out = np.zeros(1 << len(clbits))
    np.add.at(out, y, vec)
    return out


def np_expectation(vec, mask):
    idx = np.arange(vec.size)
    par = np.zeros(vec.size, dtype=np.int64)
    for c in range(max(int(mask).bit_length(), 1)):
        if mask >> c & 1:
            par ^= (idx >> c) & 1
    return float(np.sum(np.where(par == 1, -vec, vec)))


# ----------------------------------------------------------------------------- index model
@pytest.mark.parametrize("m", range(6))
def test_reduce_bits_host_matches_brute_force_for_every_keep_mask(m):
    """Every keep_mask at m <= 5 (keep = 0, keep = all and m = 0 included), flips 0 / all dropped /
    random, with the kernel's tile width and with tiny tiles and split thresholds, so that the
    high/low split, the subset walk and the chunked second stage all carry real bits."""
    rng = np.random.default_rng(100 + m)
    for keep in range(1 << m):
        drop = ((1 << m) - 1) & ~keep
        flips = [0, drop] + [int(rng.integers(0, 1 << m)) & drop for _ in range(2)]
        src = rng.integers(-8, 9, size=(3, (1 << m) + 2)).astype(np.float64)
        ref = brute_reduce(src, m, keep, flips)
        for tile_bits, min_groups in ((10, 256), (2, 1), (2, 8), (1, 64), (3, 4)):
            got = ob.reduce_bits_host(src, m, keep, flips, tile_bits=tile_bits, min_groups=min_groups)
            np.testing.assert_array_equal(got, ref, err_msg=f"m={m} keep={keep:#x} tile={tile_bits} min={min_groups}")


def test_reduce_bits_shape_split_depends_on_shape_only():
    sh = ob.reduce_bits_shape(1, 16, 0)
    assert (sh["t"], sh["klo"], sh["khi"], sh["dhi"], sh["split"]) == (10, 0, 0, 6, 64)  # 64 tiles, all split
    sh = ob.reduce_bits_shape(1296, 16, 0)
    assert sh["split"] == 1 and sh["groups"] == 1296
    sh = ob.reduce_bits_shape(5, 13, 0x1FFF)  # copy: nothing dropped
    assert sh["split"] == 1 and sh["groups"] == 5 << 3 and sh["drop_lo"] == 0 and sh["drop_hi"] == 0
    sh = ob.reduce_bits_shape(3, 13, 0x3FF)  # low bits kept, high bits dropped
    assert (sh["klo"], sh["khi"], sh["dhi"], sh["split"]) == (10, 0, 3, 8)


def test_pext_pdep_roundtrip():
    rng = random.Random(5)
    for _ in range(200):
        mask = rng.getrandbits(20)
        v = rng.getrandbits(bin(mask).count("1")) if mask else 0
        assert ob.pext(ob.pdep(v, mask), mask) == v
        assert ob.pdep(v, mask) & ~mask == 0


# ----------------------------------------------------------------------------- mask splitting
def _fragment_clbits(cut):
    virt = VirtualCircuit(cut)
    frags = engine.prepare_fragments(virt, upload=False)
    return virt, [[] if fs.dropped else list(fs.prog.clbits) for fs in frags]


SPLIT_CASES = {
    "partial": lambda: circuits.partial_measure(),
    "many_traced": lambda: circuits.many_traced(),
    "gate_zoo_cut": lambda: circuits.gate_zoo_cut(4),
    "extra_clbit": obs_cases.extra_clbit,
    "interleaved": obs_cases.interleaved,
}


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_split_masks_and_clbits_over_fragments(case):
    _, cut = SPLIT_CASES[case]()
    virt, fcl = _fragment_clbits(cut)
    N = virt.circuit.num_clbits
    owner = {c: (f, i) for f, cl in enumerate(fcl) for i, c in enumerate(cl)}
    assert len(owner) == sum(len(cl) for cl in fcl)  # disjoint supports
    assert all(cl == sorted(cl) for cl in fcl)
    rng = random.Random(11)
    for _ in range(20):
        mask = rng.getrandbits(N)
        local = ob.split_mask(mask, fcl)
        for f, cl in enumerate(fcl):
            assert local[f] == ob.pext(mask, sum(1 << c for c in cl))
            assert local[f] >> len(cl) == 0
        back = 0
        for f, cl in enumerate(fcl):
            for i, c in enumerate(cl):
                if local[f] >> i & 1:
                    back |= 1 << c
        assert back == mask & sum(1 << c for c in owner)  # bits on clbits nobody measures are dropped
        clbits = rng.sample(range(N), rng.randint(0, N))
        keep, pos = ob.split_clbits(clbits, fcl)
        order = sorted(clbits)
        seen = []
        for f, cl in enumerate(fcl):
            kept = [c for i, c in enumerate(cl) if keep[f] >> i & 1]
            assert kept == [c for c in cl if c in clbits]
            assert [order[p] for p in pos[f]] == kept and pos[f] == sorted(pos[f])
            seen += kept
        assert sorted(seen) == [c for c in order if c in owner]


def test_split_cases_have_the_shapes_they_are_there_for():
    virt, fcl = _fragment_clbits(circuits.gate_zoo_cut(4)[1])
    frags = [f for f in virt.fragment_circuits if len(f)]
    assert [len(f) for f in frags] == [13, 14] and [len(cl) for cl in fcl] == [12, 13]  # wire-cut carrier
    virt, fcl = _fragment_clbits(obs_cases.extra_clbit()[1])
    assert fcl == [[0], [2, 4]] and virt.circuit.num_clbits == 5  # not contiguous, clbits 1 and 3 unwritten
    _, fcl = _fragment_clbits(obs_cases.interleaved()[1])
    assert fcl == [[0, 2], [1, 3]]
    _, fcl = _fragment_clbits(circuits.many_traced()[1])
    assert sorted(len(cl) for cl in fcl) == [3, 3]  # 11 of 14 qubits traced


def _oracle_rows(cut):
    """``(view, [(fragment, q_f, clbits_f)])``: the oracle's rows of every fragment, swept once."""
    view = qvm.CutView(cut)
    rows = []
    for qreg in view.qregs:
        frag = list(qreg)
        if not frag:
            continue
        q, cl = dense.fragment_q(view, frag)
        if q is not None:
            rows.append((tuple(frag), q, cl))
    return view, rows


def _host_knit_reduced(view, rows, keep, flips, positions):
    """The oracle rows reduced with the host model, knitted over the labels at ``positions``."""
    qs, cls = {}, {}
    for (frag, q, cl), kp, fl, p in zip(rows, keep, flips, positions):
        qs[frag] = ob.reduce_bits_host(q, len(cl), kp, [fl])
        cls[frag] = p
    return dense.dense_knit(view, qs, cls)


@pytest.mark.parametrize("case", ["partial", "extra_clbit", "interleaved", "cx_3cuts"])
def test_host_knit_of_reduced_rows_matches_reduced_dense_knit(case):
    """The identity the feature rests on, on the CPU: knitting the marginalised / sign-summed oracle
    rows equals the marginal / Z expectation of the dense knit. An unmeasured clbit has value 0 in a
    marginal and contributes +1 to an expectation."""
    make = SPLIT_CASES.get(case) or (lambda: circuits.two_fragment("cx", 3, 3, n_cuts=3))
    _, cut = make()
    full = dense.run_dense(cut)
    N = int(math.log2(full.size))
    view, rows = _oracle_rows(cut)
    fcl = [cl for _, _, cl in rows]
    rng = random.Random(3)
    sets = [list(range(N)), [0], [N - 1], rng.sample(range(N), min(3, N)), rng.sample(range(N), N - 1)]
    for clbits in sets:
        keep, pos = ob.split_clbits(clbits, fcl)
        got = _host_knit_reduced(view, rows, keep, [0] * len(fcl), pos)[:1 << len(clbits)]
        ref = np_marginal(full, sorted(clbits))
        np.testing.assert_allclose(got, ref, atol=TOL, rtol=0)
    for mask in [0, (1 << N) - 1, 1, 1 << (N - 1)] + [rng.getrandbits(N) for _ in range(8)]:
        got = _host_knit_reduced(view, rows, [0] * len(fcl), ob.split_mask(mask, fcl), [[] for _ in fcl])[0]
        assert abs(got - np_expectation(full, mask)) <= TOL
    if case == "extra_clbit":
        one = np_marginal(full, [1])
        assert one[1] == 0.0 and abs(one[0] - full.sum()) <= TOL  # nobody measures clbit 1: always 0
        assert abs(np_expectation(full, 0b01010) - full.sum()) <= TOL  # Z on clbits 1 and 3 only: factor +1
        _, fcl = _fragment_clbits(cut)
        assert ob.split_mask(0b01010, fcl) == [0] * len(fcl)
        assert ob.split_clbits([1, 3], fcl) == ([0] * len(fcl), [[] for _ in fcl])


# ----------------------------------------------------------------------------- QuasiDistr helpers
@pytest.mark.parametrize("case", ["partial", "extra_clbit", "interleaved", "cx_3cuts"])
def test_quasi_distr_marginal_and_expectation_match_numpy(case, monkeypatch):
    make = SPLIT_CASES.get(case) or (lambda: circuits.two_fragment("cx", 3, 3, n_cuts=3))
    full = dense.run_dense(make()[1])
    N = int(math.log2(full.size))
    monkeypatch.setattr(pqd, "ACCURACY", 0.0)  # every entry kept: the comparison is exact up to rounding
    qd = QuasiDistr({i: float(v) for i, v in enumerate(full)})
    rng = random.Random(9)
    for clbits in [[0], [N - 1, 0], list(range(N)), list(reversed(range(N))), rng.sample(range(N), 3)]:
        got = qd.marginal(clbits).to_dense(len(clbits))
        np.testing.assert_allclose(got, np_marginal(full, clbits), atol=TOL, rtol=0)
    for mask in [0, 1, (1 << N) - 1] + [rng.getrandbits(N) for _ in range(8)]:
        assert abs(qd.expectation(mask) - np_expectation(full, mask)) <= TOL
    assert qd.expectation("Z" + "I" * (N - 1)) == qd.expectation(1 << (N - 1))
    assert qd.expectation("I" * (N - 1) + "Z") == qd.expectation(1)


def test_quasi_distr_marginal_truncates_like_every_quasi_distr():
    qd = QuasiDistr({0: 0.5, 1: 0.5 - 4e-6, 2: 4e-5, 3: -3.8e-5})
    assert dict(qd.marginal([0])) == {0: 0.5 + 4e-5, 1: 0.5 - 4e-6 - 3.8e-5}
    assert set(qd.marginal([1])) == {0}  # 4e-5 - 3.8e-5 is below ACCURACY
    with pytest.raises(ValueError):
        qd.marginal([0, 0])
    with pytest.raises(ValueError):
        qd.expectation("ZX")


# ----------------------------------------------------------------------------- validation
def test_clbits_and_observables_are_validated():
    assert ob.check_clbits([3, 0, 2], 4) == [3, 0, 2]
    with pytest.raises(ValueError, match="duplicate"):
        ob.check_clbits([1, 2, 1], 4)
    with pytest.raises(ValueError, match="outside"):
        ob.check_clbits([0, 4], 4)
    with pytest.raises(ValueError, match="outside"):
        ob.check_clbits([-1], 4)
    assert ob.parse_masks(["ZIIZ", 5, "IIII"], 4) == [0b1001, 5, 0]
    assert ob.parse_masks("IZ", 2) == [1] and ob.parse_masks(3, 2) == [3]
    with pytest.raises(ValueError, match="characters"):
        ob.parse_masks(["ZIZ"], 4)
    with pytest.raises(ValueError, match="only I and Z"):
        ob.parse_masks(["ZXIZ"], 4)
    with pytest.raises(ValueError, match="outside"):
        ob.parse_masks([16], 4)
    assert ob.parse_masks([1 << 61], 62) == [1 << 61]  # Python ints: wide outputs


def test_reduce_bits_rejects_bad_masks_before_touching_a_device():
    with pytest.raises(ValueError, match="overlaps"):
        engine.reduce_bits(None, None, 4, 0b0011, [0b0010])
    with pytest.raises(ValueError, match="outside"):
        engine.reduce_bits(None, None, 4, 0b10000, [0])
    with pytest.raises(ValueError, match="outside"):
        engine.reduce_bits(None, None, 4, 0, [0b10000])
    with pytest.raises(ValueError, match="0..30"):
        engine.reduce_bits(None, None, 31, 0, [0])
    with pytest.raises(ValueError, match="at least one"):
        engine.reduce_bits(None, None, 4, 0, [])
    overlapping_rows = engine.torch().ones(32, dtype=engine.torch().float64).as_strided((2, 16), (8, 1))
    with pytest.raises(ValueError, match="row stride"):
        engine.reduce_bits(None, overlapping_rows, 4, 0, [0])
    with pytest.raises(ValueError):
        ob.reduce_bits_host(np.zeros((1, 16)), 4, 0b0011, [0b0010])


def test_reduce_bits_entry_validates_arguments_without_device():
    """The C entry rejects a null context before touching the GPU; its workspace query is pure host
    code and checks its own arguments."""
    import ctypes

    lib = _lib.lib()
    masks = (ctypes.c_uint64 * 1)(0)
    assert lib.qk_reduce_bits(None, 1, 4, None, 16, 0, 1, masks, None, 1, None, 0) != 0
    assert lib.qk_last_error(None) == b"null context"
    need = ctypes.c_int64(-1)
    assert lib.qk_reduce_bits_workspace_bytes(1, 16, 0, 1, ctypes.byref(need)) == 0
    assert need.value == 64 * 8  # 64 tiles split over 64 workgroups, one partial each
    assert lib.qk_reduce_bits_workspace_bytes(1296, 16, 0, 1024, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.qk_reduce_bits_workspace_bytes(3, 13, 0x3FF, 40, ctypes.byref(need)) == 0
    assert need.value == 3 * 8 * 16 * 1024 * 8  # groups x chunks x one batch of masks x 2^klo doubles
    assert lib.qk_reduce_bits_workspace_bytes(1, 31, 0, 1, ctypes.byref(need)) != 0
    assert lib.qk_reduce_bits_workspace_bytes(1, -1, 0, 1, ctypes.byref(need)) != 0
    assert lib.qk_reduce_bits_workspace_bytes(1, 4, 16, 1, ctypes.byref(need)) != 0
    assert lib.qk_reduce_bits_workspace_bytes(1, 4, 0, 0, ctypes.byref(need)) != 0
    assert lib.qk_reduce_bits_workspace_bytes(1, 4, 0, 1, None) != 0
    assert engine.REDUCE_BITS_BATCH == 16


def test_entry_points_refuse_what_is_out_of_scope():
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (run_virtual_circuit_expectation,
                                                                          run_virtual_circuit_marginal)

    virt = VirtualCircuit(circuits.two_fragment("cx")[1])
    with pytest.raises(ValueError, match="one GPU"):
        run_virtual_circuit_marginal(virt, [0], group="WORLD")
    with pytest.raises(ValueError, match="exact"):
        run_virtual_circuit_marginal(virt, [0], sample=True)
    with pytest.raises(ValueError, match="one GPU"):
        run_virtual_circuit_expectation(virt, [1], group="WORLD")
    with pytest.raises(ValueError, match="exact"):
        run_virtual_circuit_expectation(virt, [1], sample=True)
