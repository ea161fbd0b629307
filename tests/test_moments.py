"""Second moments of the knit, host side: the longdouble models (``gram_host``, ``second_moment_host``), the
kernel's chunk decomposition (``gram_split``), the fragment pairing rule (``match_fragments``) and the argument
checks of the two C entries that need no device."""
import itertools

import numpy as np
import pytest

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import _lib
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import (gram_host, gram_split, match_fragments,
                                                                                  second_moment_host)


def test_gram_host_equals_the_integer_matmul():
    rng = np.random.default_rng(1)
    for RA, RB, m in ((1, 1, 0), (3, 5, 1), (17, 4, 5), (65, 16, 7)):
        A = rng.integers(-3, 4, size=(RA, (1 << m) + 2))
        B = rng.integers(-3, 4, size=(RB, (1 << m) + 5))
        want = A[:, :1 << m] @ B[:, :1 << m].T
        got = gram_host(A.astype(np.float64), B.astype(np.float64), m)
        assert got.dtype == np.longdouble and got.shape == (RA, RB)
        assert np.array_equal(got, want)
        sym = gram_host(A.astype(np.float64), None, m)
        assert np.array_equal(sym, A[:, :1 << m] @ A[:, :1 << m].T) and np.array_equal(sym, sym.T)
    assert np.array_equal(gram_host(np.ones((2, 4))), np.full((2, 2), 4.0))  # m defaults to every column
    with pytest.raises(ValueError):
        gram_host(np.ones((2, 3)), None, 2)


def _dense_knit(Xs):
    """R[x_0, x_1, ...] = sum_k prod_f X_f[k, x_f] as a dense longdouble array, one axis per fragment."""
    K = Xs[0].shape[0]
    R = 0
    for k in range(K):
        term = np.ones((), dtype=np.longdouble)
        for X in Xs:
            term = np.multiply.outer(term, X[k].astype(np.longdouble))
        R = R + term
    return R


@pytest.mark.parametrize("ms", [ms for F in (1, 2, 3) for ms in itertools.product((0, 1, 3), repeat=F)])
def test_second_moment_host_equals_the_dense_sum(ms):
    rng = np.random.default_rng(sum((i + 2) * (m + 1) for i, m in enumerate(ms)))
    K, K2 = 4, 7
    Xs = [rng.standard_normal((K, 1 << m)) for m in ms]
    Ys = [rng.standard_normal((K2, 1 << m)) for m in ms]
    R, R2 = _dense_knit(Xs), _dense_knit(Ys)
    scale = float((np.abs(_dense_knit([np.abs(X) for X in Xs])) * np.abs(_dense_knit([np.abs(Y) for Y in Ys]))).sum())
    tol = 64 * K * K2 * np.finfo(np.longdouble).eps * scale
    assert abs(second_moment_host(Xs, Ys) - (R * R2).sum()) <= tol
    assert abs(second_moment_host(Xs) - (R * R).sum()) <= tol
    with pytest.raises(ValueError):
        second_moment_host(Xs, Ys[:-1] if len(ms) > 1 else [])


def test_gram_split_tiles_the_outcomes_and_depends_on_the_shape_alone():
    for RA, RB, m in itertools.product((1, 3, 64, 65, 256, 1000, 5000), (1, 17, 64, 300), (0, 1, 5, 8, 9, 10, 13, 16, 20, 30)):
        sh = gram_split(RA, RB, m)
        assert sh == gram_split(RA, RB, m)
        assert sh["ba"] == -(-RA // 64) and sh["bb"] == -(-RB // 64)
        S, chunks = sh["split"], sh["chunks"]
        assert S >= 1 and S & (S - 1) == 0 and len(chunks) == S and sh["chunk"] * S == 1 << m
        assert chunks[0][0] == 0 and chunks[-1][1] == 1 << m
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(x1 - x0 == sh["chunk"] for x0, x1 in chunks)
        if S > 1:  # split only while the grid is short of 512 workgroups, and never below 256 outcomes a chunk
            assert sh["ba"] * sh["bb"] * S // 2 < 512 and sh["chunk"] >= 256 and S <= 256
            assert sh["workspace_bytes"] == sh["ba"] * sh["bb"] * S * 64 * 64 * 8
        else:
            assert sh["workspace_bytes"] == 0
        if sh["ba"] * sh["bb"] * S < 512:
            assert sh["chunk"] < 512 or S == 256  # nothing left to split
    assert gram_split(64, 64, 16)["split"] == 256 and gram_split(256, 256, 16)["split"] == 32
    assert gram_split(64, 64, 20)["split"] == 256 and gram_split(64, 128, 20)["split"] == 256
    assert gram_split(64, 64, 5)["split"] == 1 and gram_split(2048, 1024, 20)["split"] == 1
    # rows inside one block count do not move the split
    assert gram_split(1, 1, 13)["chunks"] == gram_split(64, 64, 13)["chunks"]
    for bad in ((0, 1, 3), (1, 0, 3), (1, 1, -1), (1, 1, 31)):
        with pytest.raises(ValueError):
            gram_split(*bad)


def test_gram_split_agrees_with_the_library_workspace_query():
    import ctypes

    lib = _lib.lib()
    for RA, RB, m in ((1, 1, 0), (64, 64, 16), (65, 3, 13), (256, 256, 16), (17, 17, 10), (300, 5000, 12)):
        need = ctypes.c_int64(-1)
        assert lib.qk_gram_rows_workspace_bytes(RA, RB, m, ctypes.byref(need)) == 0
        assert need.value == gram_split(RA, RB, m)["workspace_bytes"], (RA, RB, m)


def test_match_fragments_pairs_by_kept_clbit_sets():
    # a reordered but equal partition
    pairs, only_a, only_b = match_fragments([[0, 2], [1, 3], [4]], [[4], [1, 3], [0, 2]], range(5))
    assert pairs == [(0, 2, None), (1, 1, None), (2, 0, None)] and only_a == [] and only_b == []
    # local bit order differs: bit i of a's index sits at bit order[i] of b's
    pairs, _, _ = match_fragments([[0, 2, 5]], [[5, 0, 2]], [0, 2, 5])
    assert pairs == [(0, 0, [1, 2, 0])]
    # fragments without kept clbits stay unmatched and are allowed, in any number on either side
    pairs, only_a, only_b = match_fragments([[0, 1], [2], []], [[3], [0, 1]], [1, 0])
    assert pairs == [(0, 1, None)] and only_a == [1, 2] and only_b == [0]
    pairs, only_a, only_b = match_fragments([[0], [1]], [[2]], [])
    assert pairs == [] and only_a == [0, 1] and only_b == [0]
    # the same clbits cut differently
    a, b = [[0, 2], [1, 3]], [[0, 1], [2, 3]]
    with pytest.raises(ValueError, match=r"\[0\]"):
        match_fragments(a, b, [0, 1])
    with pytest.raises(ValueError, match="differently"):
        match_fragments(b, a, [0, 1])
    pairs, only_a, only_b = match_fragments(a, b, [0, 3])
    assert pairs == [(0, 0, None), (1, 1, None)] and only_a == [] and only_b == []
    assert match_fragments(a, b, [3, 0]) == (pairs, only_a, only_b)
    # a clbit only one side measures
    with pytest.raises(ValueError, match=r"\[4\]"):
        match_fragments([[0]], [[0], [4]], [0, 4])
    with pytest.raises(ValueError, match=r"\[4\]"):
        match_fragments([[0], [4]], [[0]], [0, 4])


def test_gram_entries_validate_arguments_without_a_device():
    import ctypes

    lib = _lib.lib()
    need = ctypes.c_int64(-7)
    assert lib.qk_gram_rows(None, 1, 1, 0, None, 1, None, 1, None, 1, None, 0) != 0
    assert lib.qk_gram_rows(None, 4, 4, 2, 8, 4, 8, 4, 1024, 4, None, 0) != 0  # a null context, whatever the rest
    assert lib.qk_gram_rows_workspace_bytes(1, 1, 0, None) != 0
    for RA, RB, m in ((0, 1, 3), (1, 0, 3), (-1, 1, 3), (1, 1, -1), (1, 1, 31), ((1 << 30) + 1, 1, 3)):
        assert lib.qk_gram_rows_workspace_bytes(RA, RB, m, ctypes.byref(need)) != 0, (RA, RB, m)
    assert need.value == -7
