"""The host side of the per-clbit channels: the numpy model of ``qk_kron2_rows`` and the parsing of channel
specifications (no device)."""
import functools

import numpy as np
import pytest

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import observables as ob

EYE = np.eye(2)


def _mats(m, seed, lo=-1, hi=3):
    """Seeded integer matrices with entries in lo .. hi - 1, drawn per bit."""
    return np.random.default_rng(seed).integers(lo, hi, size=(m, 2, 2)).astype(np.float64)


@pytest.mark.parametrize("m", range(7))
def test_kron2_host_is_the_kronecker_product_highest_bit_first(m):
    mats = _mats(m, 10 + m)
    src = np.random.default_rng(m).integers(-8, 9, size=(3, (1 << m) + 2)).astype(np.float64)
    full = functools.reduce(np.kron, [mats[b] for b in reversed(range(m))], np.ones((1, 1)))
    got = ob.kron2_host(src, m, mats)
    assert got.shape == (3, 1 << m) and got.dtype == np.float64
    np.testing.assert_array_equal(got, src[:, :1 << m] @ full.T)
    np.testing.assert_array_equal(ob.kron2_host(src[0], m, mats), got[0])  # a single row
    assert np.array_equal(src, np.random.default_rng(m).integers(-8, 9, size=(3, (1 << m) + 2)).astype(np.float64))


def test_kron2_host_tells_a_matrix_from_its_transpose_and_the_bits_apart():
    up = np.array([[1.0, 1.0], [0.0, 0.0]])  # sums the bit out onto 0
    src = np.array([[1.0, 2.0, 3.0, 4.0]])
    np.testing.assert_array_equal(ob.kron2_host(src, 2, [up, EYE]), [[3.0, 0.0, 7.0, 0.0]])
    np.testing.assert_array_equal(ob.kron2_host(src, 2, [EYE, up]), [[4.0, 6.0, 0.0, 0.0]])
    np.testing.assert_array_equal(ob.kron2_host(src, 2, [up.T, EYE]), [[1.0, 1.0, 3.0, 3.0]])
    had = np.array([[1.0, 1.0], [1.0, -1.0]])
    wide = np.random.default_rng(0).integers(-8, 9, size=(2, 32))
    np.testing.assert_array_equal(ob.kron2_host(wide, 5, np.tile(had, (5, 1, 1))), ob.wht_host(wide, 5))


def test_kron2_host_keeps_the_dtype_and_checks_its_arguments():
    src = np.random.default_rng(5).standard_normal((2, 8))
    imats = _mats(3, 1).astype(np.int64)
    assert ob.kron2_host(src.astype(np.int64), 3, imats).dtype == np.int64
    assert ob.kron2_host(src, 3, imats).dtype == np.float64
    assert ob.kron2_host(src.astype(np.longdouble), 3, imats.astype(np.float64)).dtype == np.longdouble
    assert ob.kron2_host(src.astype(np.longdouble), 0, np.zeros((0, 2, 2))).dtype == np.longdouble
    np.testing.assert_array_equal(ob.kron2_host(src, 0, np.zeros((0, 2, 2))), src[:, :1])
    with pytest.raises(ValueError):
        ob.kron2_host(src, 4, _mats(4, 0))  # 16 columns are not there
    with pytest.raises(ValueError, match="shape"):
        ob.kron2_host(src, 3, _mats(2, 0))
    with pytest.raises(ValueError, match="shape"):
        ob.kron2_host(src, 3, np.zeros((3, 2, 3)))


def test_readout_matrix_is_column_stochastic_and_checks_its_range():
    A = ob.readout_matrix(0.02, 0.05)
    np.testing.assert_array_equal(A, [[0.98, 0.05], [0.02, 0.95]])
    np.testing.assert_array_equal(A.sum(axis=0), [1.0, 1.0])
    np.testing.assert_array_equal(ob.readout_matrix(0, 0), EYE)
    np.testing.assert_array_equal(ob.readout_matrix(1, 1), [[0.0, 1.0], [1.0, 0.0]])
    for e0, e1 in ((-0.1, 0.0), (0.0, 1.5), (float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ob.readout_matrix(e0, e1)
    ob.check_stochastic([A, EYE])
    for bad in ([[1.1, 0.0], [-0.1, 1.0]], [[0.9, 0.0], [0.0, 1.0]], 2 * EYE):
        with pytest.raises(ValueError, match="stochastic"):
            ob.check_stochastic([A, bad])


def test_invert_channels_inverts_every_matrix_and_refuses_a_singular_one():
    mats = np.stack([ob.readout_matrix(0.01 * (b + 1), 0.05 - 0.01 * b) for b in range(4)] + [np.array([[2.0, 1.0], [-1.0, 3.0]])])
    inv = ob.invert_channels(mats)
    assert inv.shape == mats.shape and inv.dtype == np.float64
    np.testing.assert_allclose(inv @ mats, np.tile(EYE, (5, 1, 1)), atol=4e-16, rtol=0)
    np.testing.assert_array_equal(ob.invert_channels(EYE), EYE)
    np.testing.assert_array_equal(ob.invert_channels([[0.0, 1.0], [1.0, 0.0]]), [[0.0, 1.0], [1.0, 0.0]])
    for singular in ([[1.0, 1.0], [0.0, 0.0]], ob.readout_matrix(0.5, 0.5), np.zeros((2, 2)),
                     [[np.inf, 0.0], [0.0, 1.0]], [[np.nan, 0.0], [0.0, 1.0]]):
        with pytest.raises(ValueError, match="determinant"):
            ob.invert_channels([EYE, singular])
    with pytest.raises(ValueError, match="2x2"):
        ob.invert_channels(np.zeros((3, 2)))


def test_bit_channels_parses_the_three_forms():
    A, B = ob.readout_matrix(0.02, 0.05), ob.readout_matrix(0.01, 0.03)
    measured = [0, 1, 3]  # clbit 2 is measured by no fragment
    one = ob.bit_channels(A, 4, measured)
    assert one.shape == (4, 2, 2) and one.dtype == np.float64
    np.testing.assert_array_equal(one, [A, A, EYE, A])
    by_dict = ob.bit_channels({3: B, 0: A}, 4, measured)
    np.testing.assert_array_equal(by_dict, [A, EYE, EYE, B])
    np.testing.assert_array_equal(ob.bit_channels({np.int64(1): B.tolist()}, 4, measured), [EYE, B, EYE, EYE])
    np.testing.assert_array_equal(ob.bit_channels({}, 4, measured), np.tile(EYE, (4, 1, 1)))
    arr = np.stack([A, B, EYE, B.T])
    got = ob.bit_channels(arr, 4, measured)
    np.testing.assert_array_equal(got, arr)
    got[0, 0, 0] = 7.0
    assert arr[0, 0, 0] == A[0, 0]  # a copy
    np.testing.assert_array_equal(ob.bit_channels({2: EYE}, 4, measured)[2], EYE)  # the identity is welcome anywhere
    np.testing.assert_array_equal(ob.bit_channels(arr.tolist(), 4, set(measured)), arr)
    # two clbits: [2, 2, 2] is an array of two matrices, [2, 2] one matrix for both
    np.testing.assert_array_equal(ob.bit_channels(np.stack([A, B]), 2, [0, 1]), [A, B])
    np.testing.assert_array_equal(ob.bit_channels(A, 2, [0, 1]), [A, A])
    assert ob.bit_channels(A, 0, []).shape == (0, 2, 2)


def test_bit_channels_raises_every_value_error():
    A = ob.readout_matrix(0.02, 0.05)
    measured = [0, 1, 3]
    with pytest.raises(ValueError, match="no fragment measures clbit 2"):
        ob.bit_channels({2: A}, 4, measured)
    with pytest.raises(ValueError, match="no fragment measures clbit 2"):
        ob.bit_channels(np.stack([A, A, A, A]), 4, measured)
    for c in (4, -1, "0", 1.0, True):
        with pytest.raises(ValueError, match="outside"):
            ob.bit_channels({c: A}, 4, measured)
    with pytest.raises(ValueError, match="2x2"):
        ob.bit_channels({0: np.zeros((2, 3))}, 4, measured)
    for shape in ((3, 2, 2), (4, 2), (4, 2, 3), (2,), (4, 4)):
        with pytest.raises(ValueError, match="shape"):
            ob.bit_channels(np.zeros(shape), 4, measured)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            ob.bit_channels({1: [[1.0, bad], [0.0, 1.0]]}, 4, measured)
        with pytest.raises(ValueError, match="finite"):
            ob.bit_channels([[1.0, 0.0], [bad, 1.0]], 4, measured)


def test_the_pass_layout_and_argument_checks_hold_on_the_host(tmp_path):
    """tools/kron_plan_check.hip walks csrc/kron_plan.h, the host half of ``qk_kron2_rows``, for m = 0..30: every index
    of every pass inside ``rows * ld``, every element touched once, every bit in one pass with its own matrix, every
    bad argument refused. No device is needed: nothing is launched."""
    import os
    import subprocess

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import build

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "kron_plan_check")
    cmd = [build.hipcc(), "-x", "hip", f"--offload-arch={build.ARCH}", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", os.path.join(build.HERE, "csrc"), os.path.join(root, "tools", "kron_plan_check.hip"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "kron_plan_check: ok" in res.stdout, res.stdout + res.stderr
