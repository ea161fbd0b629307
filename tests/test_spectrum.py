"""The host side of the Walsh-Hadamard spectrum route: the numpy model of ``qk_wht_rows`` and the
vectorised mask handling (no device)."""
import random

import numpy as np
import pytest

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import observables as ob


def sign_matrix(m):
    """``S[z, x] = (-1)^popcount(x & z)``, written out."""
    idx = np.arange(1 << m)
    par = np.zeros((1 << m, 1 << m), dtype=np.int64)
    for b in range(m):
        par ^= ((idx[:, None] >> b) & 1) & ((idx[None, :] >> b) & 1)
    return 1 - 2 * par


@pytest.mark.parametrize("m", range(9))
def test_wht_host_is_the_explicit_sign_matrix_product(m):
    src = np.random.default_rng(m).integers(-8, 9, size=(3, (1 << m) + 2)).astype(np.float64)
    got = ob.wht_host(src, m)
    assert got.shape == (3, 1 << m) and got.dtype == np.float64
    np.testing.assert_array_equal(got, src[:, :1 << m] @ sign_matrix(m).T.astype(np.float64))
    one = ob.wht_host(src[0], m)  # a single row, and the source is left alone
    np.testing.assert_array_equal(one, got[0])
    assert np.array_equal(src, np.random.default_rng(m).integers(-8, 9, size=(3, (1 << m) + 2)).astype(np.float64))


@pytest.mark.parametrize("m", range(9))
def test_wht_host_is_an_involution_up_to_2_to_the_m(m):
    src = np.random.default_rng(100 + m).integers(-8, 9, size=(2, 1 << m)).astype(np.float64)
    np.testing.assert_array_equal(ob.wht_host(ob.wht_host(src, m), m), float(1 << m) * src)


def test_wht_host_keeps_the_dtype_and_refuses_short_rows():
    src = np.random.default_rng(5).standard_normal((2, 8))
    assert ob.wht_host(src.astype(np.longdouble), 3).dtype == np.longdouble
    assert ob.wht_host(src.astype(np.int64), 3).dtype == np.int64
    with pytest.raises(ValueError):
        ob.wht_host(src, 4)


def test_wht_pass_bits_cover_the_index_in_one_to_three_passes():
    for m in range(31):
        bits = ob.wht_pass_bits(m)
        assert sum(bits) == m and bits[0] == min(m, 13) and all(1 <= b <= 9 for b in bits[1:])
        assert len(bits) == (1 if m <= 13 else 2 if m <= 22 else 3)
    assert ob.wht_pass_bits(16) == [13, 3] and ob.wht_pass_bits(30) == [13, 9, 8]


def test_masks_array_agrees_with_parse_masks_on_lists_and_strings():
    n = 6
    rng = random.Random(1)
    ints = [rng.getrandbits(n) for _ in range(20)] + [0, (1 << n) - 1]
    strings = ["".join("Z" if z >> c & 1 else "I" for c in reversed(range(n))) for z in ints]
    for masks in (ints, strings, ints[:3] + strings[3:6], 5, "IIZIZZ", [], [np.int64(3)]):
        got = ob.masks_array(masks, n)
        assert got.dtype == np.int64 and got.ndim == 1
        assert got.tolist() == ob.parse_masks(masks, n)
    arr = np.array(ints)
    for a in (arr, arr.astype(np.int32), arr.astype(np.uint64), arr.astype(np.uint8)):
        got = ob.masks_array(a, n)
        assert got.dtype == np.int64 and got.tolist() == ints
    assert ob.masks_array(np.zeros(0, dtype=np.int64), n).shape == (0,)
    wide = np.array([(1 << 62) - 1, 1 << 61, 0], dtype=np.int64)
    assert ob.masks_array(wide, 62).tolist() == wide.tolist()
    with pytest.raises(ValueError, match="characters"):
        ob.masks_array(["ZZ"], n)
    with pytest.raises(ValueError, match="outside"):
        ob.masks_array([1 << n], n)


def test_masks_array_takes_a_torch_tensor():
    torch = pytest.importorskip("torch")
    got = ob.masks_array(torch.tensor([3, 0, 63], dtype=torch.int64), 6)
    assert got.dtype == np.int64 and got.tolist() == [3, 0, 63]
    with pytest.raises(ValueError, match="outside"):
        ob.masks_array(torch.tensor([3, 64], dtype=torch.int64), 6)


@pytest.mark.parametrize("bad", [np.array([1, -1, 2]), np.array([0, 64]), np.array([1 << 40], dtype=np.int64),
                                 np.array([1 << 63], dtype=np.uint64)])
def test_masks_array_rejects_masks_outside_the_clbits_in_an_array(bad):
    with pytest.raises(ValueError, match="outside"):
        ob.masks_array(bad, 6)


def test_masks_array_rejects_arrays_that_are_not_lists_of_integers():
    with pytest.raises(ValueError, match="integers"):
        ob.masks_array(np.array([1.0, 2.0]), 6)
    with pytest.raises(ValueError, match="one-dimensional"):
        ob.masks_array(np.zeros((2, 2), dtype=np.int64), 6)


def _wide_split():
    rng = random.Random(62)
    order = list(range(62))
    rng.shuffle(order)
    return [sorted(order[:30]), sorted(order[30:51]), [], sorted(order[51:])]


SPLITS = {
    "one_and_two": ([[0], [2, 4]], 5),
    "interleaved": ([[0, 2], [1, 3]], 4),
    "empty_entry": ([[1, 3, 4], [], [0, 5]], 7),
    "wide_62": (_wide_split(), 62),
}


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_split_masks_array_equals_split_mask(name):
    fcl, n = SPLITS[name]
    rng = random.Random(n)
    masks = [0, (1 << n) - 1] + [1 << c for c in range(n)] + [rng.getrandbits(n) for _ in range(200)]
    got = ob.split_masks_array(ob.masks_array(np.array(masks, dtype=np.int64), n), fcl)
    assert len(got) == len(fcl)
    want = [ob.split_mask(z, fcl) for z in masks]
    for f, loc in enumerate(got):
        assert loc.dtype == np.int64 and loc.shape == (len(masks),)
        assert loc.tolist() == [w[f] for w in want]
    for f, cl in enumerate(fcl):
        if not cl:
            assert not got[f].any()
