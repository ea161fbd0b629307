"""The dict result chain (``qk_threshold_count``, ``qk_select_above``, ``qk_npd``, ``qk_npd_pairs``): the host
model of ``nearest_probability_distribution`` and the inputs shared by ``test_post.py`` (CPU) and
``test_gpu_post.py`` (GPU). No GPU and no torch here.

The chain under test: ``count_abs_above`` -> ``select_abs_above`` -> ``radix_sort_pairs`` by key ->
``radix_sort_pairs`` stably by value -> ``exclusive_sum`` -> ``sel_first_kept`` / ``sel_emit``.

Sizes. Each list names the constant of ``csrc/qknit_prim.hip`` / ``csrc/qknit_select.hip`` its members straddle
(the constants are restated here, not imported: a changed constant must show up as a reviewed change here).

* Radix sort (``rs_plan``): a wave of 64 lanes walks a chunk in steps of 64; ``RS_ELEMS_PER_WAVE = 8192`` gives
  ``W = ceil(n / 8192)`` single-wave workgroups, at most ``RS_MAX_WAVES = 4096``.
  1, 2: a single, partly filled step (and ``key_bits`` 0 / 1 on the dense path); 63, 64, 65: the 64-lane step
  (ragged, full, full + 1 lane); 8191, 8192, 8193: ``W`` 1 -> 2; 65,537: ``W = 9``, so the digit-major histogram
  holds 256 * 9 = 2304 ``uint32`` counts, a full scan tile of 2048 plus a ragged second block; 2^25 + 1: the
  first size past 4096 * 8192, where ``W`` is capped and chunks grow past 8192 (8256 elements, ``W = 4065``).
* Exclusive scan (``scan_plan``): ``SC_TILE = 256 * 8 = 2048`` per workgroup pass, at most ``SC_MAX_BLOCKS =
  1024`` workgroups. 2047, 2048, 2049: one ragged tile, one full tile, two workgroups; 2,097,152 = 1024 * 2048:
  1024 workgroups of exactly one tile, the last size without the carry; 2,097,153: the workgroup count is capped,
  chunks become two tiles (4096, 513 workgroups) and the second tile starts from ``carry``.
* ``sel_first_kept`` / ``sel_emit`` (``sel_grid``): at most 4096 workgroups of 256 threads, so 1,048,577 =
  4096 * 256 + 1 is the first size at which a thread takes a second grid-stride step.
"""
from __future__ import annotations

import numpy as np

SORT_SIZES = (1, 2, 63, 64, 65, 8191, 8192, 8193, 65537)
WAVE_CAP_SIZE = (1 << 25) + 1
SCAN_SIZES = (2047, 2048, 2049, 2097152, 2097153)
EMIT_SIZES = (1048577,)
PAIR_SIZES = tuple(sorted(set(SORT_SIZES + SCAN_SIZES + EMIT_SIZES)))
HOST_SIZES = tuple(n for n in PAIR_SIZES if n <= 65537)  # where the dict oracle is still quick

DENSE_ACC = 2.0 ** -11  # every planted m / 1024 (|m| >= 1) is kept, the zeros are not
# dense length -> kept entries; key_bits 0, 1, 2, 9, 10, 16, 17: 0, 1, 1, 2, 2, 2 and 3 digit passes of the key
# sort, the last digit partial (1 or 2 bits) or full (key_bits 16)
DENSE_CASES = ((1, 1), (2, 2), (3, 2), (257, 100), (1000, 300), (65536, 5000), (65537, 5000))
DENSE_WIDE = ((1 << 24) + 1, 5000)        # key_bits 25: 4 digit passes (slow: 128 MiB of zeros)
DENSE_FULL = ((1 << 22) + 1, 2097153)     # the scan carry, the emit stride and the select at scale

# the continuous cases (size, seed): seeds at which the host model decides more than 100 bands away from zero
# (test_post.py checks it; about half of all seeds sum below zero, and then nothing at all is kept)
CONT_PAIRS = (300001, 0)
CONT_DENSE = (65536, 3)

FEW_VALUES = np.array([-24.0, -5.0, 3.0, 17.0, 32.0]) / 1024.0
FAMILIES = ("dyadic", "few")


def npd_host(keys, vals):
    """``(keys_out, vals_out, k)``: the reference's ``nearest_probability_distribution`` of the dict
    ``{key: value}`` (keys unique). ``sorted(d.items(), key=value)`` over a dict built in key order is a stable sort
    by key, then by value; ``beta`` is the sequential sum of the dropped prefix, which ``np.cumsum`` is; once an
    entry is kept every later one is (values ascend, ``beta / n`` stops changing), so the dropped entries are a
    prefix ``i < k``."""
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    n = vals.size
    assert keys.shape == vals.shape == (n,)
    if n == 0:
        return keys.copy(), vals.copy(), 0
    o = np.argsort(keys, kind="stable")
    keys, vals = keys[o], vals[o]
    o = np.argsort(vals, kind="stable")
    keys, vals = keys[o], vals[o]
    S = np.concatenate(([0.0], np.cumsum(vals)[:-1]))
    left = (n - np.arange(n)).astype(np.float64)
    kept = np.flatnonzero(~(vals + S / left < 0))
    k = int(kept[0]) if kept.size else n
    if k == n:
        return keys[:0], vals[:0], n
    return keys[k:], vals[k:] + S[k] / float(n - k), k


def npd_band(keys, vals):
    """For values whose sums round: ``(k, band, margin)`` of the host model. ``band`` bounds the difference of
    the shift ``S_k / (n - k)`` between two summation orders of the dropped prefix, ``2 (k - 1) 2^-53
    sum_{i<k} |v_i| / (n - k)`` (each order is within ``(k - 1) 2^-53 sum |v_i|`` of the exact sum); ``margin`` is
    the smaller of ``|v_i + S_i / (n - i)|`` at ``i = k - 1`` and ``i = k``, the distance of the decision from
    zero."""
    vals = np.sort(np.asarray(vals, dtype=np.float64), kind="stable")
    n = vals.size
    _, _, k = npd_host(keys, vals)
    assert 0 < k < n
    S = np.concatenate(([0.0], np.cumsum(vals)[:-1]))
    band = 2.0 * (k - 1) * 2.0 ** -53 * float(np.abs(vals[:k]).sum()) / (n - k)
    margin = min(abs(vals[i] + S[i] / (n - i)) for i in (k - 1, k))
    return k, band, margin


# ----------------------------------------------------------------------------- values
def dyadic(rng, n, negative=0.3):
    """``m / 1024``, ``1 <= |m| <= 32``: many exact ties; a sum of up to 2^26 of them is a multiple of 2^-10 below
    2^21, exact in float64 in any order."""
    m = rng.integers(1, 33, n).astype(np.float64)
    m[rng.random(n) < negative] *= -1.0
    return m / 1024.0


def few_valued(rng, n):
    """Five distinct values of mixed sign (mantissas -24, -5, 3, 17, 32 times 2^-10): almost every entry ties."""
    return FEW_VALUES[rng.integers(0, FEW_VALUES.size, n)]


def continuous(rng, n):
    """``standard_normal * 1e-2`` with a fifth of the signs flipped: no ties, sums that round."""
    v = rng.standard_normal(n) * 1e-2
    v[rng.random(n) < 0.2] *= -1.0
    return v


def values(family, rng, n):
    return {"dyadic": dyadic, "few": few_valued, "continuous": continuous}[family](rng, n)


# ----------------------------------------------------------------------------- keys
def small_range_bits(n):
    """Keys below 2^20, as a knit of 20 clbits gives; the sizes above 2^20 need one or two bits more."""
    return max(20, int(n - 1).bit_length())


def keys_small(rng, n):
    """``n`` distinct keys below 2^20 (2^21, 2^22 where ``n`` does not fit) in random order: digit passes 3..7 of
    the key sort see zeros only."""
    return rng.permutation(1 << small_range_bits(n))[:n].astype(np.int64)


def keys_wide(rng, n):
    """``n`` distinct keys spread over 62 bits in random order: every digit pass of the key sort sees all digits."""
    k = np.unique(rng.integers(0, 2 ** 62, n + 64, dtype=np.int64))
    while k.size < n:  # (a repeat among 2^62 values: practically never)
        k = np.unique(np.concatenate((k, rng.integers(0, 2 ** 62, n, dtype=np.int64))))
    return rng.permutation(k)[:n]


def pairs_case(family, n, wide, seed=0):
    """The (keys, values) of one pairs case, seeded by its parameters."""
    rng = np.random.default_rng([FAMILIES.index(family) if family in FAMILIES else 2, n, int(wide), seed])
    vals = values(family, rng, n)
    return (keys_wide if wide else keys_small)(rng, n), vals


def dense_case(family, n, kept, seed=0):
    """A dense vector of length ``n`` holding ``kept`` values of the family at random places, zeros elsewhere;
    its (indices, values) in index order."""
    rng = np.random.default_rng([FAMILIES.index(family) if family in FAMILIES else 2, n, kept, seed])
    idx = np.sort(rng.permutation(n)[:kept]).astype(np.int64)
    vals = values(family, rng, kept)
    vec = np.zeros(n)
    vec[idx] = vals
    return vec, idx, vals


# ----------------------------------------------------------------------------- the threshold
def threshold_specials(acc):
    """Values on and next to the strict ``abs(v) > acc`` rule, and the ones with an ``abs`` of their own."""
    up, down = np.nextafter(acc, np.inf), np.nextafter(acc, 0.0)
    return np.array([acc, -acc, up, -up, down, -down, 0.0, -0.0, np.inf, -np.inf, np.nan])


def threshold_input(rng, n, acc, rotate=0, specials=None):
    """Noise below ``acc / 2`` with the special values planted at random places (all of them three times over
    where ``n`` has the room, else the first ``n`` from ``rotate`` on)."""
    sp = threshold_specials(acc) if specials is None else specials
    v = (rng.random(n) - 0.5) * acc
    where = rng.permutation(n)[: min(n, 3 * sp.size)]
    v[where] = sp[(np.arange(where.size) + rotate) % sp.size]
    return v
