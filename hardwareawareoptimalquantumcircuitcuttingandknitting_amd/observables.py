"""Marginals and Pauli-Z string expectation values of a knit, without its 2^N output.

The knit is ``R[key] = sum_k prod_f X_f[k][x_f]`` with ``X_f = W_f^T q_f`` and the
fragments' clbit supports are disjoint, so a reduction of ``R`` that factorises over bits
factorises over fragments::

    marginal onto S:   R_S[y] = sum_k prod_f X_f^S[k][y_f],  X_f^S[k][y_f] = sum_{x: pext(x, S_f) = y_f} X_f[k][x]
    Z string on Z:     <Z>    = sum_k prod_f ( sum_x (-1)^popcount(x & Z_f) X_f[k][x] )

Both reductions are linear, so they are applied to the swept rows ``q_f`` (``qk_reduce_bits``,
csrc/qknit_obs.hip) before the transform ``W_f``; everything after works on narrow operands. A
:class:`KnitReducer` sweeps once and answers any number of such questions; nothing on this path
allocates or indexes ``2^N``, so the output width is bounded by the int64 keys (N <= 62), not by
memory.

Many Z strings at once: a fragment's factor of every string is one entry of its rows' Walsh-Hadamard
transform, ``H_f[k][z] = sum_x (-1)^popcount(x & z) X_f[k][x]`` (``qk_wht_rows``, csrc/qknit_wht.hip), so
``<Z_mask> = sum_k prod_f H_f[k][pext(mask, clbits_f)]``: :meth:`KnitReducer.z_spectrum` transforms once,
then any number of masks is a gather (``expectation(method="spectrum")``, ``expectation_sum``,
``correlations``).

The knit at chosen keys is a gather as well: with each operand transposed once (``qk_transpose_rows``,
csrc/qknit_lookup.hip) the factors a key takes from a fragment are one contiguous row, and ``qk_knit_at``
sums their products over the terms: :meth:`KnitReducer.probabilities`, ``linear_xeb``,
``fidelity_to_counts``, and ``expectation(method="fused")`` on the transposed spectrum.

Second moments factorise too: ``sum_x R[x] R'[x] = sum_{k,k'} prod_f (X_f X'_f^T)[k][k']``, and
``X_f X'_f^T = W_f^T (q_f q'_f^T) W'_f`` needs one tall product per fragment, the cross-Gram of the swept rows
(``qk_gram_rows``, csrc/qknit_moments.hip): :meth:`KnitReducer.overlap`, ``collision_probability``,
``renyi2_entropy``, ``ideal_xeb``, ``l2_distance``, ``mutual_information2``.

A linear map that factorises over the clbits, ``R'[y] = sum_x prod_c A_c[y_c][x_c] R[x]`` with a real 2x2 matrix
per clbit (readout error, its inverse, a flip, a bit summed out), acts on the column index of each fragment's
swept rows and commutes with ``W_f``: :meth:`KnitReducer.with_channels` applies it to the rows once
(``qk_kron2_rows``, csrc/qknit_kron.hip) and returns a reducer whose every answer is that of ``R'``
(``with_readout_error``, ``with_readout_mitigation``).

It builds on the direct path (``engine.prepare_fragments`` / ``sweep_fragment`` / ``knit_operands``
/ ``fragment_operands`` / ``contract``, as ``run._direct_dense``), not on the cached
``KnitPipeline``: the pipeline's row pruning rests on a per-entry bound on ``R`` and a marginal sums
up to ``2^(N-k)`` entries, so that bound does not carry over.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import engine
from .backend import MI355XBackend
from .knit_plan import LabelSpace

MAX_CLBITS = 62  # keys are int64
SPECTRUM_GATHER_CHUNK = 1 << 20  # masks per gather of the spectrum route: [terms, chunk] doubles per fragment


# ----------------------------------------------------------------------------- host index model
def pext(x: int, mask: int) -> int:
    """The bits of ``x`` at the set positions of ``mask``, packed in ascending order."""
    out, i = 0, 0
    while mask:
        low = mask & -mask
        if x & low:
            out |= 1 << i
        i += 1
        mask ^= low
    return out


def pdep(v: int, mask: int) -> int:
    """The low bits of ``v`` spread to the set positions of ``mask``, ascending."""
    out = 0
    while mask:
        low = mask & -mask
        if v & 1:
            out |= low
        v >>= 1
        mask ^= low
    return out


def popcount(x) -> np.ndarray:
    """The number of set bits of every entry of a non-negative integer array (a Python int has ``bit_count``)."""
    x = np.asarray(x, dtype=np.int64)
    n = np.zeros_like(x)
    while np.any(x):
        n += x & 1
        x = x >> 1
    return n


def reduce_bits_shape(rows: int, m: int, keep_mask: int, tile_bits: int = 10, min_groups: int = 256) -> dict:
    """The tile decomposition ``qk_reduce_bits`` uses for a shape (qknit_obs.hip: rb_make_shape)."""
    t = min(m, tile_bits)
    lo, hi = (1 << t) - 1, (1 << (m - t)) - 1
    keep_lo, drop_lo = keep_mask & lo, ~keep_mask & lo
    keep_hi, drop_hi = (keep_mask >> t) & hi, ~(keep_mask >> t) & hi
    klo, khi, dhi = keep_lo.bit_count(), keep_hi.bit_count(), drop_hi.bit_count()
    groups, split = rows << khi, 1
    while groups * split < min_groups and split < (1 << dhi):
        split *= 2
    return dict(t=t, keep_lo=keep_lo, drop_lo=drop_lo, keep_hi=keep_hi, drop_hi=drop_hi, klo=klo, khi=khi, dhi=dhi,
                groups=groups, split=split)


def reduce_bits_host(src: np.ndarray, m: int, keep_mask: int, flips, tile_bits: int = 10,
                     min_groups: int = 256) -> np.ndarray:
    """numpy model of ``qk_reduce_bits`` with the kernel's index mathematics: the row cut into tiles
    of ``2^min(m, tile_bits)`` values, a (row, kept high bits) group walking the subsets of the
    dropped high bits in ascending order (``sub = ((sub | ~drop) + 1) & drop``) in ``split`` chunks,
    the sign split into a per-tile and an in-tile parity, the in-tile sum onto ``pext(xl, keep_lo)``
    and the chunks' partials added in ascending order. ``out[r, j * 2^k + y]``."""
    src = np.asarray(src, dtype=np.float64)
    flips = [int(f) for f in flips]
    if keep_mask >> m or any(f >> m or f & keep_mask for f in flips):
        raise ValueError("masks outside the m bits, or a flip mask that overlaps keep_mask")
    sh = reduce_bits_shape(src.shape[0], m, keep_mask, tile_bits, min_groups)
    t, klo, khi, dhi = sh["t"], sh["klo"], sh["khi"], sh["dhi"]
    T, k = 1 << t, klo + khi
    xl = np.arange(T)
    yl = np.array([pext(int(x), sh["keep_lo"]) for x in xl])
    out = np.zeros((src.shape[0], len(flips) << k))
    chunk = (1 << dhi) // sh["split"]
    for r in range(src.shape[0]):
        for yhi in range(1 << khi):
            base_hi = pdep(yhi, sh["keep_hi"])
            for j, f in enumerate(flips):
                lane = popcount(xl & f) & 1
                total = None
                for s in range(sh["split"]):
                    sub = pdep(s * chunk, sh["drop_hi"])
                    part = np.zeros(1 << klo)
                    for _ in range(chunk):
                        tile = base_hi | sub
                        neg = lane ^ (((tile << t) & f).bit_count() & 1)
                        v = src[r, tile * T:(tile + 1) * T]
                        np.add.at(part, yl, np.where(neg == 1, -v, v))
                        sub = ((sub | ~sh["drop_hi"]) + 1) & sh["drop_hi"]
                    total = part if total is None else total + part
                o = (j << k) + (yhi << klo)
                out[r, o:o + (1 << klo)] = total
    return out


# ----------------------------------------------------------------------------- argument handling
def check_clbits(clbits, n_clbits: int) -> list:
    """``clbits`` as a list of distinct ints in ``0..n_clbits-1`` (any order), else ``ValueError``."""
    out = [int(c) for c in clbits]
    if len(set(out)) != len(out):
        raise ValueError(f"duplicate clbits in {out}")
    for c in out:
        if not 0 <= c < n_clbits:
            raise ValueError(f"clbit {c} outside 0..{n_clbits - 1}")
    return out


def check_not_negative(name: str, value, kind=int):
    """``kind(value)`` (``int`` for a count, ``float`` for a bound), else ``ValueError`` when it is negative or no
    number."""
    v = kind(value)
    if not v >= 0:
        raise ValueError(f"{name} must not be negative, not {v}")
    return v


def parse_masks(masks, n_clbits: int) -> list:
    """Z-string observables as int masks over clbits ``0..n_clbits-1``. Each is a Python int (bit
    ``i`` = Z on clbit ``i``) or a string of ``n_clbits`` characters from ``I`` / ``Z`` whose rightmost
    character is clbit 0. A single int or string counts as a list of one."""
    if isinstance(masks, (str, int, np.integer)):
        masks = [masks]
    out = []
    for z in masks:
        if isinstance(z, str):
            if len(z) != n_clbits:
                raise ValueError(f"observable {z!r} has {len(z)} characters for {n_clbits} clbits")
            if set(z.upper()) - set("IZ"):
                raise ValueError(f"observable {z!r}: only I and Z")
            z = sum(1 << i for i, ch in enumerate(reversed(z.upper())) if ch == "Z")
        z = int(z)
        if z < 0 or z >> n_clbits:
            raise ValueError(f"mask {z:#x} outside the {n_clbits} clbits")
        out.append(z)
    return out


def split_clbits(clbits: list, fragment_clbits: list) -> tuple:
    """Split a set of global clbits over the fragments. ``fragment_clbits[f]``: the ascending global
    clbits of fragment f's local outcome bits (local bit i = its i-th ascending clbit; ``[]`` for a
    dropped fragment). Returns ``(keep, positions)``: per fragment the local ``keep_mask`` and, for
    its kept bits in ascending order, their positions in the ascending list of ``clbits`` (the
    re-indexed clbits of the narrow contraction). A clbit no fragment measures appears nowhere: its
    bit of the result stays 0."""
    rank = {c: i for i, c in enumerate(sorted(clbits))}
    keep, positions = [], []
    for fcl in fragment_clbits:
        keep.append(sum(1 << i for i, c in enumerate(fcl) if c in rank))
        positions.append([rank[c] for c in fcl if c in rank])
    return keep, positions


def split_mask(mask: int, fragment_clbits: list) -> list:
    """Per fragment the local mask ``pext(mask, its clbits)``. A bit on a clbit that no fragment
    measures is dropped: that clbit is always 0, its Z contributes +1."""
    return [sum(1 << i for i, c in enumerate(fcl) if mask >> c & 1) for fcl in fragment_clbits]


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _check_range(what: str, lo: int, hi: int, n_bits: int) -> None:
    """``ValueError`` unless ``lo`` and ``hi``, the least and the greatest of a batch, lie in ``0 .. 2^n_bits - 1``."""
    if lo < 0 or hi >> n_bits:
        raise ValueError(f"{what} {hi if lo >= 0 else lo:#x} outside 0..2^{n_bits} - 1")


def _int64_vector(what: str, values: np.ndarray, n_bits: int) -> np.ndarray:
    """An integer numpy array of at most one dimension as a contiguous ``int64`` ``[M]``, every entry in
    ``0 .. 2^n_bits - 1`` (checked before the conversion: a uint64 at or above 2^63 is out of range)."""
    if values.dtype.kind not in "iu":
        raise ValueError(f"a {what} array must hold integers, not {values.dtype}")
    if values.ndim > 1:
        raise ValueError(f"a {what} array must be one-dimensional, not {values.shape}")
    if values.size:
        _check_range(what, int(values.min()), int(values.max()), n_bits)
    return np.ascontiguousarray(values.reshape(-1), dtype=np.int64)


def masks_array(masks, n_clbits: int) -> np.ndarray:
    """Z-string observables as an ``int64`` array ``[M]`` of masks over clbits ``0..n_clbits-1``. An
    integer numpy array or a torch int64 tensor (of any number of masks) is checked vectorised;
    anything else (ints, ``'IZ'`` strings, lists of them) goes through :func:`parse_masks`."""
    if _is_tensor(masks):
        masks = masks.detach().cpu().numpy()
    if isinstance(masks, np.ndarray):
        return _int64_vector("mask", masks, n_clbits)
    return np.array(parse_masks(masks, n_clbits), dtype=np.int64).reshape(-1)


def split_masks_array(zs: np.ndarray, fragment_clbits: list) -> list:
    """:func:`split_mask` of every mask of an int64 array at once: per fragment the ``int64`` array
    ``[M]`` of local masks (a loop over its clbits, vectorised over the masks)."""
    zs = np.asarray(zs, dtype=np.int64)
    out = []
    for fcl in fragment_clbits:
        loc = np.zeros(zs.shape, dtype=np.int64)
        for i, c in enumerate(fcl):
            loc |= ((zs >> np.int64(c)) & 1) << np.int64(i)
        out.append(loc)
    return out


def wht_pass_bits(m: int, tile_bits: int = 13, later_bits: int = 9) -> list:
    """The index bits each pass of ``qk_wht_rows`` transforms (qknit_wht.hip: wh_schedule): the low
    ``min(m, 13)`` in pass 0, the rest spread evenly over ``ceil((m - 13) / 9)`` strided passes."""
    t0 = min(m, tile_bits)
    rem = m - t0
    later = -(-rem // later_bits)
    return [t0] + [rem // later + (1 if i < rem % later else 0) for i in range(later)]


def wht_host(src, m: int) -> np.ndarray:
    """numpy model of ``qk_wht_rows``: ``out[..., z] = sum_{x < 2^m} (-1)^popcount(x & z) src[..., x]``,
    unnormalised, by ``m`` levels of butterflies ``(a, b) -> (a + b, a - b)`` with ``a`` the element whose
    bit is clear, lowest bit first, in the dtype of ``src`` (the kernel takes the bits in another fixed
    order: equal for exactly representable sums, equal to rounding otherwise)."""
    src = np.asarray(src)
    n = 1 << m
    if src.shape[-1] < n:
        raise ValueError(f"{src.shape[-1]} columns for m = {m}")
    x = np.array(src[..., :n], copy=True, order="C")
    lead = x.shape[:-1]
    for b in range(m):
        y = x.reshape(*lead, n >> (b + 1), 2, 1 << b)
        a = y[..., 0, :].copy()
        y[..., 0, :] += y[..., 1, :]
        np.subtract(a, y[..., 1, :], out=y[..., 1, :])
    return x


def kron2_host(src, m: int, mats) -> np.ndarray:
    """numpy model of ``qk_kron2_rows``: ``out[..., y] = sum_{x < 2^m} prod_b mats[b][y_b][x_b] src[..., x]``, by
    ``m`` levels of butterflies ``(a, b) -> (A[0][0] a + A[0][1] b, A[1][0] a + A[1][1] b)`` with ``a`` the element
    whose bit is clear and ``A = mats[b]``, lowest bit first, in the common dtype of ``src`` and ``mats`` (int64,
    float64 or ``np.longdouble``; the kernel takes the bits in another fixed order and fuses one product: equal
    for exactly representable sums, equal to rounding otherwise)."""
    src, A = np.asarray(src), np.asarray(mats)
    n = 1 << m
    if src.shape[-1] < n:
        raise ValueError(f"{src.shape[-1]} columns for m = {m}")
    if A.shape != (m, 2, 2) and not (m == 0 and A.size == 0):
        raise ValueError(f"mats must have shape [{m}, 2, 2], not {list(A.shape)}")
    x = np.array(src[..., :n], dtype=np.result_type(src.dtype, A.dtype) if m else src.dtype, copy=True, order="C")
    lead = x.shape[:-1]
    for b in range(m):
        y = x.reshape(*lead, n >> (b + 1), 2, 1 << b)
        lo, hi = y[..., 0, :].copy(), y[..., 1, :].copy()
        y[..., 0, :] = A[b, 0, 0] * lo + A[b, 0, 1] * hi
        y[..., 1, :] = A[b, 1, 0] * lo + A[b, 1, 1] * hi
    return x


ROWS_DOT_SEGMENT = 8192  # qknit_dot.hip: elements per (unit, segment) workgroup of qk_rows_dot


def rows_dot_chain(n: int) -> int:
    """The longest chain of additions an element passes through in ``qk_rows_dot`` at ``n`` elements per unit
    (qknit_dot.hip): 16 fused multiply-adds per accumulator, even + odd, a 6-level wave tree and 3 adds of the
    four wave sums in a segment; then ``ceil(segments / 64)`` lane-strided adds and the tree again."""
    nseg = -(-int(n) // ROWS_DOT_SEGMENT)
    return (16 + 1 + 6 + 3) + (-(-nseg // 64) + 6)


def rows_dot_host(Q, D, per: int = 1) -> np.ndarray:
    """numpy model of ``qk_rows_dot``: ``out[u] = sum_i Q[u, i] * D[u // per, i]`` for ``Q [units, n]`` and
    ``D [units / per, n]`` (numpy's pairwise summation; the kernel's own fixed order differs in the last bits)."""
    Q, D = np.asarray(Q, dtype=np.float64), np.asarray(D, dtype=np.float64)
    per = int(per)
    if Q.ndim != 2 or D.ndim != 2 or per < 1 or Q.shape[0] != D.shape[0] * per or Q.shape[1] != D.shape[1]:
        raise ValueError(f"Q {Q.shape} and D {D.shape} do not fit per = {per}")
    return np.einsum("dpi,di->dp", Q.reshape(D.shape[0], per, Q.shape[1]), D).reshape(-1)


def cotangent_scatter_host(C: np.ndarray, local_masks: list) -> tuple:
    """``(distinct masks ascending, C @ G)``: the columns of ``C [..., M]`` (one per Z string) summed onto the
    distinct values of ``local_masks`` by the 0/1 matrix ``G [M, distinct]``. Several strings may coincide on one
    fragment; the matmul combines them in one fixed order, where a scatter-add would not."""
    uniq = sorted(set(int(z) for z in local_masks))
    col = {z: j for j, z in enumerate(uniq)}
    G = np.zeros((len(local_masks), len(uniq)))
    G[np.arange(len(local_masks)), [col[int(z)] for z in local_masks]] = 1.0
    return uniq, np.matmul(C, G)


def cotangent_rows_host(Ws: list, qs: list, local: list, w) -> list:
    """numpy model of ``ParametricKnit.cotangent_rows``: per fragment ``D_f [rows_f, 2^m_f]`` with
    ``<D_f, q_f> = E_w = sum_m w[m] sum_t prod_f X_f[t, m]``, ``X_f = W_f^T red_f`` and ``red_f[r, m] = sum_x
    (-1)^popcount(x & local[f][m]) q_f[r, x]``. ``Ws[f]``: ``[rows_f, terms]``; ``qs[f]``: ``[rows_f, 2^m_f]``;
    ``local[f]``: the ``M`` masks restricted to fragment ``f``. ``D_f = wht(scatter(W_f (prod_{f' != f} X_f' * w)))``."""
    w = np.asarray(w, dtype=np.float64)
    X = []
    for W, q, fl in zip(Ws, qs, local):
        x = np.arange(q.shape[1])
        signs = np.stack([1.0 - 2.0 * (popcount(x & int(z)) & 1) for z in fl], axis=1)  # [2^m, M]
        X.append(W.T @ (q @ signs))
    out = []
    for f, (W, q, fl) in enumerate(zip(Ws, qs, local)):
        prod = np.ones_like(X[f])
        for g, xg in enumerate(X):
            if g != f:
                prod = prod * xg
        uniq, Cu = cotangent_scatter_host(W @ (prod * w[None, :]), fl)
        D = np.zeros(q.shape)
        D[:, uniq] = Cu
        out.append(wht_host(D, q.shape[1].bit_length() - 1))
    return out


def readout_matrix(e0: float, e1: float) -> np.ndarray:
    """The confusion matrix ``[[1 - e0, e1], [e0, 1 - e1]]`` of one clbit: ``A[y][x]`` is the probability of
    reading ``y`` when the bit is ``x``, ``e0 = P(read 1 | 0)`` and ``e1 = P(read 0 | 1)``, both in [0, 1]."""
    e0, e1 = float(e0), float(e1)
    if not (0.0 <= e0 <= 1.0 and 0.0 <= e1 <= 1.0):
        raise ValueError(f"e0 and e1 must lie in [0, 1], not {e0} and {e1}")
    return np.array([[1.0 - e0, e1], [e0, 1.0 - e1]])


def invert_channels(mats) -> np.ndarray:
    """The inverse of every 2x2 matrix of ``mats [..., 2, 2]``; ``ValueError`` where a determinant is 0 or not
    finite."""
    A = np.asarray(mats, dtype=np.float64)
    if A.ndim < 2 or A.shape[-2:] != (2, 2):
        raise ValueError(f"2x2 matrices, not an array of shape {list(A.shape)}")
    det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    if not np.isfinite(det).all() or (det == 0).any():
        raise ValueError("a matrix with determinant 0 (or a determinant that is not finite) has no inverse")
    inv = np.empty_like(A)
    inv[..., 0, 0], inv[..., 0, 1] = A[..., 1, 1] / det, -A[..., 0, 1] / det
    inv[..., 1, 0], inv[..., 1, 1] = -A[..., 1, 0] / det, A[..., 0, 0] / det
    return inv


def bit_channels(spec, n_clbits: int, measured) -> np.ndarray:
    """Per-clbit 2x2 matrices as float64 ``[n_clbits, 2, 2]``. ``spec``: such an array; a dict ``{clbit: 2x2}``,
    the identity for every other clbit; or one 2x2 matrix for every clbit in ``measured`` (the clbits some
    fragment measures). A clbit outside ``measured`` reads 0 in every key and can only carry the identity:
    ``ValueError`` for any other matrix on it, for a clbit out of range, a wrong shape or a value that is not
    finite."""
    measured = {int(c) for c in measured}
    out = np.tile(np.eye(2), (n_clbits, 1, 1))
    if isinstance(spec, dict):
        for c, A in spec.items():
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < n_clbits:
                raise ValueError(f"clbit {c!r} outside 0..{n_clbits - 1}")
            A = np.asarray(A, dtype=np.float64)
            if A.shape != (2, 2):
                raise ValueError(f"clbit {c}: a 2x2 matrix, not shape {list(A.shape)}")
            out[int(c)] = A
    else:
        A = np.asarray(spec, dtype=np.float64)
        if A.shape == (2, 2):
            out[sorted(measured)] = A
        elif A.shape == (n_clbits, 2, 2):
            out[:] = A
        else:
            raise ValueError(f"channels must be [{n_clbits}, 2, 2], a dict {{clbit: 2x2}} or one 2x2 matrix, "
                             f"not shape {list(A.shape)}")
    if not np.isfinite(out).all():
        raise ValueError("channel matrices must be finite")
    for c in range(n_clbits):
        if c not in measured and not np.array_equal(out[c], np.eye(2)):
            raise ValueError(f"no fragment measures clbit {c}: it is always 0 and takes only the identity")
    return out


def check_stochastic(mats, tol: float = 1e-12) -> None:
    """``ValueError`` unless every matrix of ``mats [..., 2, 2]`` is column-stochastic: no negative entry and
    column sums within ``tol`` of 1."""
    A = np.asarray(mats, dtype=np.float64)
    if (A < 0).any() or (np.abs(A.sum(axis=-2) - 1.0) > tol).any():
        raise ValueError("a confusion matrix must be column-stochastic: entries >= 0, columns summing to 1")


def key_positions(clbits: list, fragment_clbits: list) -> tuple:
    """For keys whose bit ``i`` is ``clbits[i]``: per fragment ``(keep, where)``, its local ``keep_mask``
    (as :func:`split_clbits`) and, for its kept local bits in ascending order, their bit of the key."""
    keep, positions = split_clbits(clbits, fragment_clbits)
    order = sorted(clbits)
    return keep, [[clbits.index(order[p]) for p in pos] for pos in positions]


def deposit_bits(keys, x, where: list):
    """``keys`` with bit ``i`` of ``x`` set at bit ``where[i]`` (integer arrays or tensors alike)."""
    for i, b in enumerate(where):
        keys = keys | (((x >> i) & 1) << b)
    return keys


def extract_bits(keys, where: list):
    """The inverse of :func:`deposit_bits`: bit ``i`` of the result is bit ``where[i]`` of ``keys`` (integer
    arrays or tensors alike)."""
    x = keys & 0
    for i, b in enumerate(where):
        x = x | (((keys >> b) & 1) << i)
    return x


def keys_array(keys, n_bits: int):
    """Outcome keys as a one-dimensional ``int64`` array ``[M]`` with every key in ``0 .. 2^n_bits - 1``. Ints,
    lists of ints and integer numpy arrays give a numpy array; a torch int64 tensor stays a tensor on its
    device and is range-checked there (one min / max sync). ``ValueError`` for a key outside the range, a
    non-integer dtype or more than one dimension."""
    if _is_tensor(keys):
        import torch as T

        if keys.dtype != T.int64:
            raise ValueError(f"a key tensor must hold int64, not {keys.dtype}")
        if keys.dim() > 1:
            raise ValueError(f"a key tensor must be one-dimensional, not {tuple(keys.shape)}")
        ks = keys.detach().reshape(-1).contiguous()
        if ks.numel():
            lo, hi = T.aminmax(ks)
            _check_range("key", int(lo), int(hi), n_bits)
        return ks
    if isinstance(keys, np.ndarray):
        return _int64_vector("key", keys, n_bits)
    keys = [keys] if isinstance(keys, (int, np.integer)) else list(keys)
    if not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in keys):
        raise ValueError("keys must be integers")
    if keys:
        _check_range("key", min(int(k) for k in keys), max(int(k) for k in keys), n_bits)
    return np.array([int(k) for k in keys], dtype=np.int64).reshape(-1)


def knit_at_host(Xs: list, positions: list, keys, dead: int = 0) -> np.ndarray:
    """numpy model of ``qk_knit_at`` in ``np.longdouble``: ``out[j] = sum_k prod_f Xs[f][k, x_f(j)]`` with bit
    ``i`` of ``x_f(j)`` = bit ``positions[f][i]`` of ``keys[j]``, and 0 where ``keys[j] & dead``. The operands
    are taken untransposed, ``[K, 2^m_f]``."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    prod = np.ones((np.asarray(Xs[0]).shape[0], keys.size), dtype=np.longdouble)
    for X, pos in zip(Xs, positions):
        prod *= np.asarray(X, dtype=np.longdouble)[:, extract_bits(keys, list(pos))]
    out = prod.sum(axis=0)
    out[(keys & np.int64(dead)) != 0] = 0
    return out


def gram_host(A, B=None, m: int | None = None) -> np.ndarray:
    """numpy model of ``qk_gram_rows`` in ``np.longdouble``: ``G[i, j] = sum_{x < 2^m} A[i, x] * B[j, x]``
    (``B=None``: ``B = A``; ``m=None``: every column of ``A``)."""
    A = np.asarray(A, dtype=np.longdouble)
    B = A if B is None else np.asarray(B, dtype=np.longdouble)
    n = A.shape[1] if m is None else 1 << int(m)
    if A.shape[1] < n or B.shape[1] < n:
        raise ValueError(f"{A.shape[1]} and {B.shape[1]} columns for {n} outcomes")
    return A[:, :n] @ B[:, :n].T


def gram_split(RA: int, RB: int, m: int, block: int = 64, min_groups: int = 512, max_split: int = 256,
               min_chunk: int = 256) -> dict:
    """The decomposition ``qk_gram_rows`` uses for a shape (qknit_moments.hip: gr_make_shape): ``ba x bb``
    blocks of ``block x block`` row pairs, the ``2^m`` outcomes cut into ``split`` equal chunks
    ``chunks[s] = (x0, x1)``, ascending; a function of ``(RA, RB, m)`` alone."""
    if RA < 1 or RB < 1 or not 0 <= m <= 30:
        raise ValueError(f"RA, RB >= 1 and 0 <= m <= 30, not ({RA}, {RB}, {m})")
    ba, bb, W = -(-RA // block), -(-RB // block), 1 << m
    split = 1
    while ba * bb * split < min_groups and split < max_split and W // (2 * split) >= min_chunk:
        split *= 2
    chunk = W // split
    return dict(ba=ba, bb=bb, split=split, chunk=chunk, chunks=[(s * chunk, (s + 1) * chunk) for s in range(split)],
                workspace_bytes=0 if split == 1 else ba * bb * split * block * block * 8)


def second_moment_host(Xs: list, Ys: list | None = None) -> np.longdouble:
    """``sum_x R[x] R'[x]`` of two knits ``R = sum_k prod_f Xs[f][k, x_f]``, ``R' = sum_k' prod_f Ys[f][k', x_f]``
    over the same fragments, in ``np.longdouble``: ``sum_{k, k'} prod_f (X_f Y_f^T)[k, k']``. ``Ys=None``:
    ``R' = R``."""
    Ys = Xs if Ys is None else Ys
    if len(Xs) != len(Ys) or not Xs:
        raise ValueError(f"{len(Xs)} and {len(Ys)} fragments")
    prod = None
    for X, Y in zip(Xs, Ys):
        G = gram_host(X, Y)
        prod = G if prod is None else prod * G
    return prod.sum()


def match_fragments(clbits_a: list, clbits_b: list, kept) -> tuple:
    """Pair the fragments of two partitions of the clbits, restricted to ``kept``. ``clbits_a[f]`` /
    ``clbits_b[g]``: the clbits of a fragment's outcome bits in local bit order. Two fragments are paired when
    they hold the same set of kept clbits, wherever they stand in their lists. Returns
    ``(pairs, only_a, only_b)``: ``pairs`` a list of ``(f, g, order)`` with ``order`` ``None`` where the kept
    clbits come in the same local order on both sides, else the list whose entry ``i`` is the bit of g's
    reduced index that holds bit ``i`` of f's; ``only_a`` / ``only_b`` the fragments with no kept clbit, which
    need no partner. ``ValueError``, naming the clbits, when the two partitions of ``kept`` differ."""
    kept = {int(c) for c in kept}
    seq_a = [[int(c) for c in fcl if int(c) in kept] for fcl in clbits_a]
    seq_b = [[int(c) for c in fcl if int(c) in kept] for fcl in clbits_b]
    by_set = {frozenset(s): g for g, s in enumerate(seq_b) if s}
    pairs, used = [], set()
    for f, s in enumerate(seq_a):
        if not s:
            continue
        g = by_set.get(frozenset(s))
        if g is None or g in used:
            theirs = sorted(sorted(t) for t in seq_b if set(t) & set(s))
            raise ValueError(f"the fragments cut the clbits differently: {sorted(s)} on one side, {theirs} on the other")
        used.add(g)
        pairs.append((f, g, None if seq_b[g] == s else [seq_b[g].index(c) for c in s]))
    for g, s in enumerate(seq_b):
        if s and g not in used:
            raise ValueError(f"the fragments cut the clbits differently: {sorted(s)} on one side only")
    return pairs, [f for f, s in enumerate(seq_a) if not s], [g for g, s in enumerate(seq_b) if not s]


# ----------------------------------------------------------------------------- the streamed scan: host models
SCAN_SIDE_BYTES = 4 << 30  # a side's operand [K, 2^bits] float64 beyond this is refused
SCAN_BINS = engine.SCAN_BINS


def scan_shape(ma: int, mb: int, i_begin: int = 0, i_end: int | None = None, tile: int = 128,
               max_groups: int = 512) -> dict:
    """The decomposition ``qk_knit_scan`` / ``qk_knit_collect`` use for a launch (qknit_scan.hip: sc_make_shape):
    ``tiles_m x tiles_n`` tiles of ``tile x tile`` outputs, tile ``t = (t // tiles_n, t % tiles_n)`` with the tile
    rows counted from ``i_begin``; ``groups = min(tiles, max_groups)`` workgroups, workgroup ``g`` owning the tiles
    ``g, g + groups, ...`` (:func:`scan_group_tiles`). A function of ``(mb, i_begin, i_end)`` alone."""
    i_end = 1 << ma if i_end is None else i_end
    if not (0 <= ma <= 30 and 0 <= mb <= 30 and 0 <= i_begin < i_end <= 1 << ma):
        raise ValueError(f"0 <= ma, mb <= 30 and 0 <= i_begin < i_end <= 2^ma, not ({ma}, {mb}, {i_begin}, {i_end})")
    tiles_m, tiles_n = -(-(i_end - i_begin) // tile), -(-(1 << mb) // tile)
    tiles = tiles_m * tiles_n
    groups = min(tiles, max_groups)
    return dict(tile=tile, i_begin=i_begin, i_end=i_end, n=1 << mb, tiles_m=tiles_m, tiles_n=tiles_n, tiles=tiles,
                groups=groups, workspace_bytes=groups * 18 * 8)


def scan_group_tiles(shape: dict, g: int) -> list:
    """The tiles of workgroup ``g`` of a :func:`scan_shape`, in the order it walks them: ``(i0, i1, j0, j1)``."""
    out, T = [], shape["tile"]
    for t in range(g, shape["tiles"], shape["groups"]):
        i0, j0 = shape["i_begin"] + (t // shape["tiles_n"]) * T, (t % shape["tiles_n"]) * T
        out.append((i0, min(i0 + T, shape["i_end"]), j0, min(j0 + T, shape["n"])))
    return out


def scan_sides(widths) -> tuple:
    """Assign fragments of ``widths[f]`` kept bits to the two sides of the scan: ``(side_a, side_b)``, lists of
    fragment indices. The widest fragment first (ties: the lower index), onto the side with fewer bits so far,
    ties to A; a fragment with no kept bit goes to A (it only scales A's rows). A side lists its fragments in the
    order they were placed: the first occupies the lowest bits of the side's index. One fragment leaves B empty
    (a column of ones)."""
    widths = [int(w) for w in widths]
    if any(w < 0 for w in widths):
        raise ValueError(f"negative width in {widths}")
    a, b, na, nb = [], [], 0, 0
    for f in sorted(range(len(widths)), key=lambda f: (-widths[f], f)):
        if widths[f] == 0 or na <= nb:
            a.append(f)
            na += widths[f]
        else:
            b.append(f)
            nb += widths[f]
    return a, b


def scan_bin(p) -> np.ndarray:
    """The histogram bin of positive values: ``clamp(-ilogb(p), 0, 127)``."""
    _, e = np.frexp(np.asarray(p, dtype=np.float64))  # p = f 2^e, 0.5 <= f < 1: ilogb = e - 1
    return np.clip(1 - e.astype(np.int64), 0, SCAN_BINS - 1)


def knit_scan_host(Xs: list, Ys: list | None = None, tau: float = 0.0) -> dict:
    """numpy model of ``qk_knit_scan`` in ``np.longdouble``, named as :func:`engine.knit_scan` names them. The knit
    is ``R[x] = sum_k prod_f Xs[f][k, x_f]`` over operands ``[K, 2^m_f]`` with fragment 0 in the lowest bits of the
    flat index ``x`` (the Khatri-Rao order); ``Ys``: a second knit on the same outputs. ``hist`` counts the float64
    value of every positive output; ``argmax`` / ``argmin`` are the lowest flat index among equal values."""
    def flat(Zs):
        R = np.ones((np.asarray(Zs[0]).shape[0], 1), dtype=np.longdouble)
        for Z in Zs:  # the new fragment above the bits so far
            Z = np.asarray(Z, dtype=np.longdouble)
            R = (Z[:, :, None] * R[:, None, :]).reshape(Z.shape[0], -1)
        return R.sum(axis=0)

    if not Xs:
        raise ValueError("no fragment")
    R = flat(Xs)
    P = np.maximum(R, 0)
    pos = R > 0
    lnP = np.log(P, where=pos, out=np.zeros_like(P))
    hist = np.bincount(scan_bin(R[pos].astype(np.float64)), minlength=SCAN_BINS).astype(np.int64)
    out = dict(sum=R.sum(), abs=np.abs(R).sum(), pos=P.sum(), sq=(R * R).sum(), ent=-(P * lnP).sum(), max=R.max(),
               min=R.min(), sum2=0.0, pos2=0.0, cross=0.0, hell=0.0, l1d=0.0, maxd=0.0,
               count_tau=int((R > tau).sum()), count_pos=int(pos.sum()), argmax=int(np.argmax(R)),
               argmin=int(np.argmin(R)), hist=hist, values=R)
    if Ys is not None:
        if len(Ys) != len(Xs) or any(np.asarray(X).shape[1] != np.asarray(Y).shape[1] for X, Y in zip(Xs, Ys)):
            raise ValueError("the two knits have different fragments")
        R2 = flat(Ys)
        P2 = np.maximum(R2, 0)
        out.update(sum2=R2.sum(), pos2=P2.sum(), cross=(R * R2).sum(), hell=np.sqrt(P * P2).sum(),
                   l1d=np.abs(R - R2).sum(), maxd=np.abs(R - R2).max(), values2=R2)
    return out


def histogram_threshold(hist, k: int) -> tuple:
    """``(tau, count)`` for the ``k`` largest outputs from a scan's histogram: the smallest bin ``b`` whose
    cumulative count (bin 0 holds the largest values) reaches ``k``, ``tau`` the largest double below that bin's
    lower edge ``2^-b`` and ``count`` the number of outputs ``> tau``, known before anything is collected. Bin 127
    has no lower edge but 0, and ``k`` above the support gives ``(0.0, support)``: every positive output."""
    hist = np.asarray(hist, dtype=np.int64)
    if hist.shape != (SCAN_BINS,) or k < 0:
        raise ValueError(f"a histogram of {SCAN_BINS} bins and k >= 0, not {hist.shape} and {k}")
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, k, side="left"))
    if k == 0 or b >= SCAN_BINS - 1:
        return (np.inf, 0) if k == 0 else (0.0, int(cum[-1]))
    return float(np.nextafter(np.ldexp(1.0, -b), 0.0)), int(cum[b])


# ----------------------------------------------------------------------------- nearest probability distribution
def project_scan_shape(ma: int, mb: int, i_begin: int = 0, i_end: int | None = None) -> dict:
    """:func:`scan_shape` for ``qk_knit_project_scan``: the same decomposition; the workspace holds 16 partial sums
    and one index per workgroup."""
    sh = scan_shape(ma, mb, i_begin, i_end)
    sh["workspace_bytes"] = sh["groups"] * 17 * 8
    return sh


def project_scan_host(Xs: list, Ys: list | None = None, theta: float = 0.0, theta2: float = 0.0,
                      accuracy: float = 0.0) -> dict:
    """numpy model of ``qk_knit_project_scan`` in ``np.longdouble``, named as :func:`engine.knit_project_scan` names
    them; the knit and the flat index as in :func:`knit_scan_host`. ``member = |v| > accuracy``,
    ``kept = v > max(theta, accuracy)`` (strict: an entry exactly at ``theta`` or at ``accuracy`` is not kept, one at
    ``-accuracy`` and an exact zero are not members), ``p = v - theta`` on the kept, else 0. ``values`` / ``values2``
    hold ``p`` / ``p'``."""
    theta, theta2, accuracy = engine.check_projection_args(theta, theta2, accuracy)

    def one(Zs, th):
        R = knit_scan_host(Zs)["values"]
        member, kept = np.abs(R) > accuracy, R > max(th, accuracy)
        p = np.where(kept, R - np.longdouble(th), np.longdouble(0))
        lnp = np.log(p, where=kept, out=np.zeros_like(p))
        return p, dict(msum=R[member].sum(), tsum=R[kept].sum(), psum=p.sum(), psq=(p * p).sum(), pent=-(p * lnp).sum(),
                       pmax=p.max(), nmember=int(member.sum()), nkept=int(kept.sum()))

    p, out = one(Xs, theta)
    out.update(argmax=int(np.argmax(p)), values=p, hell=0.0, l1d=0.0, maxd=0.0, nmember2=0, nkept2=0)
    out.update({name + "2": 0.0 for name in ("msum", "tsum", "psum", "psq", "pent", "pmax")})
    if Ys is not None:
        if len(Ys) != len(Xs) or any(np.asarray(X).shape[1] != np.asarray(Y).shape[1] for X, Y in zip(Xs, Ys)):
            raise ValueError("the two knits have different fragments")
        q, second = one(Ys, theta2)
        out.update({name + "2": v for name, v in second.items()})
        out.update(hell=np.sqrt(p * q).sum(), l1d=np.abs(p - q).sum(), maxd=np.abs(p - q).max(), values2=q)
    return out


# ----------------------------------------------------------------------------- the projection as a distribution
PROJ_TILE_MASKS = engine.PROJ_TILE_MASKS
PROJ_TILE_BYTES = 64 << 20  # the tile masses W [masks, tiles] float64 of one pass: beyond it, fewer masks per pass
PROJ_DRAW_LABEL = 1 << 20   # the uniforms' label of KnitReducer.projected_sample, clear of sample()'s fragment labels
PROJ_MARGINAL_MASK_BITS = 6  # projected_marginal by the mask route: 2^k expectations


def project_tile_walk() -> np.ndarray:
    """int64 ``[16384, 2]``: the (row, column) offsets in a 128 x 128 tile in walk order, the order in which
    ``qk_knit_project_tiles`` adds a tile's outputs and ``qk_knit_project_draw`` counts them: thread ``tid``
    ascending, within a thread block row ``i``, block column ``j``, register ``r`` ascending, which is the output at
    row ``64 (wave & 1) + 16 i + (lane >> 4) + 4 r`` and column ``64 (wave >> 1) + 16 j + (lane & 15)`` with
    ``lane = tid & 63``, ``wave = tid >> 6`` (qknit_scan.hip: sc_row, sc_col)."""
    tid, i, j, r = np.meshgrid(np.arange(256), np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    lane, wave = tid & 63, tid >> 6
    row = 64 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r
    col = 64 * (wave >> 1) + 16 * j + (lane & 15)
    return np.stack([row.reshape(-1), col.reshape(-1)], axis=1).astype(np.int64)


def _project_sides(Xs: list) -> tuple:
    if len(Xs) != 2:
        raise ValueError("the tile models take the two sides [B, A] (side B in the low bits of the flat index)")
    nb, na = np.asarray(Xs[0]).shape[1], np.asarray(Xs[1]).shape[1]
    if na & (na - 1) or nb & (nb - 1):
        raise ValueError(f"sides of {na} and {nb} columns: not powers of two")
    return na.bit_length() - 1, nb.bit_length() - 1


def _project_tiled(Xs: list, theta: float, accuracy: float, i_begin: int, i_end) -> tuple:
    """``(P [tiles, 128, 128], shape)``: ``p`` of the rows ``[i_begin, i_end)`` cut into the tiles of
    :func:`scan_shape`, zero where a tile passes the range."""
    ma, mb = _project_sides(Xs)
    sh = scan_shape(ma, mb, i_begin, i_end)
    p = project_scan_host(Xs, theta=theta, accuracy=accuracy)["values"].reshape(1 << ma, 1 << mb)
    P = np.zeros((sh["tiles_m"] * 128, sh["tiles_n"] * 128), dtype=np.longdouble)
    P[:sh["i_end"] - sh["i_begin"], :1 << mb] = p[sh["i_begin"]:sh["i_end"]]
    P = P.reshape(sh["tiles_m"], 128, sh["tiles_n"], 128).transpose(0, 2, 1, 3).reshape(sh["tiles"], 128, 128)
    return P, sh, ma, mb


def project_tiles_host(Xs: list, theta: float, accuracy: float, masks=((0, 0),), i_begin: int = 0,
                       i_end: int | None = None) -> np.ndarray:
    """numpy model of ``qk_knit_project_tiles`` in ``np.longdouble``: ``W [len(masks), tiles]``. ``Xs = [B, A]``,
    the two sides as :func:`project_scan_host` takes them (side B in the low bits); ``masks``: pairs ``(za, zb)``
    over the absolute side indices."""
    P, sh, ma, mb = _project_tiled(Xs, theta, accuracy, i_begin, i_end)
    tm, tn = np.divmod(np.arange(sh["tiles"]), sh["tiles_n"])
    rows = (sh["i_begin"] + 128 * tm)[:, None] + np.arange(128)  # [tiles, 128] absolute
    cols = (128 * tn)[:, None] + np.arange(128)
    out = np.zeros((len(masks), sh["tiles"]), dtype=np.longdouble)
    for m, (za, zb) in enumerate(masks):
        if za < 0 or zb < 0 or za >> ma or zb >> mb:
            raise ValueError(f"mask ({za:#x}, {zb:#x}) has a bit outside the sides' {ma} and {mb} bits")
        sa = 1 - 2 * (popcount(rows & za) & 1)
        sb = 1 - 2 * (popcount(cols & zb) & 1)
        out[m] = (P * sa[:, :, None] * sb[:, None, :]).sum(axis=(1, 2))
    return out


def project_draw_host(Xs: list, theta: float, accuracy: float, u, i_begin: int = 0, i_end: int | None = None) -> tuple:
    """numpy model of ``qk_knit_project_draw`` in ``np.longdouble``: ``(flat int64 [n], pval [n], total)`` from the
    CDF of ``p`` in (tile, walk) order, draw ``d`` being the first output whose inclusive prefix exceeds
    ``u[d] * total``; ``flat = -1`` and ``pval = 0`` where the total is not > 0. ``Xs`` as
    :func:`project_tiles_host`."""
    P, sh, ma, mb = _project_tiled(Xs, theta, accuracy, i_begin, i_end)
    walk = project_tile_walk()
    seq = P[:, walk[:, 0], walk[:, 1]].reshape(-1)
    u = np.asarray(u, dtype=np.longdouble).reshape(-1)
    cdf = np.cumsum(seq)
    total = cdf[-1]
    if not total > 0:
        return np.full(u.size, -1, dtype=np.int64), np.zeros(u.size, dtype=np.longdouble), total
    kept = np.flatnonzero(seq > 0)
    at = np.minimum(np.searchsorted(cdf, u * total, side="right"), kept[-1])
    at = kept[np.searchsorted(kept, at)]  # an output that is kept: the prefix rises only there
    tile, pos = np.divmod(at, 16384)
    row = sh["i_begin"] + 128 * (tile // sh["tiles_n"]) + walk[pos, 0]
    col = 128 * (tile % sh["tiles_n"]) + walk[pos, 1]
    return (row << mb | col).astype(np.int64), seq[at], total


def project_walk_rank(ma: int, mb: int, i_begin: int = 0, i_end: int | None = None) -> np.ndarray:
    """int64 ``[2^(ma + mb)]``: the rank of every flat index ``i << mb | j`` in the (tile, walk) order of the rows
    ``[i_begin, i_end)`` (``16384 tile + position in the walk``); -1 for a row outside the range."""
    sh = scan_shape(ma, mb, i_begin, i_end)
    walk = project_tile_walk()
    pos = np.empty((128, 128), dtype=np.int64)
    pos[walk[:, 0], walk[:, 1]] = np.arange(16384)
    i, j = np.arange(sh["i_begin"], sh["i_end"])[:, None], np.arange(1 << mb)[None, :]
    tile = ((i - sh["i_begin"]) >> 7) * sh["tiles_n"] + (j >> 7)
    out = np.full((1 << ma, 1 << mb), -1, dtype=np.int64)
    out[sh["i_begin"]:sh["i_end"]] = 16384 * tile + pos[(i - sh["i_begin"]) & 127, j & 127]
    return out.reshape(-1)


def inverse_wht_marginal(values) -> np.ndarray:
    """The ``2^k`` entries of a distribution over ``k`` bits from its ``2^k`` Z-string expectation values,
    ``values[s] = sum_y (-1)^popcount(s & y) q[y]``: ``q[y] = 2^-k sum_s (-1)^popcount(s & y) values[s]``."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    k = v.size.bit_length() - 1
    if v.size != 1 << k:
        raise ValueError(f"{v.size} values: not a power of two")
    s = np.arange(v.size)
    H = 1 - 2 * (popcount(s[:, None] & s[None, :]) & 1)
    return (H @ v) / v.size


@dataclass
class ProjectionThreshold:
    """What :func:`projection_threshold` returns. ``msum`` / ``tsum``: the last evaluation's."""
    theta: float
    kept: int
    passes: int
    msum: float
    tsum: float


def projection_threshold(evaluate, max_passes: int = 32) -> ProjectionThreshold:
    """The threshold of ``nearest_probability_distribution`` (``quasi_distr.py:28-43``) by Newton's (Michelot's)
    iteration. ``evaluate(theta) -> (MSUM, TSUM, NKEPT)``: the sum of the members, and the sum and the number of the
    kept entries (those above ``theta``). The projection keeps ``v - theta`` on ``{v > theta}`` with ``theta`` such
    that the kept values sum to ``MSUM``: ``f(theta) = TSUM - theta NKEPT - MSUM`` is convex, piecewise linear and
    decreasing with ``f(0) >= 0``, so ``theta <- (TSUM - MSUM) / NKEPT`` from 0 rises monotonically, never passes
    the root and has reached it when ``NKEPT`` stops changing. ``MSUM <= 0``, or no kept entry at some pass, is the
    empty projection: ``kept = 0``, ``theta = inf``. ``RuntimeError`` after ``max_passes`` evaluations."""
    theta, last = 0.0, None
    for passes in range(1, int(max_passes) + 1):
        msum, tsum, kept = evaluate(theta)
        msum, tsum, kept = float(msum), float(tsum), int(kept)
        if not msum > 0.0 or kept == 0:
            return ProjectionThreshold(float("inf"), 0, passes, msum, 0.0)
        if kept == last:
            return ProjectionThreshold(theta, kept, passes, msum, tsum)
        theta, last = (tsum - msum) / kept, kept
    raise RuntimeError(f"the projection threshold did not settle in {max_passes} passes (theta = {theta!r}, "
                       f"{last} kept)")


@dataclass
class KnitProjection:
    """What :meth:`KnitReducer.project` returns: the nearest probability distribution of the knit ``R`` (of its
    marginal onto ``clbits``) is ``R - theta`` on ``{R > max(theta, accuracy)}`` and 0 elsewhere."""
    theta: float         # inf: the empty projection (mass <= 0)
    accuracy: float      # the truncation: only |R| > accuracy are members
    mass: float          # MSUM: the sum of the members, which the kept entries' projections sum to
    kept: int            # entries of the projection
    members: int
    dropped_mass: float  # MSUM - TSUM: the sum of the members that are not kept, spread over the kept ones
    passes: int          # kernel passes the iteration took
    clbits: list         # bit i of a key is clbits[i]


@dataclass
class ProjectedScan:
    """What :meth:`KnitReducer.projected_scan` returns: statistics of the projection ``p``."""
    mass: float             # sum p
    collision: float        # sum p^2
    shannon_entropy: float  # bits, of p / sum p (nan without the entropy term or with nothing kept)
    max: float
    argmax: int | None      # key of the maximum, the lowest flat index among equal values; None with nothing kept
    support: int            # kept entries


def _side_operand(ctx, parts: list, K: int, dev):
    """One side of the scan from ``parts = [X_f [K, 2^w_f], ...]``: their Khatri-Rao product, the first part in the
    lowest bits; parts of one column only scale the rows; no part at all is a column of ones."""
    T = engine.torch()
    bits = sum(X.shape[1].bit_length() - 1 for X in parts)
    if bits > 30 or K * 8 << bits > SCAN_SIDE_BYTES:
        raise ValueError(f"a side of the scan holds K = {K} terms of {bits} bits: [{K}, 2^{bits}] float64 exceeds "
                         f"SCAN_SIDE_BYTES = {SCAN_SIDE_BYTES}")
    X = scale = None
    for Xf in parts:
        if Xf.shape[1] == 1:
            scale = Xf if scale is None else scale * Xf
        else:
            X = Xf if X is None else engine.khatri_rao(ctx, X.contiguous(), Xf.contiguous())
    if X is None:
        X = T.ones((K, 1), dtype=T.float64, device=dev)
    return X if scale is None else X * scale


class ScanSides(NamedTuple):
    """What :meth:`KnitReducer._scan_operands` returns: the two sides of the scan of a marginal, each the Khatri-Rao
    product of its fragments' reduced operands (:func:`scan_sides`, :func:`_side_operand`)."""
    A: object          # device float64 [K, 2^len(where_a)]
    B: object          # device float64 [K, 2^len(where_b)]
    where_a: list      # the key bit of every bit of side A's index
    where_b: list
    A2: object = None  # the same sides of another reducer's knit, in this one's bit order
    B2: object = None

    def key(self, flat):
        """Flat scan indices ``i << mb | j`` (an int or an int64 tensor) as keys."""
        mb = len(self.where_b)
        return deposit_bits(deposit_bits(flat & 0, flat >> mb, self.where_a), flat & ((1 << mb) - 1), self.where_b)


@dataclass
class KnitScan:
    """What :meth:`KnitReducer.scan` returns: statistics of the exact knit (or a marginal of it) ``R``."""
    mass: float            # sum R
    l1: float              # sum |R|
    positive_mass: float   # sum max(R, 0)
    negativity: float      # (l1 - mass) / 2: the negative mass of the quasi-distribution
    collision: float       # sum R^2
    shannon_entropy: float  # bits, of p = max(R, 0) / positive_mass (nan without the entropy term)
    max: float
    argmax: int            # key of the maximum, the lowest flat index among equal values
    min: float
    argmin: int
    count_above: int       # outputs with R > threshold (strict)
    support: int           # outputs with R > 0
    histogram: np.ndarray  # int64 [128]: positive outputs by binade, bin clamp(-ilogb(p), 0, 127)


MOMENT_WORK_BYTES = 256 << 20  # the [rows, K'] temporaries of KnitReducer.overlap: K beyond it goes in row blocks


def _ones_spec(T, dev, K: int) -> tuple:
    """The gather that repeats row 0 ``K`` times with coefficient 1: the operand of an ``m = 0`` factor of ones."""
    return ("G", T.zeros(K, dtype=T.int64, device=dev), T.ones(K, dtype=T.float64, device=dev))


def _permute_bits(T, rows, order):
    """``rows`` re-indexed so that bit ``i`` of the new column index is bit ``order[i]`` of the old one."""
    if order is None:
        return rows
    y = T.arange(rows.shape[1], dtype=T.int64, device=rows.device)
    return rows.index_select(1, deposit_bits(T.zeros_like(y), y, order))


def overlap_of_sides(ctx, side_a: tuple, side_b, kept) -> float:
    """``sum_{k, k'} prod_f G_f[k, k']`` of two sides ``(rows, specs, clbits, K)``, the work of
    :meth:`KnitReducer.overlap`. ``rows[f]``: device float64 ``[R_f, 2^k_f]``, a fragment's rows reduced onto its
    kept clbits (column bit ``i`` = its ``i``-th kept clbit in ``clbits[f]`` order); ``specs[f]``: how its operand
    ``X_f [K, 2^k_f]`` follows from them, ``("T", W^T [R_f, K])`` for ``X_f = W rows`` or ``("G", idx [K], coefs [K])``
    for ``X_f[k] = coefs[k] rows[idx[k]]``, on the device; ``clbits[f]``: the fragment's clbits in local bit order;
    ``K``: the number of terms. ``side_b=None``: the side itself (the Grams are then symmetric calls). The
    fragments are paired by :func:`match_fragments` on ``kept``; where the local bit orders of a pair differ the
    columns of b's rows are permuted to a's order."""
    T = engine.torch()
    same = side_b is None
    qa, sa, cla, Ka = side_a
    qb, sb, clb, Kb = side_a if same else side_b
    dev = qa[0].device
    pairs, only_a, only_b = match_fragments(cla, clb, kept)
    one = T.ones((1, 1), dtype=T.float64, device=dev)
    # (rows_a, spec_a, rows_b, spec_b, symmetric): an unpaired fragment meets a row of one 1.0 gathered K times
    work = [(qa[f], sa[f], _permute_bits(T, qb[g], order), sb[g], same and f == g) for f, g, order in pairs]
    work += [(qa[f], sa[f], one, _ones_spec(T, dev, Kb), False) for f in only_a]
    work += [(one, _ones_spec(T, dev, Ka), qb[g], sb[g], False) for g in only_b]
    halves = []  # per fragment: Gq applied to the b side, [R_a, K']
    for ra, _, rb, spec_b, sym in work:
        m = ra.shape[1].bit_length() - 1
        if spec_b[0] == "T":  # H = Gq W' = (Gq^T)^T W': the Gram is formed transposed
            GqT = engine.gram_rows(ctx, ra, None, m) if sym else engine.gram_rows(ctx, rb, ra, m)
            H = T.empty((ra.shape[0], Kb), dtype=T.float64, device=dev)
            halves.append(engine.gemm_keyed(ctx, GqT, spec_b[1], out=H, strideA=Kb))
        else:
            Gq = engine.gram_rows(ctx, ra, None if sym else rb, m)
            halves.append(Gq.index_select(1, spec_b[1]) * spec_b[2])
    step = max(1, MOMENT_WORK_BYTES // (16 * Kb))
    sums = T.empty(Ka, dtype=T.float64, device=dev)
    for k0 in range(0, Ka, step):
        k1 = min(k0 + step, Ka)
        prod = None
        for (_, spec_a, _, _, _), H in zip(work, halves):
            if spec_a[0] == "T":  # G_f[k0:k1] = (W^T[:, k0:k1])^T H
                G = T.empty((k1 - k0, Kb), dtype=T.float64, device=dev)
                engine.gemm_keyed(ctx, spec_a[1][:, k0:k1], H, out=G, strideA=Kb)
            else:
                G = H.index_select(0, spec_a[1][k0:k1]) * spec_a[2][k0:k1, None]
            prod = G if prod is None else prod.mul_(G)
        T.sum(prod, dim=1, out=sums[k0:k1])  # a row's K' products, then the rows: two fixed trees
    return float(sums.sum())


def _user_order(T, asc_result, clbits: list):
    """Result indexed with bit i = clbits[i], from the one indexed by the ascending clbits."""
    order = sorted(clbits)
    if clbits == order:
        return asc_result
    rank = {c: i for i, c in enumerate(order)}
    u = T.arange(asc_result.numel(), dtype=T.int64, device=asc_result.device)
    a = T.zeros_like(u)
    for i, c in enumerate(clbits):
        a |= ((u >> i) & 1) << rank[c]
    return asc_result[a]


# ----------------------------------------------------------------------------- the reducer
class KnitReducer:
    """One sweep of a cut circuit, then marginals and Z-string expectation values of its exact
    knit. Exact instances on the MI355X backend, one GPU. ``factored``: None / True take the
    factored knit where ``engine.factored_ok`` holds, False the direct knit over all labels."""

    def __init__(self, virt, *, device: int = 0, factored: bool | None = None):
        if not all(isinstance(virt.get_backend(f), MI355XBackend) for f in virt.fragment_circuits if len(f)):
            raise ValueError("KnitReducer needs every fragment on the MI355X backend")
        self.N = virt.circuit.num_clbits
        if self.N > MAX_CLBITS:
            raise ValueError(f"{self.N} clbits: keys are int64, at most {MAX_CLBITS}")
        self.device = device
        self.ctx = ctx = engine.get_context(device)
        self.factored = (factored is None or bool(factored)) and engine.factored_ok(virt)
        self.frags = engine.prepare_fragments(virt, device, basis=self.factored)
        # the swept rows: only ever read from here on
        self.qs = [engine.sweep_fragment(ctx, fs).contiguous() for fs in self.frags]
        self.ops = engine.knit_operands(virt, self.frags, self.factored)
        self.clbits = [list(c) for c in self.ops.clbits]
        self._spectrum = None  # z_spectrum(): formed on first use
        self._transposed = None  # transposed_operands(): formed on first use
        self._moment_specs = None  # _moment_sides(): the transforms / gathers on the device, formed on first use
        self._spectrum_t = None  # the spectrum transposed (expectation(method="fused")): formed on first use
        if not self.frags:  # no fragment at all: the knit is the sum of the coefficients at key 0
            vg = [v.operation for v in virt.vgate_instructions]
            self._scalar = float(LabelSpace([g.num_instantiations for g in vg],
                                            [g.knit_coefficients() for g in vg]).coefficients().sum())

    # -- pieces ---------------------------------------------------------------------------------
    def _clbits(self, clbits) -> list:
        return list(range(self.N)) if clbits is None else check_clbits(clbits, self.N)

    def _check_other(self, other) -> None:
        """``ValueError`` unless ``other`` is a reducer this one's knit can be compared with."""
        if not isinstance(other, KnitReducer):
            raise ValueError("other must be a KnitReducer")
        if other.N != self.N:
            raise ValueError(f"{self.N} clbits against {other.N}")
        if other.device != self.device:
            raise ValueError(f"reducers on devices {self.device} and {other.device}")

    def _reduced(self, keep: list, flips: list | None = None) -> list:
        """Per fragment ``[R_f, len(flips[f]) * 2^k_f]``: its swept rows reduced onto ``keep[f]``, once per flip mask
        (``None``: the plain marginal, ``[0]`` for every fragment)."""
        reds = []
        for q, fcl, kp, fl in zip(self.qs, self.clbits, keep, flips or [[0]] * len(keep)):
            m = len(fcl)
            if kp == (1 << m) - 1 and fl == [0]:  # nothing to sum out
                reds.append(q)
            else:
                reds.append(engine.reduce_bits(self.ctx, q, m, kp, fl))
        return reds

    def _operands(self, keep: list, flips: list | None = None) -> list:
        """Per fragment ``[terms, len(flips[f]) * 2^k_f]``: its swept rows reduced (:meth:`_reduced`), then
        transformed."""
        return engine.fragment_operands(self.ctx, self.ops, self._reduced(keep, flips))

    def _keyed_operands(self, cl: list) -> tuple:
        """``(mats, where, K)`` for keys whose bit ``i`` is ``cl[i]``: per fragment its operand reduced onto its
        clbits in ``cl`` and the key bit of every bit of that operand's column index (:func:`key_positions`), and
        the number of terms. No fragment at all is one fragment of no bit whose single entry holds ``_scalar``."""
        if not self.frags:
            T = engine.torch()
            return [T.full((1, 1), self._scalar, dtype=T.float64, device=T.device("cuda", self.device))], [[]], 1
        keep, where = key_positions(cl, self.clbits)
        return self._operands(keep), where, self.ops.num_terms

    def _contract(self, mats: list, positions: list, k: int):
        T = engine.torch()
        out = T.zeros(1 << k, dtype=T.float64, device=T.device("cuda", self.device))
        if not mats:
            out[0] = self._scalar
            return out
        return engine.contract(self.ctx, mats, positions, out)

    # -- per-clbit channels ---------------------------------------------------------------------
    def _measured(self) -> set:
        return {c for fcl in self.clbits for c in fcl}

    def _measured_among(self, clbits) -> int:
        """How many of the chosen clbits (``None``: all) some fragment measures."""
        return len(self._measured() & set(self._clbits(clbits)))

    def with_channels(self, spec) -> "KnitReducer":
        """A reducer of ``R'[y] = sum_x prod_c A_c[y_c][x_c] R[x]``, ``A_c`` the real 2x2 matrix of clbit ``c``
        (``spec``: see :func:`bit_channels`), without another sweep: the map acts on the column index of each
        fragment's swept rows, one bit at a time, and commutes with the transform ``W_f`` on their row index, so
        the new reducer holds the rows transformed out of place (``qk_kron2_rows``; fragment f takes the matrices
        of its clbits) and shares the context, the fragments and the operands' description with this one. Every
        answer of the new reducer is that of ``R'``; its caches start empty, and this reducer is left as it is.
        No fragment at all: the reducer itself (no clbit is measured, only the identity applies)."""
        mats = bit_channels(spec, self.N, self._measured())
        if not self.frags:
            return self
        self.ctx.bind_stream()
        new = object.__new__(KnitReducer)
        new.__dict__.update(self.__dict__)
        new.qs = [engine.kron2_rows(self.ctx, q, mats[fcl] if fcl else np.zeros((0, 2, 2)), len(fcl))
                  for q, fcl in zip(self.qs, self.clbits)]
        new._spectrum = new._transposed = new._moment_specs = new._spectrum_t = None
        return new

    def with_readout_error(self, confusion) -> "KnitReducer":
        """:meth:`with_channels` of per-clbit confusion matrices (:func:`readout_matrix`): the distribution a
        device with that readout error returns. Every matrix must be column-stochastic (:func:`check_stochastic`)."""
        mats = bit_channels(confusion, self.N, self._measured())
        check_stochastic(mats)
        return self.with_channels(mats)

    def with_readout_mitigation(self, confusion) -> "KnitReducer":
        """:meth:`with_channels` of the inverses of per-clbit confusion matrices (:func:`invert_channels`): the
        quasi-distribution that readout mitigation makes of this knit. ``confusion`` as for
        :meth:`with_readout_error`, and every matrix invertible."""
        mats = bit_channels(confusion, self.N, self._measured())
        check_stochastic(mats)
        return self.with_channels(invert_channels(mats))

    # -- public ---------------------------------------------------------------------------------
    def marginal(self, clbits):
        """Device fp64 tensor ``[2^k]`` of the exact knit summed over every other clbit; bit ``i`` of
        the index is ``clbits[i]``. A clbit no fragment measures is always 0."""
        self.ctx.bind_stream()
        cl = check_clbits(clbits, self.N)
        keep, positions = split_clbits(cl, self.clbits)
        return _user_order(engine.torch(), self._contract(self._operands(keep), positions, len(cl)), cl)

    def expectation(self, masks, *, method: str = "reduce") -> np.ndarray:
        """float64 ``[M]``: ``sum_key (-1)^popcount(key & mask) R[key]`` of the exact quasi-distribution
        (no projection onto the probability simplex) per mask; see :func:`parse_masks`.
        ``method="reduce"``: one ``qk_reduce_bits`` pass over the swept rows per batch of masks.
        ``method="spectrum"``: a gather from :meth:`z_spectrum` (formed once per reducer), for many masks;
        ``masks`` may then also be an integer numpy array or an int64 tensor (:func:`masks_array`). The
        two agree to rounding, not bit for bit.
        ``method="fused"``: the same spectrum, read by the lookup kernel (``qk_knit_at`` on a transposed copy
        of it, formed once and kept; as much memory again): one launch for all masks, the masks being the
        keys. Masks as for ``"spectrum"``; agrees with it to rounding."""
        if method == "spectrum":
            return self._expectation_spectrum(masks)
        if method == "fused":
            return self._expectation_fused(masks)
        if method != "reduce":
            raise ValueError(f"method must be 'reduce', 'spectrum' or 'fused', not {method!r}")
        self.ctx.bind_stream()
        zs = parse_masks(masks, self.N)
        if not zs:
            return np.zeros(0)
        if not self.frags:
            return np.full(len(zs), self._scalar)
        local = [list(col) for col in zip(*(split_mask(z, self.clbits) for z in zs))]  # per fragment, per mask
        mats = self._operands([0] * len(self.frags), local)  # [terms, M] per fragment
        prod = mats[0]
        for a in mats[1:]:
            prod = prod * a
        return prod.sum(0).cpu().numpy()

    # -- all Z strings: the Walsh-Hadamard spectrum ---------------------------------------------
    def z_spectrum(self) -> list:
        """Per fragment the device tensor ``H_f [terms, 2^m_f]``: the Walsh-Hadamard transform
        (``qk_wht_rows``) of its unreduced operand ``X_f``, so ``H_f[k][z] = sum_x (-1)^popcount(x & z)
        X_f[k][x]`` is the fragment's factor of every Z string at once. Formed on first use and kept:
        later calls return the same tensors (as much memory as the operands themselves; treat them as
        read-only). A dropped fragment is an ``m = 0`` factor; no fragment at all gives ``[]``."""
        if self._spectrum is None:
            self.ctx.bind_stream()
            mats = engine.fragment_operands(self.ctx, self.ops, self.qs) if self.frags else []
            # the operands are fresh tensors: transform them where they are
            self._spectrum = [engine.wht_rows(self.ctx, X, len(fcl), out=X) for X, fcl in zip(mats, self.clbits)]
        return self._spectrum

    def _spectrum_chunks(self, zs: np.ndarray):
        """``(start, device float64 [n])`` per chunk of ``SPECTRUM_GATHER_CHUNK`` masks: the product over
        fragments of ``H_f[:, z_f]``, summed over the terms by a fixed tree of elementwise adds (a mask's
        value does not depend on the chunk it falls in)."""
        T = engine.torch()
        dev = T.device("cuda", self.device)
        H = self.z_spectrum()
        local = split_masks_array(zs, self.clbits)
        for s in range(0, len(zs), SPECTRUM_GATHER_CHUNK):
            prod = None
            for Hf, lf in zip(H, local):
                g = Hf.index_select(1, T.from_numpy(lf[s:s + SPECTRUM_GATHER_CHUNK]).to(dev))
                prod = g if prod is None else prod.mul_(g)
            while prod.shape[0] > 1:  # rows k and k + ceil(K / 2), level by level
                h = (prod.shape[0] + 1) // 2
                prod[:prod.shape[0] - h] += prod[h:]
                prod = prod[:h]
            yield s, prod[0]

    def _expectation_spectrum(self, masks) -> np.ndarray:
        self.ctx.bind_stream()
        zs = masks_array(masks, self.N)
        if not self.frags:
            return np.full(len(zs), self._scalar) if len(zs) else np.zeros(0)
        out = np.zeros(len(zs))
        for s, vals in self._spectrum_chunks(zs):
            out[s:s + vals.numel()] = vals.cpu().numpy()
        return out

    def expectation_sum(self, masks, weights) -> float:
        """``sum_j weights[j] <Z_masks[j]>`` by the spectrum route (a cost function of many Z terms):
        the per-mask values never leave the device, only the sum does."""
        self.ctx.bind_stream()
        T = engine.torch()
        zs = masks_array(masks, self.N)
        w = np.ascontiguousarray(np.asarray(weights.cpu() if hasattr(weights, "cpu") else weights, dtype=np.float64))
        if w.ndim != 1 or len(w) != len(zs):
            raise ValueError(f"{len(zs)} masks but weights of shape {w.shape}")
        if not len(zs):
            return 0.0
        if not self.frags:
            return float(self._scalar * w.sum())
        dev = T.device("cuda", self.device)
        acc = T.zeros((), dtype=T.float64, device=dev)
        for s, vals in self._spectrum_chunks(zs):
            acc += T.dot(vals, T.from_numpy(w[s:s + vals.numel()]).to(dev))
        return float(acc)

    def correlations(self, clbits=None) -> np.ndarray:
        """numpy ``[k, k]``: entry ``(i, j)`` is ``<Z_clbits[i] Z_clbits[j]>``, the diagonal ``<Z_clbits[i]>``;
        symmetric. ``None``: all clbits. The ``k (k + 1) / 2`` strings go through the spectrum route."""
        cl = self._clbits(clbits)
        k = len(cl)
        iu, ju = np.triu_indices(k)
        bit = np.left_shift(np.int64(1), np.asarray(cl, dtype=np.int64))
        vals = self._expectation_spectrum(bit[iu] | bit[ju])
        out = np.zeros((k, k))
        out[iu, ju] = vals
        out[ju, iu] = vals
        return out

    def sample(self, shots: int, seed: int = 0, clbits=None):
        """``shots`` measurement outcomes of the exact knit: device int64 ``[shots]`` of keys in draw
        order, bit ``i`` of a key = ``clbits[i]`` (``None``: all clbits, bit i = clbit i). Drawn fragment
        by fragment (``qk_sample_rows``, DESIGN.md §4a "Shots"): step f draws fragment f's outcome from
        ``max(sum_k c[k] t_f[k] X_f[k][x], 0)`` with ``u(seed, f, shot)``, ``c`` the product of the earlier
        fragments' columns at their drawn outcomes and ``t_f`` the later fragments' row sums. A pure
        function of (circuit, seed, shot index): nothing of size 2^N is formed. ``RuntimeError`` if a
        conditional distribution has no positive weight."""
        self.ctx.bind_stream()
        T = engine.torch()
        dev = T.device("cuda", self.device)
        shots = check_not_negative("shots", shots)
        cl = self._clbits(clbits)
        keys = T.zeros(shots, dtype=T.int64, device=dev)
        if shots == 0 or not self.frags:
            return keys
        mats, where, _ = self._keyed_operands(cl)  # X_f [K, 2^k_f]
        sums = [engine.reduce_bits(self.ctx, X, len(pos), 0, [0])[:, 0] for X, pos in zip(mats, where)]
        tails = [None] * len(mats)  # t_f[k] = prod_{g > f} s_g[k]
        tail = T.ones(mats[0].shape[0], dtype=T.float64, device=dev)
        for f in reversed(range(len(mats))):
            tails[f] = tail
            tail = tail * sums[f]
        c = T.ones((shots, mats[0].shape[0]), dtype=T.float64, device=dev)
        for f, (X, pos) in enumerate(zip(mats, where)):
            # shots with the same prefix share a row; a row's draws are in shot order
            _, inv, counts = T.unique(keys, return_inverse=True, return_counts=True)
            by_row = T.argsort(inv, stable=True)
            draw_off = T.zeros(counts.numel() + 1, dtype=T.int64, device=dev)
            T.cumsum(counts, 0, out=draw_off[1:])
            C = c[by_row[draw_off[:-1]]] * tails[f]
            u = engine.uniforms(self.ctx, seed, f, 0, shots)[by_row]
            xs, _, _ = engine.sample_rows(self.ctx, X, C, draw_off, u, m=len(pos))
            if bool((xs < 0).any()):
                raise RuntimeError(f"fragment {f}: a conditional distribution of the knit has no positive weight")
            x = T.empty_like(xs)
            x[by_row] = xs
            c = c * X[:, x].T
            keys = deposit_bits(keys, x, pos)
        return keys

    # -- the knit at chosen keys ----------------------------------------------------------------
    def _check_fragment_limit(self) -> None:
        if len(self.frags) > engine.KNIT_AT_MAX_FRAGMENTS:
            raise ValueError(f"{len(self.frags)} fragments: the lookup kernel (qk_knit_at) takes at most "
                             f"{engine.KNIT_AT_MAX_FRAGMENTS}")

    def _device_keys(self, ks):
        T = engine.torch()
        dev = T.device("cuda", self.device)
        return (T.from_numpy(ks) if isinstance(ks, np.ndarray) else ks).to(dev)

    def transposed_operands(self) -> list:
        """Per fragment the device tensor ``Xt_f [2^m_f, ldt]``: its unreduced operand ``X_f`` transposed
        (``qk_transpose_rows``; ``ldt`` = the terms rounded up to 16, zero padded), so the factors a key takes
        from a fragment are one contiguous row. Formed on first use and kept, like :meth:`z_spectrum` (as
        much memory again as the operands; read-only)."""
        if self._transposed is None:
            self.ctx.bind_stream()
            mats = engine.fragment_operands(self.ctx, self.ops, self.qs) if self.frags else []
            self._transposed = [engine.transpose_rows(self.ctx, X, len(fcl)) for X, fcl in zip(mats, self.clbits)]
        return self._transposed

    def probabilities(self, keys, clbits=None):
        """Device fp64 tensor ``[M]``: the exact knit ``R[key]`` at the given keys (the quasi-distribution
        itself: no clamp, no projection), without the 2^N output: a gather of one row per fragment and key
        from the transposed operands (``qk_knit_at``, DESIGN.md §4a "Probabilities at chosen keys").
        ``keys``: ints, a list, an integer numpy array or an int64 tensor (a device tensor stays on the
        device; :func:`keys_array`). Bit ``i`` of a key is ``clbits[i]`` (``None``: all clbits, bit i = clbit i);
        with chosen ``clbits`` the result is the marginal onto them at the keys: the rows are reduced first,
        as in :meth:`sample`. A key with a bit set on a clbit that no fragment measures has probability 0."""
        self.ctx.bind_stream()
        T = engine.torch()
        cl = self._clbits(clbits)
        ks = self._device_keys(keys_array(keys, len(cl)))
        if not self.frags:
            return (ks == 0).to(T.float64) * self._scalar
        self._check_fragment_limit()
        if cl == list(range(self.N)):
            Xts, where = self.transposed_operands(), self.clbits
        else:
            mats, where, _ = self._keyed_operands(cl)
            Xts = [engine.transpose_rows(self.ctx, X, len(pos)) for X, pos in zip(mats, where)]
        dead = ((1 << len(cl)) - 1) & ~sum(1 << b for pos in where for b in pos)
        return engine.knit_at(self.ctx, Xts, where, ks, dead)

    def linear_xeb(self, keys, clbits=None) -> float:
        """Linear cross-entropy benchmarking score of the sampled ``keys`` against the exact knit:
        ``D * mean_j R[key_j] - 1`` with ``D = 2^(number of the chosen clbits that some fragment measures)``.
        The mean is taken on the device; only the scalar leaves it. Arguments as :meth:`probabilities`."""
        p = self.probabilities(keys, clbits)
        if not p.numel():
            raise ValueError("linear_xeb needs at least one key")
        return float(p.mean()) * 2.0 ** self._measured_among(clbits) - 1.0

    def fidelity_to_counts(self, counts: dict, clbits=None) -> float:
        """Hellinger fidelity between the knit and a counts dict ``{key: count}`` (shots of an uncut run or
        of a device), from the knit at the observed keys alone:
        ``(sum_key sqrt(max(R[key], 0) * count / shots))^2 / mass`` with ``mass = expectation([0])``. The knit is
        normalised by its signed total ``mass``, as ``fidelity.hellinger_fidelity`` normalises a dict by the
        plain sum of its values, not by the total of its clipped entries; the two normalisations differ by
        the knit's negative mass, which is rounding for exact instances."""
        T = engine.torch()
        if not counts:
            raise ValueError("fidelity_to_counts needs at least one key")
        p = self.probabilities(list(counts), clbits)
        c = T.tensor([float(v) for v in counts.values()], dtype=T.float64, device=p.device)
        mass = float(self.expectation([0])[0])
        return float((p.clamp(min=0.0) * (c / c.sum())).sqrt().sum()) ** 2 / mass

    def _expectation_fused(self, masks) -> np.ndarray:
        self.ctx.bind_stream()
        on_device = _is_tensor(masks) and masks.is_cuda
        ks = keys_array(masks, self.N) if on_device else masks_array(masks, self.N)  # device masks stay there
        if not self.frags:
            return np.full(len(ks), self._scalar) if len(ks) else np.zeros(0)
        self._check_fragment_limit()
        if self._spectrum_t is None:
            self._spectrum_t = [engine.transpose_rows(self.ctx, H, len(fcl))
                                for H, fcl in zip(self.z_spectrum(), self.clbits)]
        # a Z on a clbit nobody measures is +1: its bit is not read, and no key is dead
        return engine.knit_at(self.ctx, self._spectrum_t, self.clbits, self._device_keys(ks), 0).cpu().numpy()

    # -- second moments: overlaps of knits --------------------------------------------------------
    def _moment_sides(self, cl: list) -> tuple:
        """``(rows, specs, clbits, K)`` for :func:`overlap_of_sides`: per fragment its swept rows reduced onto the
        kept clbits ``[R_f, 2^k_f]``, how its operand follows from them (``("T", W^T [R_f, K])`` or
        ``("G", rows [K], coefs [K])``, on the device: uploaded on first use and kept), and its clbits. No
        fragment at all is one ``m = 0`` fragment whose single row holds ``_scalar``."""
        T = engine.torch()
        dev = T.device("cuda", self.device)
        if not self.frags:
            one = T.full((1, 1), self._scalar, dtype=T.float64, device=dev)
            return [one], [_ones_spec(T, dev, 1)], [[]], 1
        if self._moment_specs is None:
            specs = []
            for W, rows, coefs in zip(self.ops.transforms, self.ops.rows, self.ops.coefs):
                if W is not None:
                    specs.append(("T", T.from_numpy(np.ascontiguousarray(W.T)).to(dev)))
                else:
                    specs.append(("G", T.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev),
                                  T.from_numpy(np.ascontiguousarray(coefs, dtype=np.float64)).to(dev)))
            self._moment_specs = specs
        keep, _ = split_clbits(cl, self.clbits)
        return self._reduced(keep), self._moment_specs, self.clbits, self.ops.num_terms

    def overlap(self, other=None, clbits=None) -> float:
        """``sum_y R_S[y] R'_S[y]``: the overlap of this knit's marginal onto ``clbits`` (``None``: all clbits)
        with that of ``other`` (another reducer on the same device with as many clbits; ``None``: itself),
        without either output (DESIGN.md §4a "Second moments"). The clbit supports of the fragments are
        disjoint, so the sum is ``sum_{k, k'} prod_f G_f[k, k']`` with ``G_f = X_f X'_f^T``: per fragment the
        swept rows are reduced onto the kept clbits (``qk_reduce_bits``), their cross-Gram is one
        ``qk_gram_rows`` and ``G_f`` follows through the two transforms (or row gathers); the product over
        the fragments and the sum over ``(k, k')`` run in row blocks of at most ``MOMENT_WORK_BYTES``.
        Restricted to ``clbits`` the fragments of the two reducers must measure the same sets of clbits, in
        any order (:func:`match_fragments`; ``ValueError`` otherwise); a fragment with no kept clbit enters
        with its row sums. Every sum has a fixed order: two calls return the same float."""
        self.ctx.bind_stream()
        same = other is None or other is self
        if not same:
            self._check_other(other)
        cl = self._clbits(clbits)
        return overlap_of_sides(self.ctx, self._moment_sides(cl), None if same else other._moment_sides(cl), cl)

    def collision_probability(self, clbits=None) -> float:
        """``sum_y R_S[y]^2`` of the marginal onto ``clbits`` (``None``: all): :meth:`overlap` with itself."""
        return self.overlap(None, clbits)

    def renyi2_entropy(self, clbits=None) -> float:
        """The Rényi-2 entropy ``-log2(sum_y p[y]^2)`` in bits of ``p = R_S / mass``, the marginal onto
        ``clbits`` normalised by the knit's signed total ``mass = expectation([0])[0]`` (as
        :meth:`fidelity_to_counts` normalises)."""
        mass = float(self.expectation([0])[0])
        return float(-np.log2(self.collision_probability(clbits) / mass ** 2))

    def ideal_xeb(self, clbits=None) -> float:
        """The linear XEB score an ideal sampler of this knit would reach in expectation:
        ``D * sum_y R_S[y]^2 - 1`` with ``D`` as in :meth:`linear_xeb`; about 1 for a Porter-Thomas output."""
        return self.collision_probability(clbits) * 2.0 ** self._measured_among(clbits) - 1.0

    def l2_distance(self, other, clbits=None) -> float:
        """``||R_S - R'_S||_2 = sqrt(max(s_aa - 2 s_ab + s_bb, 0))`` from three overlaps. The three sums cancel:
        a distance below about ``sqrt(2^-52 * (s_aa + s_bb))`` is rounding, whatever it reads."""
        s_ab = self.overlap(other, clbits)  # first: it checks other and the pairing
        s_aa, s_bb = self.overlap(None, clbits), other.overlap(None, clbits)
        return float(np.sqrt(max(s_aa - 2.0 * s_ab + s_bb, 0.0)))

    def mutual_information2(self, a, b) -> float:
        """``S2(a) + S2(b) - S2(a + b)`` in bits for two disjoint lists of clbits (:meth:`renyi2_entropy`)."""
        a, b = check_clbits(a, self.N), check_clbits(b, self.N)
        if set(a) & set(b):
            raise ValueError(f"clbits {sorted(set(a) & set(b))} in both lists")
        return self.renyi2_entropy(a) + self.renyi2_entropy(b) - self.renyi2_entropy(a + b)

    # -- nonlinear functionals: the streamed scan ------------------------------------------------
    def _scan_operands(self, cl: list, other=None) -> ScanSides:
        """The two sides of the scan of the marginal onto ``cl`` (:func:`scan_sides` of the fragments' kept widths).
        ``other``: also the same sides of another reducer's knit, its fragments paired by :func:`match_fragments` and
        permuted to this one's bit order."""
        T = engine.torch()
        dev = T.device("cuda", self.device)
        mats, where, K = self._keyed_operands(cl)
        sa, sb = scan_sides([len(w) for w in where])
        sides = ScanSides(A=_side_operand(self.ctx, [mats[f] for f in sa], K, dev),
                          B=_side_operand(self.ctx, [mats[f] for f in sb], K, dev),
                          where_a=[b for f in sa for b in where[f]], where_b=[b for f in sb for b in where[f]])
        if other is None:
            return sides
        pairs, _, only_o = match_fragments(self.clbits if self.frags else [[]], other.clbits if other.frags else [[]], cl)
        omats, _, K2 = other._keyed_operands(cl)
        partner = {f: _permute_bits(T, omats[g], order) for f, g, order in pairs}
        extra = [omats[g] for g in only_o]  # no kept clbit: they scale side A
        return sides._replace(A2=_side_operand(self.ctx, [partner[f] for f in sa if f in partner] + extra, K2, dev),
                              B2=_side_operand(self.ctx, [partner[f] for f in sb if f in partner], K2, dev))

    def scan(self, clbits=None, *, threshold: float = 0.0, entropy: bool = True) -> KnitScan:
        """Statistics of the exact knit ``R`` (``clbits``: of its marginal onto them, bit ``i`` of a key =
        ``clbits[i]``) that do not factorise over the fragments, without its 2^N output: the knit is formed tile by
        tile on the matrix cores and consumed in registers (``qk_knit_scan``, DESIGN.md §4a "Nonlinear
        functionals"). ``threshold``: ``count_above`` counts ``R > threshold``. ``entropy=False`` skips the
        logarithm (``shannon_entropy`` is then nan). Keys with a bit set on a clbit that no fragment measures hold
        exact zeros: they are not scanned but enter ``min`` / ``max`` / ``count_above`` as such. Deterministic: two
        calls return the same values."""
        self.ctx.bind_stream()
        cl = self._clbits(clbits)
        sides = self._scan_operands(cl)
        st = engine.knit_scan(self.ctx, sides.A, sides.B, tau=threshold, entropy=entropy, hist=True)
        P = st["pos"]
        H = (st["ent"] / P + np.log(P)) / np.log(2.0) if entropy and P > 0 else float("nan")
        # key bits that no fragment measures: every key with one of them set holds an exact zero
        scanned = sides.where_a + sides.where_b
        dead = [b for b in range(len(cl)) if b not in scanned]
        if dead:
            zero_key = 1 << dead[0]  # the lowest such key
            if threshold < 0:
                st["count_tau"] += ((1 << len(dead)) - 1) << len(scanned)
            if st["max"] < 0:
                st["max"], st["argmax"] = 0.0, None
            if st["min"] > 0:
                st["min"], st["argmin"] = 0.0, None
        key = lambda flat: zero_key if flat is None else int(sides.key(flat))
        return KnitScan(mass=st["sum"], l1=st["abs"], positive_mass=P, negativity=(st["abs"] - st["sum"]) / 2,
                        collision=st["sq"], shannon_entropy=float(H), max=st["max"],
                        argmax=key(st["argmax"]), min=st["min"],
                        argmin=key(st["argmin"]), count_above=st["count_tau"],
                        support=st["count_pos"], histogram=st["hist"])

    def shannon_entropy(self, clbits=None) -> float:
        """The Shannon entropy in bits of ``p = max(R_S, 0) / sum max(R_S, 0)`` (:meth:`scan`)."""
        return self.scan(clbits).shannon_entropy

    def negativity(self, clbits=None) -> float:
        """The negative mass ``(sum |R_S| - sum R_S) / 2`` of the quasi-distribution (:meth:`scan`)."""
        return self.scan(clbits, entropy=False).negativity

    def mode(self, clbits=None) -> tuple:
        """``(key, value)`` of the most probable outcome, the lowest flat index among equal values (:meth:`scan`)."""
        sc = self.scan(clbits, entropy=False)
        return sc.argmax, sc.max

    def _collect_sorted(self, sides: ScanSides, tau: float, capacity: int):
        T = engine.torch()
        idx, vals, count = engine.knit_collect(self.ctx, sides.A, sides.B, tau, capacity)
        if count > capacity:
            raise ValueError(f"{count} outcomes above {tau!r}, more than capacity = {capacity}")
        keys, by_key = T.sort(sides.key(idx))
        vals, by_val = T.sort(vals[by_key], descending=True, stable=True)  # ties stay in key order
        return keys[by_val], vals

    def _outputs_above(self, tau: float, cl: list, capacity: int) -> tuple:
        """What :meth:`heavy_outputs` and :meth:`projected_heavy_outputs` share: the sorted outcomes above ``tau``."""
        self.ctx.bind_stream()
        return self._collect_sorted(self._scan_operands(cl), tau, int(capacity))

    def _largest(self, k: int, cl: list, capacity: int, lower: float = 0.0, above_lower: int = 0) -> tuple:
        """What :meth:`top_k` and :meth:`projected_top_k` share: the ``k`` largest outcomes above ``lower``, of which
        there are ``above_lower``. The histogram's threshold is never negative, so :meth:`top_k`'s ``lower = 0`` never
        replaces it."""
        self.ctx.bind_stream()
        k = check_not_negative("k", k)
        sides = self._scan_operands(cl)
        st = engine.knit_scan(self.ctx, sides.A, sides.B, hist=True)
        tau, count = histogram_threshold(st["hist"], k)
        if tau < lower:
            tau, count = lower, above_lower
        if count > capacity:
            raise ValueError(f"{count} outcomes share the binades of the top {k}, more than capacity = {capacity}")
        keys, vals = self._collect_sorted(sides, tau, count)
        return keys[:k], vals[:k]

    def heavy_outputs(self, threshold: float, clbits=None, capacity: int = 1 << 24) -> tuple:
        """Device ``(keys int64, values float64)`` of every outcome with ``R_S > threshold`` (strict), sorted by
        value descending, ties by key ascending (``qk_knit_collect``). ``threshold >= 0``: a key on a clbit that no
        fragment measures holds a zero and is never listed. ``ValueError``, naming the count, when more than
        ``capacity`` outcomes qualify."""
        return self._outputs_above(check_not_negative("threshold", threshold, float), self._clbits(clbits), capacity)

    def top_k(self, k: int, clbits=None, capacity: int = 1 << 24) -> tuple:
        """Device ``(keys, values)`` of the ``k`` most probable outcomes (fewer when fewer are positive), sorted as
        :meth:`heavy_outputs`: one scan with the histogram, then :func:`histogram_threshold` gives a threshold whose
        count is known before anything is collected. ``ValueError``, naming the count, when the binade that holds
        the ``k``-th value makes that count exceed ``capacity`` (a uniform output, say)."""
        return self._largest(k, self._clbits(clbits), capacity)

    def _pair_scan(self, other, clbits) -> dict:
        self._check_other(other)
        self.ctx.bind_stream()
        sides = self._scan_operands(self._clbits(clbits), other)
        return engine.knit_scan(self.ctx, sides.A, sides.B, sides.A2, sides.B2)

    def hellinger_fidelity(self, other, clbits=None) -> float:
        """The Hellinger fidelity ``(sum sqrt(p q))^2 / (sum p sum q)`` of ``p = max(R_S, 0)`` and
        ``q = max(R'_S, 0)``, the two knits clipped (the normalisation of ``engine.fidelity_from_sums``), without
        either output: one pair scan. ``other``: a reducer with the same clbits whose fragments cut ``clbits`` as
        this one's do (:func:`match_fragments`; ``ValueError`` otherwise)."""
        st = self._pair_scan(other, clbits)
        return engine.fidelity_from_sums(st["hell"], st["pos"], st["pos2"])

    def total_variation(self, other, clbits=None) -> float:
        """``sum |R_S - R'_S| / 2`` (one pair scan; arguments as :meth:`hellinger_fidelity`)."""
        return self._pair_scan(other, clbits)["l1d"] / 2

    def max_difference(self, other, clbits=None) -> float:
        """``max |R_S - R'_S|`` (one pair scan; arguments as :meth:`hellinger_fidelity`)."""
        return self._pair_scan(other, clbits)["maxd"]

    # -- the nearest probability distribution ---------------------------------------------------
    def project(self, clbits=None, *, accuracy: float = 0.0, max_passes: int = 32) -> KnitProjection:
        """The nearest probability distribution of the knit (``clbits``: of its marginal onto them), the reference's
        ``nearest_probability_distribution`` of the entries with ``|R| > accuracy``, without the 2^N output: the
        threshold by :func:`projection_threshold`, one ``qk_knit_project_scan`` pass per step (DESIGN.md §4a
        "Nearest probability distribution"). Keys on clbits that no fragment measures hold exact zeros and are never
        members. With no fragment at all there is one outcome at key 0."""
        self.ctx.bind_stream()
        cl = self._clbits(clbits)
        _, _, accuracy = engine.check_projection_args(0.0, 0.0, accuracy)
        sides = self._scan_operands(cl)
        seen = {}

        def evaluate(theta):
            seen.update(engine.knit_project_scan(self.ctx, sides.A, sides.B, theta=theta, accuracy=accuracy))
            return seen["msum"], seen["tsum"], seen["nkept"]

        th = projection_threshold(evaluate, max_passes)
        return KnitProjection(theta=th.theta, accuracy=accuracy, mass=th.msum, kept=th.kept, members=seen["nmember"],
                              dropped_mass=th.msum - th.tsum, passes=th.passes, clbits=cl)

    @staticmethod
    def _check_projection(projection) -> float:
        """The lower bound ``max(theta, accuracy)`` of a projection's kept entries."""
        if not isinstance(projection, KnitProjection):
            raise ValueError("projection must be a KnitProjection (KnitReducer.project)")
        theta, _, accuracy = engine.check_projection_args(projection.theta, 0.0, projection.accuracy)
        return max(theta, accuracy)

    def projected_probabilities(self, keys, projection: KnitProjection):
        """Device fp64 ``[M]``: the projection at the given keys, :meth:`probabilities` (over the projection's
        clbits) mapped through ``R > max(theta, accuracy) ? R - theta : 0`` on the device."""
        lower = self._check_projection(projection)
        R = self.probabilities(keys, projection.clbits)
        T = engine.torch()
        return T.where(R > lower, R - projection.theta, T.zeros_like(R))

    def projected_scan(self, projection: KnitProjection, *, entropy: bool = True) -> ProjectedScan:
        """Statistics of the projection: one ``qk_knit_project_scan`` pass at the final threshold (with
        ``entropy``, one more launch of the mainloop for the logarithms)."""
        self._check_projection(projection)
        self.ctx.bind_stream()
        sides = self._scan_operands(projection.clbits)
        st = engine.knit_project_scan(self.ctx, sides.A, sides.B, theta=projection.theta, accuracy=projection.accuracy,
                                      entropy=entropy)
        P = st["psum"]
        H = (st["pent"] / P + np.log(P)) / np.log(2.0) if entropy and st["nkept"] and P > 0 else float("nan")
        key = int(sides.key(st["argmax"])) if st["nkept"] else None
        return ProjectedScan(mass=P, collision=st["psq"], shannon_entropy=float(H), max=st["pmax"], argmax=key,
                             support=st["nkept"])

    def projected_heavy_outputs(self, projection: KnitProjection, min_value: float = 0.0,
                                capacity: int = 1 << 24) -> tuple:
        """Device ``(keys, values)`` of every entry of the projection with a value above ``min_value >= 0``
        (strict; 0: every kept entry), sorted as :meth:`heavy_outputs`: ``qk_knit_collect`` at
        ``max(theta, accuracy, theta + min_value)``, then the shift. ``ValueError``, naming the count, when more
        than ``capacity`` entries qualify."""
        lower = self._check_projection(projection)
        tau = max(lower, projection.theta + check_not_negative("min_value", min_value, float))
        keys, vals = self._outputs_above(tau, projection.clbits, capacity)
        return keys, vals - projection.theta

    def projected_top_k(self, k: int, projection: KnitProjection, capacity: int = 1 << 24) -> tuple:
        """Device ``(keys, values)`` of the ``k`` largest entries of the projection (fewer when fewer are kept),
        sorted as :meth:`heavy_outputs`: the route of :meth:`top_k` with its threshold raised to the kept set's
        (the shift leaves the order of the entries as it is)."""
        lower = self._check_projection(projection)
        keys, vals = self._largest(k, projection.clbits, capacity, lower, projection.kept)
        return keys, vals - projection.theta

    def _projected_pair_scan(self, other, projection, other_projection, clbits) -> dict:
        self._check_projection(projection)
        self._check_projection(other_projection)
        cl = list(projection.clbits) if clbits is None else check_clbits(clbits, self.N)
        if cl != list(projection.clbits) or cl != list(other_projection.clbits):
            raise ValueError(f"the projections are over clbits {projection.clbits} and {other_projection.clbits}, "
                             f"the comparison over {cl}")
        if projection.accuracy != other_projection.accuracy:
            raise ValueError(f"the projections were truncated at {projection.accuracy} and "
                             f"{other_projection.accuracy}: one pass takes one accuracy")
        self._check_other(other)
        self.ctx.bind_stream()
        sides = self._scan_operands(cl, other)
        return engine.knit_project_scan(self.ctx, sides.A, sides.B, sides.A2, sides.B2, theta=projection.theta,
                                        theta2=other_projection.theta, accuracy=projection.accuracy)

    def projected_hellinger_fidelity(self, other, projection: KnitProjection, other_projection: KnitProjection,
                                     clbits=None) -> float:
        """The Hellinger fidelity ``(sum sqrt(p p'))^2 / (sum p sum p')`` of the two knits' projections (the
        reference's ``cutVsUncutFidelity`` on what it compares), without either output: one pair pass. ``other``
        as for :meth:`hellinger_fidelity`; ``projection`` / ``other_projection``: :meth:`project` of this reducer
        and of ``other`` over the same clbits (``clbits``, when given, must be those) and accuracy. 0.0 when either
        projection is empty."""
        st = self._projected_pair_scan(other, projection, other_projection, clbits)
        return engine.fidelity_from_sums(st["hell"], st["psum"], st["psum2"])

    def projected_total_variation(self, other, projection: KnitProjection, other_projection: KnitProjection,
                                  clbits=None) -> float:
        """``sum |p - p'| / 2`` of the two projections (one pair pass; arguments as
        :meth:`projected_hellinger_fidelity`)."""
        return self._projected_pair_scan(other, projection, other_projection, clbits)["l1d"] / 2

    # -- the projection as a distribution -------------------------------------------------------
    def _tile_masses(self, A, B, projection: KnitProjection, pairs: list) -> list:
        """Per slab of side A the device ``W [len(pairs), tiles]`` of ``qk_knit_project_tiles``."""
        ma, mb = A.shape[1].bit_length() - 1, B.shape[1].bit_length() - 1
        return [engine.knit_project_tiles(self.ctx, A, B, projection.theta, projection.accuracy, pairs, i0, i1)
                for i0, i1 in engine.scan_slabs(ma, mb)]

    def projected_expectation(self, masks, projection: KnitProjection) -> np.ndarray:
        """float64 ``[M]``: ``sum_key (-1)^popcount(key & mask) p[key]`` of the projection ``p`` (:meth:`project`)
        per Z string; masks as for :meth:`expectation` (ints, ``'IZ'`` strings, an integer array or tensor) over
        the circuit's clbits, every bit within ``projection.clbits``. ``p`` is not multilinear in the fragments: each
        pass forms all its outcomes (``qk_knit_project_tiles``, DESIGN.md §4a "The projection as a distribution")
        and answers up to ``PROJ_TILE_MASKS`` masks, fewer where the tile masses of a pass would exceed
        ``PROJ_TILE_BYTES``. A bit on a clbit that no fragment measures is dropped. A mask's tile masses are added as
        one vector per slab (a fixed association for a given shape), the slabs ascending on the host."""
        self._check_projection(projection)
        self.ctx.bind_stream()
        T = engine.torch()
        cl = list(projection.clbits)
        zs = masks_array(masks, self.N)
        held = sum(1 << c for c in cl)
        for z in zs:
            if int(z) & ~held:
                raise ValueError(f"mask {int(z):#x} has a bit outside the projection's clbits {cl}")
        out = np.zeros(len(zs))
        if not len(zs):
            return out
        sides = self._scan_operands(cl)
        side = lambda z, w: sum(1 << i for i, b in enumerate(w) if z >> cl[b] & 1)
        pairs = [(side(int(z), sides.where_a), side(int(z), sides.where_b)) for z in zs]
        ma, mb = len(sides.where_a), len(sides.where_b)
        tiles = sum(scan_shape(ma, mb, i0, i1)["tiles"] for i0, i1 in engine.scan_slabs(ma, mb))
        per = max(1, min(PROJ_TILE_MASKS, PROJ_TILE_BYTES // (8 * tiles)))
        for c0 in range(0, len(pairs), per):
            chunk = pairs[c0:c0 + per]
            sums = [T.stack([W[m].sum() for m in range(len(chunk))])
                    for W in self._tile_masses(sides.A, sides.B, projection, chunk)]
            out[c0:c0 + len(chunk)] = engine.sum_slabs(T.stack(sums).cpu().numpy())
        return out

    def projected_marginal(self, clbits, projection: KnitProjection, *, route: str | None = None):
        """Device fp64 ``[2^k]``: the projection summed over every clbit but ``clbits`` (a subset of
        ``projection.clbits``; bit ``i`` of the index is ``clbits[i]``): the marginal of the nearest probability
        distribution, not the nearest probability distribution of the marginal (``project(clbits)``).
        ``route="tile"``: each side's columns are permuted so that its kept bits are the top bits of its index; with
        at most ``max(side bits - 7, 0)`` kept bits per side every 128 x 128 tile lies in one cell and the marginal
        is the sum of the plain tile masses per cell: one pass. ``route="mask"``: for ``k <=
        PROJ_MARGINAL_MASK_BITS``, the ``2^k`` :meth:`projected_expectation` values of the masks inside ``clbits``
        and their inverse Walsh-Hadamard transform (:func:`inverse_wht_marginal`): ``2^k / 8`` passes. ``None``: the
        tile route where it applies, else the mask route, else ``ValueError``. The routes agree to rounding."""
        self._check_projection(projection)
        self.ctx.bind_stream()
        T = engine.torch()
        dev = T.device("cuda", self.device)
        cl, pcl = check_clbits(clbits, self.N), list(projection.clbits)
        if set(cl) - set(pcl):
            raise ValueError(f"clbits {sorted(set(cl) - set(pcl))} are not among the projection's {pcl}")
        if route not in (None, "tile", "mask"):
            raise ValueError(f"route must be None, 'tile' or 'mask', not {route!r}")
        k = len(cl)
        sides = self._scan_operands(pcl)
        A, B, wa, wb = sides.A, sides.B, sides.where_a, sides.where_b
        ma, mb = len(wa), len(wb)
        want = {pcl.index(c): i for i, c in enumerate(cl)}  # key bit of the projection -> bit of the result
        ka, kb = [i for i, b in enumerate(wa) if b in want], [i for i, b in enumerate(wb) if b in want]
        tile_ok = len(ka) <= max(ma - 7, 0) and len(kb) <= max(mb - 7, 0)
        if route == "tile" and not tile_ok:
            raise ValueError(f"the tile route keeps at most max(side bits - 7, 0) bits per side: {len(ka)} of {ma} and "
                             f"{len(kb)} of {mb} here")
        if route == "mask" and k > PROJ_MARGINAL_MASK_BITS:
            raise ValueError(f"the mask route takes at most {PROJ_MARGINAL_MASK_BITS} clbits, not {k}")
        if route is None and not tile_ok and k > PROJ_MARGINAL_MASK_BITS:
            raise ValueError(f"{k} clbits: the tile route keeps at most max(side bits - 7, 0) bits per side ({len(ka)} "
                             f"of {ma} and {len(kb)} of {mb} here), the mask route at most {PROJ_MARGINAL_MASK_BITS} "
                             f"clbits")
        if route == "mask" or (route is None and not tile_ok):
            masks = [sum(1 << c for i, c in enumerate(cl) if s >> i & 1) for s in range(1 << k)]
            return T.from_numpy(inverse_wht_marginal(self.projected_expectation(masks, projection))).to(dev)
        na, nb = len(ka), len(kb)
        A = _permute_bits(T, A, [i for i in range(ma) if i not in ka] + ka if na else None)
        B = _permute_bits(T, B, [i for i in range(mb) if i not in kb] + kb if nb else None)
        cells = T.zeros((1 << na, 1 << nb), dtype=T.float64, device=dev)
        gb = max(1, (1 << (mb - nb)) >> 7)  # tile columns per cell
        for (i0, i1), W in zip(engine.scan_slabs(ma, mb), self._tile_masses(A.contiguous(), B.contiguous(), projection,
                                                                           [(0, 0)])):
            tiles_m = -(-(i1 - i0) // 128)
            ga = min(tiles_m, max(1, (1 << (ma - na)) >> 7))  # tile rows per cell, within this slab
            first = i0 >> (ma - na)
            cells[first:first + tiles_m // ga] += W[0].view(tiles_m // ga, ga, 1 << nb, gb).sum(dim=(1, 3))
        y = T.arange(1 << k, dtype=T.int64, device=dev)
        ca = extract_bits(y, [want[wa[i]] for i in ka])
        cb = extract_bits(y, [want[wb[i]] for i in kb])
        dead = sum(1 << i for b, i in want.items() if b not in wa and b not in wb)  # nobody measures them: zeros
        return T.where((y & dead) == 0, cells[ca, cb], T.zeros((), dtype=T.float64, device=dev))

    def projected_sample(self, shots: int, projection: KnitProjection, seed: int = 0):
        """``shots`` outcomes distributed as the projection ``p / sum p``: device int64 ``[shots]`` of keys over
        ``projection.clbits`` in draw order. Inverse-CDF draws in (tile, walk) order (``qk_knit_project_tiles`` for
        the tile masses, then ``qk_knit_project_draw``: a draw forms the one tile it falls into again) with
        ``u = engine.uniforms(seed, PROJ_DRAW_LABEL, 0, shots)``: a pure function of (circuit, projection, seed, shot
        index), the first ``n`` shots of a longer run being an ``n``-shot run. Every key has ``p > 0``, which
        :meth:`sample`'s fragment-by-fragment chain does not give for a knit with negative entries.
        ``RuntimeError`` for an empty projection with ``shots > 0``."""
        self._check_projection(projection)
        self.ctx.bind_stream()
        T = engine.torch()
        dev = T.device("cuda", self.device)
        shots = check_not_negative("shots", shots)
        if shots == 0:
            return T.zeros(0, dtype=T.int64, device=dev)
        sides = self._scan_operands(list(projection.clbits))
        A, B = sides.A, sides.B
        slabs = engine.scan_slabs(len(sides.where_a), len(sides.where_b))
        Ws = [W[0] for W in self._tile_masses(A, B, projection, [(0, 0)])]
        u = engine.uniforms(self.ctx, seed, PROJ_DRAW_LABEL, 0, shots)
        draw = lambda s, us: engine.knit_project_draw(self.ctx, A, B, projection.theta, projection.accuracy, Ws[s], us,
                                                      *slabs[s])
        if len(slabs) == 1:
            flat, _, total = draw(0, u)
            if not total > 0:
                raise RuntimeError("the projection is empty: nothing to draw from")
        else:
            # the slab of a draw from the chain of the slabs' totals, then the draw within it at the rescaled u
            totals = np.array([draw(s, u[:0])[2] for s in range(len(slabs))])
            cum = np.cumsum(totals)  # a serial chain, ascending
            if not cum[-1] > 0:
                raise RuntimeError("the projection is empty: nothing to draw from")
            target = u * float(cum[-1])
            of = T.clamp(T.searchsorted(T.from_numpy(cum).to(dev), target, right=True), max=len(slabs) - 1)
            flat = T.empty(shots, dtype=T.int64, device=dev)
            for s in T.unique(of).tolist():
                sel = T.nonzero(of == s).reshape(-1)
                before = float(cum[s - 1]) if s else 0.0
                us = T.clamp((target[sel] - before) / float(totals[s]), 0.0, float(np.nextafter(1.0, 0.0)))
                flat[sel] = draw(s, us.contiguous())[0]
        if bool((flat < 0).any()):
            raise RuntimeError("the projection is empty: nothing to draw from")
        return sides.key(flat)

    def marginal_parity(self, clbits, masks):
        """The mixed form: device fp64 ``[M, 2^k]``, row j the marginal onto ``clbits`` of
        ``(-1)^popcount(key & masks[j]) R[key]``. A mask must not touch ``clbits``."""
        self.ctx.bind_stream()
        T = engine.torch()
        cl = check_clbits(clbits, self.N)
        zs = parse_masks(masks, self.N)
        held = sum(1 << c for c in cl)
        for z in zs:
            if z & held:
                raise ValueError(f"mask {z:#x} overlaps the kept clbits {sorted(cl)}")
        out = T.zeros((len(zs), 1 << len(cl)), dtype=T.float64, device=T.device("cuda", self.device))
        if not zs:
            return out
        keep, positions = split_clbits(cl, self.clbits)
        local = [list(col) for col in zip(*(split_mask(z, self.clbits) for z in zs))]  # per fragment, per mask
        mats = self._operands(keep, local)
        widths = [1 << len(p) for p in positions]
        for j in range(len(zs)):
            row = self._contract([a[:, j * w:(j + 1) * w] for a, w in zip(mats, widths)], positions, len(cl))
            out[j] = _user_order(T, row, cl)
        return out
