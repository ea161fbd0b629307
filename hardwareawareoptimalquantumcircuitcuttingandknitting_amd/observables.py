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

It builds on the direct path (``engine.prepare_fragments`` / ``sweep_fragment`` / ``knit_operands``
/ ``fragment_operands`` / ``contract``, as ``run._direct_dense``), not on the cached
``KnitPipeline``: the pipeline's row pruning rests on a per-entry bound on ``R`` and a marginal sums
up to ``2^(N-k)`` entries, so that bound does not carry over.
"""
from __future__ import annotations

import numpy as np

from . import engine
from .backend import MI355XBackend
from .knit_plan import LabelSpace

MAX_CLBITS = 62  # keys are int64


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


def _parity(x) -> int:
    return bin(int(x)).count("1") & 1


def reduce_bits_shape(rows: int, m: int, keep_mask: int, tile_bits: int = 10, min_groups: int = 256) -> dict:
    """The tile decomposition ``qk_reduce_bits`` uses for a shape (qknit_obs.hip: rb_make_shape)."""
    t = min(m, tile_bits)
    lo, hi = (1 << t) - 1, (1 << (m - t)) - 1
    keep_lo, drop_lo = keep_mask & lo, ~keep_mask & lo
    keep_hi, drop_hi = (keep_mask >> t) & hi, ~(keep_mask >> t) & hi
    klo, khi, dhi = bin(keep_lo).count("1"), bin(keep_hi).count("1"), bin(drop_hi).count("1")
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
                lane = np.array([_parity(int(x) & f) for x in xl])
                total = None
                for s in range(sh["split"]):
                    sub = pdep(s * chunk, sh["drop_hi"])
                    part = np.zeros(1 << klo)
                    for _ in range(chunk):
                        tile = base_hi | sub
                        neg = lane ^ _parity((tile << t) & f)
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
        if not self.frags:  # no fragment at all: the knit is the sum of the coefficients at key 0
            vg = [v.operation for v in virt.vgate_instructions]
            self._scalar = float(LabelSpace([g.num_instantiations for g in vg],
                                            [g.knit_coefficients() for g in vg]).coefficients().sum())

    # -- pieces ---------------------------------------------------------------------------------
    def _operands(self, keep: list, flips: list) -> list:
        """Per fragment ``[terms, len(flips[f]) * 2^k_f]``: its swept rows reduced, then transformed."""
        reds = []
        for q, fcl, kp, fl in zip(self.qs, self.clbits, keep, flips):
            m = len(fcl)
            if kp == (1 << m) - 1 and fl == [0]:  # nothing to sum out
                reds.append(q)
            else:
                reds.append(engine.reduce_bits(self.ctx, q, m, kp, fl))
        return engine.fragment_operands(self.ctx, self.ops, reds)

    def _contract(self, mats: list, positions: list, k: int):
        T = engine.torch()
        out = T.zeros(1 << k, dtype=T.float64, device=T.device("cuda", self.device))
        if not mats:
            out[0] = self._scalar
            return out
        return engine.contract(self.ctx, mats, positions, out)

    # -- public ---------------------------------------------------------------------------------
    def marginal(self, clbits):
        """Device fp64 tensor ``[2^k]`` of the exact knit summed over every other clbit; bit ``i`` of
        the index is ``clbits[i]``. A clbit no fragment measures is always 0."""
        self.ctx.bind_stream()
        cl = check_clbits(clbits, self.N)
        keep, positions = split_clbits(cl, self.clbits)
        mats = self._operands(keep, [[0]] * len(keep))
        return _user_order(engine.torch(), self._contract(mats, positions, len(cl)), cl)

    def expectation(self, masks) -> np.ndarray:
        """float64 ``[M]``: ``sum_key (-1)^popcount(key & mask) R[key]`` of the exact quasi-distribution
        (no projection onto the probability simplex) per mask; see :func:`parse_masks`."""
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
        shots = int(shots)
        if shots < 0:
            raise ValueError(f"shots must not be negative, not {shots}")
        cl = list(range(self.N)) if clbits is None else check_clbits(clbits, self.N)
        keys = T.zeros(shots, dtype=T.int64, device=dev)
        if shots == 0 or not self.frags:
            return keys
        keep, where = key_positions(cl, self.clbits)
        mats = self._operands(keep, [[0]] * len(keep))  # X_f [K, 2^k_f]
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
