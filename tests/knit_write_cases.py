"""The write-bound two-fragment knit (``qk_knit_outer_stream`` / ``qk_knit_outer_stream_range``): a plain
Python model of its dispatcher, the case table shared by the host and GPU tests, and the exact CPU
reference of the write.

Kinds (``qk_knit_outer_stream_kind``): 0 the per-output gather kernel, 1 the blocked kernel with A and B
staged in LDS, 2 the blocked kernel reading B from global memory, 3 the rows kernel (B runs in registers),
instantiated ``<1,13> <2,12> <4,11> <8,11>`` for K = 1 / 2 / 3..4 / 5..8."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

STAGE_BYTES = 24 * 1024  # LDS budget of the blocked kernel's operand stage
# both are read once per process by the dispatcher: a test of the default dispatch cannot run under them
PROCESS_ENV = ("QKNIT_OB_ROWS", "QKNIT_OB_BGLOBAL")
# read at every launch / query: they change the dispatch too, so the default-dispatch tests need them unset
LAUNCH_ENV = ("QKNIT_OB_TB", "QKNIT_OB_WG_PER_CU", "QKNIT_OB_SPREAD", "QKNIT_OR_SPREAD")


def dispatch_env_set() -> list:
    return [v for v in PROCESS_ENV + LAUNCH_ENV if v in os.environ]


def ctz(x: int) -> int:
    assert x != 0  # a negative x counts as two's complement (~mask)
    return (x & -x).bit_length() - 1


def mask_of(bits) -> int:
    return sum(1 << b for b in bits)


def model_rows_bits(K: int, mask_b: int, align: int) -> int:
    """log2 outputs per piece of the rows kernel, 0 when it does not apply: B must hold output bits
    0 .. want-1 and the range must be 2^want-aligned; want = 13 / 12 / 11 for K = 1 / 2 / >= 3."""
    low = ctz(~mask_b)  # contiguous B bits from bit 0
    want = 13 if K <= 1 else (12 if K <= 2 else 11)
    return want if (want <= low and want <= align) else 0


def model_blocked_tile(nbits: int, K: int, mask_a: int, mask_b: int, align: int, cap: int = 16):
    """(task_bits, b_global) of the blocked kernel, task_bits 0 when no task width fits: the widest tb in
    9 .. min(nbits, 16, align) whose stage fits 24 KiB, with A and B staged ("both") or A alone ("aonly");
    B from global when that alone allows tasks of >= 2^14 outputs."""
    top = min(nbits, 16, align, cap)
    both = aonly = 0
    for tb in range(top, 8, -1):
        low = (1 << tb) - 1
        sa = 8 * K << bin(mask_a & low).count("1")
        sb = 8 * K << bin(mask_b & low).count("1")
        if not aonly and sa <= STAGE_BYTES and mask_b & 1:
            aonly = tb
        if not both and sa + sb <= STAGE_BYTES:
            both = tb
    b_global = both < 14 and aonly >= 14 and aonly > both
    return (aonly if b_global else both), b_global


def model_kind(nbits: int, K: int, mask_a: int, mask_b: int, o_begin: int = 0, o_count: int | None = None,
               cap: int = 16):
    """(kind, task_bits) the dispatcher takes for outputs [o_begin, o_begin + o_count)."""
    if o_count is None:
        o_count = (1 << nbits) - o_begin
    align = ctz(o_begin | o_count)
    rc = model_rows_bits(K, mask_b, align)
    if rc:
        return 3, rc
    tb, bg = model_blocked_tile(nbits, K, mask_a, mask_b, align, cap)
    return ((2 if bg else 1) if tb else 0), tb


def rows_instantiation(K: int) -> str:
    return "<1,13>" if K <= 1 else "<2,12>" if K <= 2 else "<4,11>" if K <= 4 else "<8,11>"


@dataclass(frozen=True)
class Case:
    name: str
    nbits: int
    K: int
    bits_b: tuple
    kind: int
    task_bits: int

    @property
    def bits_a(self) -> tuple:
        return tuple(b for b in range(self.nbits) if b not in self.bits_b)

    @property
    def mask_a(self) -> int:
        return mask_of(self.bits_a)

    @property
    def mask_b(self) -> int:
        return mask_of(self.bits_b)

    @property
    def M(self) -> int:
        return 1 << len(self.bits_a)

    @property
    def N(self) -> int:
        return 1 << len(self.bits_b)

    @property
    def total(self) -> int:
        return 1 << self.nbits

    def with_k(self, K: int, name: str | None = None) -> "Case":
        kind, tb = model_kind(self.nbits, K, self.mask_a, self.mask_b)
        return Case(name or f"{self.name}@K{K}", self.nbits, K, self.bits_b, kind, tb)


def _r(*spans) -> tuple:
    out = []
    for s in spans:
        out += [s] if isinstance(s, int) else list(range(s[0], s[1] + 1))
    return tuple(out)


# name, nbits, K, bits_b, kind, task_bits: the full-range dispatch of each, as the library gives it
TABLE = (
    Case("stream2", 2, 1, (0,), 0, 0),
    Case("stream8", 8, 8, (0, 3, 4, 7), 0, 0),
    Case("blk9", 9, 8, (0, 2, 5, 6), 1, 9),
    Case("blk16", 16, 8, tuple(range(0, 16, 2)), 1, 15),
    Case("blk17", 17, 2, (0, 1, 2, 3, 8, 9, 10, 11, 16), 1, 16),
    Case("bg_k8", 18, 8, _r((0, 9), (11, 14)), 2, 16),
    Case("bg_k1", 18, 1, _r((0, 11), 14, 15), 2, 16),
    Case("bg_k2", 17, 2, _r((0, 10), (12, 15)), 2, 16),
    Case("rows_k1", 16, 1, _r((0, 12), 15), 3, 13),
    Case("rows_k2", 16, 2, _r((0, 11), 14), 3, 12),
    Case("rows_k3", 15, 3, _r((0, 10), 13), 3, 11),
    Case("rows_k4", 15, 4, _r((0, 10), 13), 3, 11),
    Case("rows_k5", 15, 5, _r((0, 10), 13), 3, 11),
    Case("rows_k8", 15, 8, _r((0, 10), 13), 3, 11),
    Case("old_last", 18, 8, _r((0, 13)), 3, 11),
)
# Further layouts (kinds from the model above; the host test holds the library to them as well):
#   stream13  the per-output kernel over several 512-output chunks (16: a grid-stride loop on a 1-CU stream):
#             K = 8 with B holding bits 0..8 stages 32 KiB of B at every task width, and A alone fits only
#             below 2^14, so no blocked form applies
#   blk_odd   the blocked kernel with K odd and no A bit inside a task: the B stage starts K (odd) doubles
#             into the LDS stage, off the 16-B alignment of its paired reads
EXTRA = (
    Case("stream13", 13, 8, _r((0, 8)), 0, 0),
    Case("blk_odd", 12, 3, _r((0, 9)), 1, 9),
)


def _modelled(name, nbits, K, bits_b) -> Case:
    bits_a = [b for b in range(nbits) if b not in bits_b]
    return Case(name, nbits, K, tuple(bits_b), *model_kind(nbits, K, mask_of(bits_a), mask_of(bits_b)))


# Layouts for CU-masked streams of 1 / 2 / 8 CUs, where the kernels' grids are small:
#   grid_blk      with the task width capped at 2^9 and one workgroup per CU: 512 tasks on <= 8 workgroups
#   grid_rows_k8  128 pieces over 4 B runs; B's bits 12 and 17 are not adjacent, so a workgroup's B run changes
#                 between its pieces (the register reload branch)
#   grid_rows_k1  the same for <1,13>: 128 pieces, 4 B runs
#   grid_rows_one 256 pieces over one B run: on 8 CUs the grid is 8 x (workgroups per CU, at most 8 of 256
#                 lanes), a multiple of 8 x the run count with >= 4 pieces per workgroup whatever the occupancy,
#                 so the rows kernel takes its 8-part piece order there
SMALL_GRID = (
    _modelled("grid_blk", 18, 2, range(0, 18, 2)),
    _modelled("grid_rows_k8", 18, 8, _r((0, 10), 12, 17)),
    _modelled("grid_rows_k1", 20, 1, _r((0, 12), 14, 19)),
    _modelled("grid_rows_one", 19, 8, _r((0, 10))),
)
GRID_ROWS = {"grid_rows_k8": (128, 4), "grid_rows_k1": (128, 4), "grid_rows_one": (256, 1)}  # name: (pieces, B runs)
# 32 output bits, written in range slices only (the whole write is 32 GiB): output offsets and task / piece bases
# past 2^31, where a 32-bit signed index would wrap. One layout per range-capable kind.
WIDE = (
    _modelled("wide_blk", 32, 2, range(0, 32, 2)),  # syc 32 5's kind of layout
    _modelled("wide_bg", 32, 8, _r((0, 9), (11, 14), 20, 25)),
    _modelled("wide_rows", 32, 1, _r((0, 15))),  # syc 32 1's layout
)
WIDE_KINDS = {"wide_blk": (1, 16), "wide_bg": (2, 16), "wide_rows": (3, 13)}
WIDE_RANGES = (((1 << 31) - (1 << 16), 1 << 17), ((1 << 32) - (1 << 16), 1 << 16))  # across 2^31; the last 2^16
CASES = {c.name: c for c in TABLE + EXTRA + SMALL_GRID + WIDE}

# name, o_begin, o_count, kind, task_bits
RANGE_TABLE = (
    ("rows_k1", 1 << 13, 1 << 13, 3, 13),
    ("rows_k1", 1 << 12, 1 << 12, 1, 11),  # the same masks reach two kernels
    ("rows_k8", 1 << 10, 3 << 10, 0, 0),  # no blocked task fits: the range entry refuses it
)

# the test_gpu.py parameters that write through qk_knit_outer_stream: (K, nbits, bits_b) -> (kind, task_bits)
LEGACY = {
    (1, 11, (0, 1, 2, 5, 6, 9)): (1, 11),
    (2, 11, (0, 3, 4, 5, 10)): (1, 11),
    (8, 11, (0, 1, 2, 3, 8, 9, 10)): (1, 11),
    (2, 3, (0, 2)): (0, 0),
    (3, 9, (0, 2, 5, 6)): (1, 9),
    (2, 17, (0, 1, 2, 3, 8, 9, 10, 11, 16)): (1, 16),
    (8, 18, tuple(range(14))): (3, 11),
    (3, 18, (0, 1, 2, 3, 8, 9, 10, 11, 16, 17)): (1, 16),
    (5, 20, tuple(range(0, 20, 2))): (1, 16),
}


def odd_partition(total: int, unit_bits: int) -> list:
    """(o_begin, o_count) pieces covering [0, total), every count an odd multiple of 2^unit_bits (1, 3, 5, ..
    units), so every piece's alignment ctz(o_begin | o_count) is exactly unit_bits."""
    units = total >> unit_bits
    assert units >= 1 and units << unit_bits == total
    sizes, left, nxt = [], units, 1
    while left > nxt:
        sizes.append(nxt)
        left -= nxt
        nxt += 2
    if left % 2 == 0:
        sizes += [1, left - 1]
    else:
        sizes.append(left)
    assert sum(sizes) == units and all(s % 2 == 1 for s in sizes)
    out, at = [], 0
    for s in sizes:
        out.append((at << unit_bits, s << unit_bits))
        at += s
    return out


# ----------------------------------------------------------------------------- operands and references
INT_BITS = 20  # |int| < 2^20
FRAC_BITS = 16  # operand = int / 2^16


def deposit(bits) -> np.ndarray:
    """key[x]: bit i of x -> bit bits[i] of the key (knit_plan.deposit_keys)."""
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.knit_plan import deposit_keys

    return deposit_keys(list(bits))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def int_operands(name: str):
    """(A_int [K, M], B_int [K, N]) int64, |.| < 2^20, fixed by the case name. As doubles (int / 2^16) every
    product is a multiple of 2^-32 below 2^8 and a sum of 8 stays below 2^11: 43 significant bits, exact in
    fp64 in any order, with or without fma."""
    c = CASES[name]
    rng = np.random.default_rng([c.nbits, c.K, c.mask_b & 0xFFFFFFFF, 20])
    lim = 1 << INT_BITS
    A = rng.integers(-lim + 1, lim, size=(c.K, c.M), dtype=np.int64)
    B = rng.integers(-lim + 1, lim, size=(c.K, c.N), dtype=np.int64)
    return _freeze(A, B)


@functools.lru_cache(maxsize=None)
def exact_write(name: str, k: int | None = None) -> np.ndarray:
    """The whole write [2^nbits] of the case's integer operands, first k terms (default all K): A_int^T B_int in
    int64, scattered through the deposit keys, times 2^-32 (exact: below 2^43 in those units)."""
    c = CASES[name]
    A, B = int_operands(name)
    k = c.K if k is None else k
    P = A[:k].T @ B[:k]  # int64, |.| < 8 * 2^40
    assert np.abs(P).max() < 1 << 43
    out = np.empty(c.total, dtype=np.int64)
    out[(deposit(c.bits_a)[:, None] + deposit(c.bits_b)[None, :]).reshape(-1)] = P.reshape(-1)
    return _freeze(out.astype(np.float64) * 2.0 ** (-2 * FRAC_BITS))


def pext(x: np.ndarray, mask: int) -> np.ndarray:
    """The bits of x under mask, packed in ascending order (a fragment's outcome index of an output)."""
    r, bit = np.zeros_like(x), 0
    for b in range(mask.bit_length()):
        if mask >> b & 1:
            r |= (x >> b & 1) << bit
            bit += 1
    return r


@functools.lru_cache(maxsize=None)
def exact_slice(name: str, o_begin: int, o_count: int, k: int | None = None) -> np.ndarray:
    """Outputs [o_begin, o_begin + o_count) of the case's integer operands by the definition
    out[o] = sum_k A[k][pext(o, maskA)] B[k][pext(o, maskB)], without forming the whole write."""
    c = CASES[name]
    A, B = int_operands(name)
    o = np.arange(o_begin, o_begin + o_count, dtype=np.int64)
    ia, ib = pext(o, c.mask_a), pext(o, c.mask_b)
    v = np.zeros(o_count, dtype=np.int64)
    for t in range(c.K if k is None else k):
        v += A[t, ia] * B[t, ib]
    return _freeze(v.astype(np.float64) * 2.0 ** (-2 * FRAC_BITS))


@functools.lru_cache(maxsize=None)
def normal_operands(name: str):
    c = CASES[name]
    rng = np.random.default_rng([c.nbits, c.K, c.mask_b & 0xFFFFFFFF, 1])
    return _freeze(rng.standard_normal((c.K, c.M)), rng.standard_normal((c.K, c.N)))


@functools.lru_cache(maxsize=None)
def normal_write(name: str):
    """(ref, band) [2^nbits] of the case's N(0,1) operands: the contraction in extended precision (math.fsum
    per entry where longdouble is no wider than double) and (K + 1) 2^-53 sum_k |A_k| |B_k|: the gamma_K bound
    of a K-term fma chain in any order plus one unit for the reference's own rounding."""
    import math

    c = CASES[name]
    A, B = normal_operands(name)
    if np.finfo(np.longdouble).nmant > 52:
        Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
        P = np.zeros((c.M, c.N), dtype=np.longdouble)
        S = np.zeros((c.M, c.N), dtype=np.longdouble)
        for k in range(c.K):
            P += Al[k][:, None] * Bl[k][None, :]
            S += np.abs(Al[k])[:, None] * np.abs(Bl[k])[None, :]
    else:
        # error-free products (Veltkamp split + Dekker: p + e == a * b exactly), summed exactly by fsum
        def split(x):
            t = 134217729.0 * x
            hi = t - (t - x)
            return hi, x - hi

        P = np.empty((c.M, c.N))
        Bh, Bl = split(B)
        for i in range(c.M):
            a = A[:, i][:, None]
            ah, al = split(a)
            p = a * B
            e = ((ah * Bh - p) + ah * Bl + al * Bh) + al * Bl
            pe = np.concatenate([p, e]).T
            P[i] = [math.fsum(row) for row in pe]
        S = np.abs(A).T @ np.abs(B)
    idx = (deposit(c.bits_a)[:, None] + deposit(c.bits_b)[None, :]).reshape(-1)
    ref, band = np.empty(c.total, dtype=P.dtype), np.empty(c.total, dtype=S.dtype)
    ref[idx] = P.reshape(-1)
    band[idx] = (c.K + 1) * 2.0 ** -53 * S.reshape(-1)
    return _freeze(ref, band)
