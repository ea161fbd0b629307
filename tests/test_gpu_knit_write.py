"""The write-bound two-fragment knit on the GPU (``qk_knit_outer_stream_range``), every kernel it dispatches to
(per-output gather, blocked with B in LDS, blocked with B from global memory, the four rows instantiations) and
every mode of each (full range, range slices, device K, small grids with the grid-stride / spread / B-reload
paths), against an exact CPU reference.

Exact: operands are int / 2^16 with |int| < 2^20, so every product is a multiple of 2^-32 below 2^8 and a sum of
8 of them stays below 2^11: the fp64 result is exact in any order, with or without fma, and is compared with
``torch.equal`` against the int64 contraction done on the CPU (tests/knit_write_cases.py). The operands sit in
NaN-padded buffers (lda = M + 3 from an odd 8-byte offset, ldb = N + 2) and the output is a view inside a
NaN-filled buffer whose guards must keep their bits. Every test first asserts, through
``qk_knit_outer_stream_kind``, that its call takes the kernel it is meant to test."""
import contextlib
import ctypes
import struct

import numpy as np
import pytest

import knit_write_cases as kw
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 512  # doubles before and after the output view
NAN = float("nan")
NAN_BITS = struct.unpack("<q", struct.pack("<d", NAN))[0]
OK, EARG = 0, 1


@pytest.fixture(scope="module")
def T(require_gpu):
    import torch

    return torch


@pytest.fixture(autouse=True)
def default_dispatch():
    found = kw.dispatch_env_set()
    if found:
        pytest.skip(f"{', '.join(found)} set in the environment: the dispatcher under test is not the default one")


# ----------------------------------------------------------------------------- operands, launches, checks
class Operands:
    """A as [K][M + 3] from an odd 8-byte offset of its buffer, B as [K][N + 2]; the padding holds NaN."""

    def __init__(self, T, c, A, B):
        self.lda, self.ldb = c.M + 3, c.N + 2
        ha = np.full(1 + c.K * self.lda, NAN)
        hb = np.full(c.K * self.ldb, NAN)
        ha[1:].reshape(c.K, self.lda)[:, :c.M] = A
        hb.reshape(c.K, self.ldb)[:, :c.N] = B
        self.host = (ha, hb)
        self.bufA, self.bufB = T.tensor(ha, device="cuda"), T.tensor(hb, device="cuda")
        assert self.bufA.data_ptr() % 16 == 0 and self.bufB.data_ptr() % 16 == 0
        self.a_ptr, self.b_ptr = self.bufA.data_ptr() + 8, self.bufB.data_ptr()
        T.cuda.synchronize()


_OPS: dict = {}
_REF: dict = {}


def _ops(T, name, normal=False) -> Operands:
    if (name, normal) not in _OPS:
        if normal:
            A, B = kw.normal_operands(name)
        else:
            A, B = (x / float(1 << kw.FRAC_BITS) for x in kw.int_operands(name))  # exact
        _OPS[name, normal] = Operands(T, kw.CASES[name], A, B)
    return _OPS[name, normal]


def _ref(T, name, k=None):
    """The exact write of the first k terms (all K), on the device."""
    if (name, k) not in _REF:
        _REF[name, k] = T.tensor(kw.exact_write(name, k), device="cuda")
        T.cuda.synchronize()
    return _REF[name, k]


def _kind(c, o_begin=0, o_count=None):
    return engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits, o_begin, o_count)


def _launch(T, c, ops, o_begin=0, o_count=None, kd=None, **over):
    """One qk_knit_outer_stream_range call on torch's current stream into the middle of a fresh NaN-filled
    buffer; ``over`` replaces arguments of the C call by name. Returns (status, buffer, n)."""
    ctx = engine.get_context(0)
    n = c.total - o_begin if o_count is None else o_count
    buf = T.full((2 * GUARD + max(n, 0),), NAN, dtype=T.float64, device="cuda")
    kd_t = None if kd is None else T.tensor([kd], dtype=T.int32, device="cuda")
    a = dict(nbits=c.nbits, K=c.K, A=ops.a_ptr, lda=ops.lda, B=ops.b_ptr, ldb=ops.ldb, mA=c.mask_a, mB=c.mask_b,
             o_begin=o_begin, o_count=n, k_dev=None if kd_t is None else kd_t.data_ptr(),
             out=buf.data_ptr() + 8 * GUARD)
    assert a["out"] % 16 == 0
    a.update(over)
    rc = ctx.lib.qk_knit_outer_stream_range(ctx.handle, a["nbits"], a["K"], a["A"], a["lda"], a["B"], a["ldb"], a["mA"],
                                            a["mB"], a["o_begin"], a["o_count"], a["k_dev"], a["out"])
    T.cuda.synchronize()
    return rc, buf, n


def _written(T, rc, buf, n):
    """The output view of a successful launch: guards intact bit for bit, no NaN left inside."""
    assert rc == OK, engine.get_context(0).lib.qk_last_error(engine.get_context(0).handle)
    bits = buf.view(T.int64)
    assert bool((bits[:GUARD] == NAN_BITS).all()), "the guard before the output was written"
    assert bool((bits[GUARD + n:] == NAN_BITS).all()), "the guard after the output was written"
    out = buf[GUARD:GUARD + n]
    assert not bool(out.isnan().any()), "outputs left unwritten, or padding read"
    return out


def _untouched(T, buf):
    assert bool((buf.view(T.int64) == NAN_BITS).all()), "a refused / empty call wrote to the output"


def _write(T, c, ops, o_begin=0, o_count=None, kd=None):
    return _written(T, *_launch(T, c, ops, o_begin, o_count, kd))


def _last_error() -> bytes:
    ctx = engine.get_context(0)
    return ctx.lib.qk_last_error(ctx.handle)


@contextlib.contextmanager
def _on_cus(T, cus):
    """Torch's current stream restricted to the CUs ``cus``: engine.get_context binds the context to it, and the
    kernels size their grids to its CU count."""
    if cus is None:
        yield
        return
    s = engine.cu_masked_stream(0, cus)
    n = ctypes.c_int()
    assert engine.get_context(0).lib.qk_stream_cu_count(0, ctypes.c_void_p(s.cuda_stream), ctypes.byref(n)) == OK
    assert n.value == len(cus), (f"CU masking is not honoured here: a stream masked to {len(cus)} CUs reports "
                                 f"{n.value}; the small-grid paths cannot be reached")
    T.cuda.synchronize()
    with T.cuda.stream(s):
        yield
    T.cuda.synchronize()


# ----------------------------------------------------------------------------- 1. the full range, every table row
@pytest.mark.parametrize("case", kw.TABLE + kw.EXTRA, ids=lambda c: c.name)
def test_full_range_write_is_exact(T, case):
    c = case
    assert _kind(c) == (c.kind, c.task_bits)
    assert T.equal(_write(T, c, _ops(T, c.name)), _ref(T, c.name))


# ----------------------------------------------------------------------------- 2. range slices
SLICED = ("blk16", "blk17", "blk_odd", "bg_k8", "bg_k1", "bg_k2", "rows_k1", "rows_k2", "rows_k3", "rows_k5", "old_last")


def _min_unit(c):
    """The smallest range alignment that still selects the case's kind: 2^9 (one 512-output iteration) for the
    blocked kernel, 2^14 for B-from-global, the piece for the rows kernel."""
    return {1: 9, 2: 14, 3: c.task_bits}[c.kind]


def _check_slices(T, name):
    c, ops, ref = kw.CASES[name], _ops(T, name), _ref(T, name)
    assert _kind(c)[0] == c.kind
    full = _write(T, c, ops)
    assert T.equal(full, ref)
    step = c.total // 4
    quarters = [(r * step, step) for r in range(4)]
    unit = _min_unit(c)
    finest = kw.odd_partition(c.total, unit)
    for pieces, tb in ((quarters, None), (finest, unit)):
        parts = []
        for o_begin, o_count in pieces:
            kind, got_tb = _kind(c, o_begin, o_count)
            assert kind == c.kind and (tb is None or got_tb == tb), (o_begin, o_count, kind, got_tb)
            part = _write(T, c, ops, o_begin, o_count)
            assert T.equal(part, ref[o_begin:o_begin + o_count]), (o_begin, o_count)
            parts.append(part)
        assert T.equal(T.cat(parts), full)


@pytest.mark.parametrize("name", SLICED)
def test_range_slices_concatenate_to_the_full_write(T, name):
    """Four equal slices, and slices of 1, 3, 5, .. units at the smallest alignment that still selects the kind,
    each into its own guarded buffer: every slice is exact and they concatenate bit for bit to the full write."""
    _check_slices(T, name)


def test_blocked_slices_of_a_rows_layout_match_the_rows_write(T):
    """rows_k1's masks over 2^12-aligned slices take the blocked kernel (tasks of 2^11: no A bit inside a task, K
    odd), over the full range the rows kernel <1,13>: two kernels, the same operands, the same bits."""
    c, ops, ref = kw.CASES["rows_k1"], _ops(T, "rows_k1"), _ref(T, "rows_k1")
    assert _kind(c) == (3, 13)
    full = _write(T, c, ops)
    assert T.equal(full, ref)
    parts = []
    for o_begin, o_count in kw.odd_partition(c.total, 12):
        assert _kind(c, o_begin, o_count) == (1, 11)
        parts.append(_write(T, c, ops, o_begin, o_count))
        assert T.equal(parts[-1], ref[o_begin:o_begin + o_count])
    assert T.equal(T.cat(parts), full)


@pytest.mark.parametrize("name", sorted(kw.WIDE_KINDS))
def test_slices_of_a_32_bit_output_past_2_31(T, name):
    """2^17 outputs across 2^31 and the last 2^16 of a 2^32-entry output, each into its own small buffer: task /
    piece bases and the o - o_begin offsets beyond a signed 32-bit index, in the blocked, B-from-global and rows
    kernels; with the host K and with a device K of 1."""
    c, ops = kw.CASES[name], _ops(T, name)
    for o_begin, o_count in kw.WIDE_RANGES:
        assert _kind(c, o_begin, o_count) == kw.WIDE_KINDS[name]
        assert T.equal(_write(T, c, ops, o_begin, o_count), T.tensor(kw.exact_slice(name, o_begin, o_count), device="cuda"))
        assert T.equal(_write(T, c, ops, o_begin, o_count, kd=1),
                       T.tensor(kw.exact_slice(name, o_begin, o_count, 1), device="cuda"))


# ----------------------------------------------------------------------------- 3. device K
DEVICE_K = ("blk16", "blk17", "blk_odd", "bg_k8", "bg_k2", "bg_k1", "rows_k1", "rows_k2", "rows_k3", "rows_k4", "rows_k5",
            "rows_k8", "old_last")


def _check_device_k(T, name):
    c, ops = kw.CASES[name], _ops(T, name)
    assert _kind(c) == (c.kind, c.task_bits) and c.kind != 0
    for kd in (0, -1):
        rc, buf, _ = _launch(T, c, ops, kd=kd)
        assert rc == OK
        _untouched(T, buf)
    # 1: the first term alone; K - 1: the k < K guard inside an instantiation wider than the run-time K;
    # K, K + 3: clamped to K
    for kd in sorted({1, max(c.K - 1, 1), c.K, c.K + 3}):
        assert T.equal(_write(T, c, ops, kd=kd), _ref(T, name, min(kd, c.K))), kd
    # a slice with a device K (the multi-GPU step's call)
    o_begin, o_count = kw.odd_partition(c.total, _min_unit(c))[-1]
    assert _kind(c, o_begin, o_count)[0] == c.kind
    assert T.equal(_write(T, c, ops, o_begin, o_count, kd=1), _ref(T, name, 1)[o_begin:o_begin + o_count])
    rc, buf, _ = _launch(T, c, ops, o_begin, o_count, kd=0)
    assert rc == OK
    _untouched(T, buf)


@pytest.mark.parametrize("name", DEVICE_K)
def test_device_k_clamps_and_predicates(T, name):
    _check_device_k(T, name)


# ----------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("name,o_begin,o_count,kd", [("stream8", 0, None, 8), ("stream8", 0, None, 0), ("stream8", 0, 128, None),
                                                     ("stream8", 128, 128, None), ("stream13", 0, None, 3),
                                                     ("stream13", 0, 4096, None), ("rows_k8", 1 << 10, 3 << 10, None),
                                                     ("rows_k8", 1 << 10, 3 << 10, 8)])
def test_ranges_and_device_k_without_a_blocked_task_are_refused(T, name, o_begin, o_count, kd):
    """The per-output kernel writes the full range with the host K only: a partial range or a device K that no
    blocked / rows form can take is QK_EARG, and nothing is written."""
    c = kw.CASES[name]
    assert _kind(c, o_begin, o_count) == (0, 0)
    rc, buf, _ = _launch(T, c, _ops(T, name), o_begin, o_count, kd)
    assert rc == EARG and b"task-aligned" in _last_error()
    _untouched(T, buf)


def test_argument_checks(T):
    c, ops = kw.CASES["blk9"], _ops(T, "blk9")
    assert _kind(c) == (1, 9)
    ctx = engine.get_context(0)

    def call(**over):
        rc, buf, _ = _launch(T, c, ops, **over)
        return rc, buf

    bad = [
        ("overlapping masks", dict(mA=c.mask_a | 4), b"masks"),  # bit 2 is B's
        ("masks with a hole", dict(mB=c.mask_b & ~4), b"masks"),
        ("masks beyond nbits", dict(mA=c.mask_a | 1 << 9), b"masks"),
        ("bit 0 in maskA", dict(mA=c.mask_a | 1, mB=c.mask_b & ~1), b"masks"),
        ("K = 0", dict(K=0), b"1 <= K <= 8"),
        ("K = 9", dict(K=9), b"1 <= K <= 8"),
        ("nbits = 1", dict(nbits=1), b"nbits"),
        ("nbits = 33", dict(nbits=33), b"nbits"),
        ("odd ldb", dict(ldb=c.N + 3), b"leading dimension"),
        ("ldb < N", dict(ldb=c.N - 2), b"leading dimension"),
        ("lda < M", dict(lda=c.M - 1), b"leading dimension"),
        ("B + 8 bytes", dict(B=ops.b_ptr + 8), b"alignment"),
        ("range past the end", dict(o_begin=256, o_count=512), b"output range"),
        ("negative begin", dict(o_begin=-512, o_count=512), b"output range"),
        ("negative count", dict(o_begin=0, o_count=-512), b"output range"),
        ("null A", dict(A=None), b"null"),
        ("null B", dict(B=None), b"null"),
        ("null out", dict(out=None), b"null"),
    ]
    for what, over, msg in bad:
        rc, buf = call(**over)
        err = _last_error()
        assert rc == EARG and err and b"qk_knit_outer_stream" in err and msg in err, (what, rc, err)
        _untouched(T, buf)
    # out + 8 bytes: the view's own address, moved
    rc, buf, _ = _launch(T, c, ops)
    assert rc == OK
    buf2 = T.full_like(buf, NAN)
    rc = ctx.lib.qk_knit_outer_stream_range(ctx.handle, c.nbits, c.K, ops.a_ptr, ops.lda, ops.b_ptr, ops.ldb, c.mask_a,
                                            c.mask_b, 0, c.total, None, buf2.data_ptr() + 8 * GUARD + 8)
    T.cuda.synchronize()
    assert rc == EARG and b"alignment" in _last_error()
    _untouched(T, buf2)
    # no context: refused, and there is nowhere to leave a message
    assert ctx.lib.qk_knit_outer_stream_range(None, c.nbits, c.K, ops.a_ptr, ops.lda, ops.b_ptr, ops.ldb, c.mask_a,
                                              c.mask_b, 0, c.total, None, buf2.data_ptr() + 8 * GUARD) == EARG
    T.cuda.synchronize()
    _untouched(T, buf2)
    # an empty range is fine and writes nothing
    rc, buf = call(o_begin=0, o_count=0)
    assert rc == OK
    _untouched(T, buf)
    rc, buf = call(o_begin=c.total, o_count=0)
    assert rc == OK
    _untouched(T, buf)
    # the full-range entry checks nbits itself
    for nbits in (1, 33):
        rc = ctx.lib.qk_knit_outer_stream(ctx.handle, nbits, c.K, ops.a_ptr, ops.lda, ops.b_ptr, ops.ldb, c.mask_a, c.mask_b,
                                          buf2.data_ptr() + 8 * GUARD)
        assert rc == EARG and b"nbits" in _last_error()
    T.cuda.synchronize()
    _untouched(T, buf2)
    # and after all the refusals the same context still writes the right thing
    assert T.equal(_write(T, c, ops), _ref(T, "blk9"))


def test_full_range_entry_equals_the_range_entry(T):
    """qk_knit_outer_stream is the range entry over 0..2^nbits with the host K."""
    ctx = engine.get_context(0)
    for name in ("stream8", "blk9", "bg_k2", "rows_k4"):
        c, ops = kw.CASES[name], _ops(T, name)
        buf = T.full((2 * GUARD + c.total,), NAN, dtype=T.float64, device="cuda")
        rc = ctx.lib.qk_knit_outer_stream(ctx.handle, c.nbits, c.K, ops.a_ptr, ops.lda, ops.b_ptr, ops.ldb, c.mask_a,
                                          c.mask_b, buf.data_ptr() + 8 * GUARD)
        T.cuda.synchronize()
        assert T.equal(_written(T, rc, buf, c.total), _ref(T, name))


# ----------------------------------------------------------------------------- 5. repeatability
@pytest.mark.parametrize("name", ["stream13", "blk16", "bg_k8", "rows_k1", "rows_k2", "rows_k4", "rows_k8"])
def test_two_launches_give_the_same_bits(T, name):
    c, ops = kw.CASES[name], _ops(T, name)
    assert _kind(c) == (c.kind, c.task_bits)
    first, second = _write(T, c, ops), _write(T, c, ops)
    assert T.equal(first, _ref(T, name)) and T.equal(second, first)


# ----------------------------------------------------------------------------- 6. N(0,1) operands, derived bound
def _check_normal(T, name, out):
    ref, band = kw.normal_write(name)
    err = np.abs(out.cpu().numpy().astype(ref.dtype) - ref)
    worst = float((err / band).max())
    print(f"{name}: worst |got - ref| / ((K + 1) 2^-53 sum|A||B|) = {worst:.3f}")
    assert np.all(err <= band), (name, worst)


@pytest.mark.parametrize("name", ["stream8", "stream13", "blk16", "blk_odd", "bg_k8", "rows_k1", "rows_k2", "rows_k3", "rows_k8"])
def test_normal_operands_stay_within_the_fma_chain_bound(T, name):
    """|got - ref| <= (K + 1) 2^-53 sum_k |A_k| |B_k| per entry against the extended-precision contraction: gamma_K
    of a K-term fma chain plus one unit for the reference. Derived, not measured; a path that loses precision
    (a float intermediate, a dropped low term) falls outside it."""
    c = kw.CASES[name]
    assert _kind(c) == (c.kind, c.task_bits)
    _check_normal(T, name, _write(T, c, _ops(T, name, normal=True)))


# ----------------------------------------------------------------------------- 7. small grids
CU_SETS = [(0,), (0, 1), tuple(range(8))]


@pytest.mark.parametrize("cus", CU_SETS, ids=lambda s: f"{len(s)}cu")
def test_small_grid_blocked_spread_order(T, monkeypatch, cus):
    """512 tasks of 2^9 outputs on one workgroup per CU (<= 8 workgroups): the grid-stride loop restages LDS per
    task and, with >= 4 tasks per workgroup, takes the tasks in the 8-part spread order. Exact, and the same
    bits as the plain order."""
    c, ops = kw.CASES["grid_blk"], _ops(T, "grid_blk")
    monkeypatch.setenv("QKNIT_OB_TB", "9")
    monkeypatch.setenv("QKNIT_OB_WG_PER_CU", "1")
    assert _kind(c) == (1, 9)
    assert (c.total >> 9) >= 4 * len(cus) and (c.total >> 9) % 8 == 0  # what the launch needs to pick spread = 8
    with _on_cus(T, cus):
        spread = _write(T, c, ops)
        monkeypatch.setenv("QKNIT_OB_SPREAD", "1")
        plain = _write(T, c, ops)
    assert T.equal(spread, _ref(T, "grid_blk")) and T.equal(plain, spread)


@pytest.mark.parametrize("name", sorted(kw.GRID_ROWS))
@pytest.mark.parametrize("cus", CU_SETS, ids=lambda s: f"{len(s)}cu")
def test_small_grid_rows_reload_and_spread_order(T, monkeypatch, cus, name):
    """128 pieces over 4 B runs on a grid of a few workgroups: each workgroup strides over pieces of different B
    runs (B's high bits are not adjacent) and reloads its B registers. Which piece order the default takes (8
    parts when the grid is a multiple of 8 x the run count with >= 4 pieces per workgroup) depends on the
    kernel's occupancy, which cannot be queried: it is not asserted; every order must be exact. grid_rows_one
    (256 pieces, one B run) on 8 CUs meets those conditions at any occupancy, so the 8-part order runs there."""
    c, ops = kw.CASES[name], _ops(T, name)
    assert _kind(c) == (c.kind, c.task_bits) and c.kind == 3
    assert (c.total >> c.task_bits, c.N >> c.task_bits) == kw.GRID_ROWS[name]
    with _on_cus(T, cus):
        default = _write(T, c, ops)
        monkeypatch.setenv("QKNIT_OR_SPREAD", "1")
        plain = _write(T, c, ops)
        monkeypatch.setenv("QKNIT_OR_SPREAD", "8")
        eight = _write(T, c, ops)
    ref = _ref(T, name)
    assert T.equal(default, ref) and T.equal(plain, ref) and T.equal(eight, ref)


@pytest.mark.parametrize("cus", CU_SETS, ids=lambda s: f"{len(s)}cu")
def test_small_grid_per_output_kernel_strides(T, cus):
    """16 chunks of 512 outputs on 8 workgroups per CU: on one CU every workgroup takes two chunks."""
    c, ops = kw.CASES["stream13"], _ops(T, "stream13")
    assert _kind(c) == (0, 0)
    with _on_cus(T, cus):
        out = _write(T, c, ops)
    assert T.equal(out, _ref(T, "stream13"))


@pytest.mark.parametrize("name", ["blk16", "bg_k8", "old_last", "rows_k2"])
def test_two_cu_stream_slices_and_device_k(T, monkeypatch, name):
    """The slice and device-K checks on a 2-CU stream with one blocked workgroup per CU, so that launches over a
    range with o_begin != 0 also stride over several tasks / pieces per workgroup."""
    monkeypatch.setenv("QKNIT_OB_WG_PER_CU", "1")
    with _on_cus(T, (0, 1)):
        _check_slices(T, name)
        _check_device_k(T, name)


# ----------------------------------------------------------------------------- 8. qk_knit_select on kinds 2 and 3
@pytest.mark.parametrize("name", ["bg_k2", "rows_k2"])
def test_knit_select_is_bit_identical_to_the_dense_write(T, name):
    """qk_knit_select's entries |v| > acc are the thresholded dense write, keys and bits, where the dense write
    comes from the B-from-global kernel and from the rows kernel (acc: the 0.99 quantile of |v|). The dense
    write on these N(0,1) operands is held to the derived bound; its indexing is pinned exactly above."""
    c = kw.CASES[name]
    assert _kind(c) == (c.kind, c.task_bits)
    ctx = engine.get_context(0)
    A, B = (T.tensor(x, device="cuda") for x in kw.normal_operands(name))
    dense = T.full((c.total,), NAN, dtype=T.float64, device="cuda")
    engine.knit_outer_stream(ctx, A, B, list(c.bits_a), list(c.bits_b), c.nbits, dense)
    T.cuda.synchronize()
    _check_normal(T, name, dense)
    mags = dense.abs()
    acc = float(T.quantile(mags.cpu(), 0.99))
    ref_keys = T.nonzero(mags > acc).reshape(-1)
    assert 0 < ref_keys.numel() < c.total // 50
    keys, vals = engine.knit_select(ctx, A, B, list(c.bits_a), list(c.bits_b), c.nbits, acc)
    order = T.argsort(keys)
    assert T.equal(keys[order], ref_keys)
    assert T.equal(vals[order], dense[ref_keys])


# ----------------------------------------------------------------------------- 9. the operands were only read
def test_operand_buffers_kept_their_bits(T):
    """Runs last: every operand buffer the tests above launched on, padding included, still holds what was
    uploaded."""
    assert _OPS
    for (name, normal), ops in _OPS.items():
        for dev, host in zip((ops.bufA, ops.bufB), ops.host):
            assert np.array_equal(dev.cpu().numpy().view(np.int64), host.view(np.int64)), (name, normal)
