"""The dispatcher of the write-bound knit (``qk_knit_outer_stream_kind``: which of the four kernels a call
launches, and its task width) against a plain Python model of it (tests/knit_write_cases.py): on the shared
case table, and on every mask pair of small outputs. Host only: the query makes no HIP call."""
import ctypes

import pytest

import knit_write_cases as kw
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import _lib, engine


@pytest.fixture(autouse=True)
def default_dispatch():
    """QKNIT_OB_ROWS / QKNIT_OB_BGLOBAL are read once per process (no monkeypatch can undo them), the others
    at every query: the default dispatch is only there with all of them unset."""
    found = kw.dispatch_env_set()
    if found:
        pytest.skip(f"{', '.join(found)} set in the environment: the dispatcher under test is not the default one")


def _bits(mask):
    return [b for b in range(64) if mask >> b & 1]


@pytest.mark.parametrize("case", kw.TABLE + kw.EXTRA + kw.SMALL_GRID, ids=lambda c: c.name)
def test_table_kinds_match_the_library_and_the_model(case):
    c = case
    assert kw.model_kind(c.nbits, c.K, c.mask_a, c.mask_b) == (c.kind, c.task_bits), "table vs model"
    assert engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits) == (c.kind, c.task_bits)
    assert engine.knit_outer_stream_kernel(c.K, c.bits_a, c.bits_b, c.nbits) == engine.OUTER_STREAM_KERNELS[c.kind]


@pytest.mark.parametrize("name,o_begin,o_count,kind,tb", kw.RANGE_TABLE)
def test_range_kinds_match_the_library_and_the_model(name, o_begin, o_count, kind, tb):
    c = kw.CASES[name]
    assert kw.model_kind(c.nbits, c.K, c.mask_a, c.mask_b, o_begin, o_count) == (kind, tb), "table vs model"
    assert engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits, o_begin, o_count) == (kind, tb)
    assert engine.knit_outer_stream_kernel(c.K, c.bits_a, c.bits_b, c.nbits, o_begin,
                                           o_count) == engine.OUTER_STREAM_KERNELS[kind]


def test_table_reaches_every_kernel_and_every_rows_instantiation():
    """By the library's own answer: the GPU tests assert the same kinds before they launch."""
    reached = set()
    for c in kw.TABLE:
        kind, _ = engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits)
        reached.add((kind, kw.rows_instantiation(c.K)) if kind == 3 else kind)
    assert reached == {0, 1, 2, (3, "<1,13>"), (3, "<2,12>"), (3, "<4,11>"), (3, "<8,11>")}
    assert {c.name: (c.kind, c.task_bits) for c in kw.SMALL_GRID} == {"grid_blk": (1, 16), "grid_rows_k8": (3, 11),
                                                                      "grid_rows_k1": (3, 13), "grid_rows_one": (3, 11)}


@pytest.mark.parametrize("case", kw.WIDE, ids=lambda c: c.name)
def test_wide_slices_keep_their_kinds(case):
    """The 32-bit layouts take their kernel over the whole range and over the slices around 2^31 and 2^32."""
    c = case
    assert (c.kind, c.task_bits) == kw.WIDE_KINDS[c.name]
    for o_begin, o_count in ((0, 1 << 32),) + kw.WIDE_RANGES:
        assert engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits, o_begin, o_count) == kw.WIDE_KINDS[c.name]
        assert kw.model_kind(c.nbits, c.K, c.mask_a, c.mask_b, o_begin, o_count) == kw.WIDE_KINDS[c.name]


@pytest.mark.parametrize("name", ["blk16", "bg_k2", "rows_k4"])
def test_slice_reference_equals_the_whole_reference(name):
    """exact_slice (pext of each output index) against exact_write (deposit keys): two routes to the same bits."""
    c = kw.CASES[name]
    whole = kw.exact_write(name)
    for o_begin, o_count in [(0, c.total), (c.total // 2 - 512, 1536), (c.total - 512, 512)]:
        assert (kw.exact_slice(name, o_begin, o_count) == whole[o_begin:o_begin + o_count]).all()
    assert (kw.exact_slice(name, 512, 1024, 1) == kw.exact_write(name, 1)[512:1536]).all()


def test_kernel_names_cover_the_four_kinds():
    assert len(engine.OUTER_STREAM_KERNELS) == 4 and len(set(engine.OUTER_STREAM_KERNELS)) == 4
    assert "rows" in engine.OUTER_STREAM_KERNELS[3] and "rows" in engine.knit_outer_stream_kernel.__doc__
    assert [kw.rows_instantiation(K) for K in range(1, 9)] == ["<1,13>", "<2,12>", "<4,11>", "<4,11>"] + ["<8,11>"] * 4


@pytest.mark.parametrize("key", sorted(kw.LEGACY), ids=lambda k: f"K{k[0]}-n{k[1]}")
def test_legacy_parameters_keep_their_kinds(key):
    """What tests/test_gpu.py's stream-knit parameters dispatch to (they assert it from this table)."""
    K, nbits, bits_b = key
    bits_a = [b for b in range(nbits) if b not in bits_b]
    assert engine.knit_outer_stream_kind(K, bits_a, list(bits_b), nbits) == kw.LEGACY[key]
    assert kw.model_kind(nbits, K, kw.mask_of(bits_a), kw.mask_of(bits_b)) == kw.LEGACY[key]


def _query():
    fn = _lib.lib().qk_knit_outer_stream_kind
    kind, tb = ctypes.c_int(), ctypes.c_int()
    pk, pt = ctypes.byref(kind), ctypes.byref(tb)

    def q(nbits, K, mA, mB, o_begin, o_count):
        assert fn(nbits, K, mA, mB, o_begin, o_count, pk, pt) == 0
        return kind.value, tb.value

    return q


def test_every_small_mask_pair_dispatches_as_the_model():
    """nbits 9..14, every (maskA, maskB) partition with bit 0 in B, K in {1, 2, 3, 8}, the full range."""
    q = _query()
    seen = set()
    for nbits in range(9, 15):
        full = (1 << nbits) - 1
        for mB in range(1, 1 << nbits, 2):
            mA = full ^ mB
            for K in (1, 2, 3, 8):
                got = q(nbits, K, mA, mB, 0, 1 << nbits)
                assert got == kw.model_kind(nbits, K, mA, mB), (nbits, K, _bits(mB))
                seen.add((got[0], K) if got[0] == 3 else got[0])
    # the sweep is not vacuous: every kind, and the rows kernel at each K, came up
    assert seen >= {0, 1, 2, (3, 1), (3, 2), (3, 3), (3, 8)}


def test_every_range_alignment_dispatches_as_the_model():
    """nbits 13, every mask pair, K in {1, 2, 3, 8}: ranges [2^a, 2^a + 2^a) of every alignment a = 8..12 (8: below
    the narrowest task), and 3 2^a outputs from 2^a (a count that is no power of two)."""
    q = _query()
    nbits = 13
    full = (1 << nbits) - 1
    for mB in range(1, 1 << nbits, 2):
        mA = full ^ mB
        for K in (1, 2, 3, 8):
            for a in range(8, 13):
                for count in (1 << a, 3 << a):
                    if (1 << a) + count > 1 << nbits:
                        continue
                    got = q(nbits, K, mA, mB, 1 << a, count)
                    assert got == kw.model_kind(nbits, K, mA, mB, 1 << a, count), (K, _bits(mB), a, count)
                    assert got[1] <= a


def test_task_width_cap_is_read_per_query(monkeypatch):
    """QKNIT_OB_TB caps the blocked task width at every query (the small-grid GPU tests rely on it); the rows
    kernel is not subject to it."""
    c = kw.CASES["blk16"]
    monkeypatch.setenv("QKNIT_OB_TB", "9")
    assert engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits) == (1, 9)
    assert kw.model_kind(c.nbits, c.K, c.mask_a, c.mask_b, cap=9) == (1, 9)
    r = kw.CASES["rows_k2"]
    assert engine.knit_outer_stream_kind(r.K, r.bits_a, r.bits_b, r.nbits) == (3, 12)
    monkeypatch.delenv("QKNIT_OB_TB")
    assert engine.knit_outer_stream_kind(c.K, c.bits_a, c.bits_b, c.nbits) == (c.kind, c.task_bits)


def test_query_rejects_bad_arguments():
    fn = _lib.lib().qk_knit_outer_stream_kind
    kind, tb = ctypes.c_int(), ctypes.c_int()
    pk, pt = ctypes.byref(kind), ctypes.byref(tb)
    assert fn(9, 1, 0x1FE, 1, 0, 512, pk, pt) == 0
    for args in [(1, 1, 0, 1, 0, 2), (33, 1, 0, 1, 0, 2), (9, 0, 0x1FE, 1, 0, 512), (9, 9, 0x1FE, 1, 0, 512),
                 (9, 1, 0x1FE, 1, 0, 0)]:
        assert fn(*args, pk, pt) == 1, args
    assert fn(9, 1, 0x1FE, 1, 0, 512, None, pt) == 1 and fn(9, 1, 0x1FE, 1, 0, 512, pk, None) == 1


def _pext(x, mask):
    r = bit = 0
    for b in range(mask.bit_length()):
        if mask >> b & 1:
            r |= (x >> b & 1) << bit
            bit += 1
    return r


@pytest.mark.parametrize("name", ["stream2", "stream8", "blk9", "blk_odd"])
def test_exact_reference_is_the_header_definition(name):
    """The GPU tests' reference (int64 GEMM scattered through deposit keys) equals include/qknit.h's
    out[o] = sum_k A[k][pext(o, maskA)] B[k][pext(o, maskB)], entry by entry in Python integers; the N(0,1)
    reference agrees with it to its own band."""
    c = kw.CASES[name]
    A, B = kw.int_operands(name)
    assert abs(A).max() < 1 << kw.INT_BITS and abs(B).max() < 1 << kw.INT_BITS and A.shape == (c.K, c.M)
    for k in (None, 1):
        ref = kw.exact_write(name, k)
        want = [sum(int(A[t, _pext(o, c.mask_a)]) * int(B[t, _pext(o, c.mask_b)]) for t in range(k or c.K))
                for o in range(c.total)]
        assert [int(v * 2.0 ** 32) for v in ref] == want and all(float(int(v * 2.0 ** 32)) == v * 2.0 ** 32 for v in ref)
    An, Bn = kw.normal_operands(name)
    nref, band = kw.normal_write(name)
    for o in range(0, c.total, max(c.total // 64, 1)):
        i, j = _pext(o, c.mask_a), _pext(o, c.mask_b)
        assert abs(float(nref[o]) - float(An[:, i] @ Bn[:, j])) <= band[o]
        assert band[o] >= (c.K + 1) * 2.0 ** -53 * float(abs(An[:, i]) @ abs(Bn[:, j])) * (1 - 2.0 ** -40)


def test_odd_partition_has_the_alignment_it_promises():
    for total_bits, unit_bits in [(16, 9), (17, 9), (18, 14), (16, 13), (16, 12), (15, 11), (18, 11), (9, 9)]:
        parts = kw.odd_partition(1 << total_bits, unit_bits)
        assert parts[0][0] == 0 and sum(n for _, n in parts) == 1 << total_bits
        assert all(b0 + n0 == b1 for (b0, n0), (b1, _) in zip(parts, parts[1:]))
        if total_bits > unit_bits:
            assert all(kw.ctz(b | n) == unit_bits for b, n in parts)
