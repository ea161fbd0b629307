"""Per-clbit 2x2 channels on the GPU: ``qk_kron2_rows`` against the numpy model, and ``KnitReducer.with_channels``
/ ``with_readout_error`` / ``with_readout_mitigation`` against the same map applied to the oracle's dense knit."""
import functools
import itertools
import random

import numpy as np
import pytest

from test_gpu_moments import _moment_band
from test_gpu_observables import DIRECT_ONLY, _case
from test_gpu_shots import SHOTS, replay
from test_observables import np_expectation, np_marginal

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (VirtualCircuit, cutting, engine,
                                                                      observables as ob,
                                                                      run_virtual_circuit_expectation,
                                                                      run_virtual_circuit_marginal)
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer

pytestmark = pytest.mark.gpu
TOL = 1e-12  # the project's parity tolerance, per entry of the knit
PAD = -77.25  # what the padding columns hold before a launch
U = 2.0 ** -53
EYE = np.eye(2)
HADAMARD = np.array([[1.0, 1.0], [1.0, -1.0]])
SUM_OUT = np.array([[1.0, 1.0], [0.0, 0.0]])


@pytest.fixture(scope="module")
def T(require_gpu):
    import torch

    return torch


def gamma(k):
    return k * U / (1 - k * U)


# ----------------------------------------------------------------------------- 1. kernel, exact
ROWS = (1, 5, 37)
# one pass up to m = 13, two up to 22 (14: the first; 22: nine strided bits), three beyond (23)
MS = (0, 1, 2, 5, 6, 7, 9, 12, 13, 14, 16, 17)
EXACT = [(r, m) for m in MS for r in ROWS] + [(1, 22), (1, 23)]
# the 192 matrices with entries in {-1, 0, 1, 2} that differ from their transpose
ASYMMETRIC = [np.array(e, dtype=np.float64).reshape(2, 2) for e in itertools.product((-1, 0, 1, 2), repeat=4) if e[1] != e[2]]


def _int_mats(m, seed):
    """A different matrix for every bit, none equal to its transpose: a transposed matrix or a matrix on the
    wrong bit changes the result."""
    pick = np.random.default_rng(seed).permutation(len(ASYMMETRIC))[:m]
    return np.stack([ASYMMETRIC[i] for i in pick]) if m else np.zeros((0, 2, 2))


def _int_rows(rows, m, pad):
    return np.random.default_rng(rows * 100 + m).integers(-8, 9, size=(rows, (1 << m) + pad)).astype(np.float64)


def _kron(T, src_np, m, mats, pad_dst=5):
    """qk_kron2_rows through engine.kron2_rows, out of place: the source as given (its padding columns belong to
    ld_src), the output padded with ``pad_dst`` pre-filled columns that must stay."""
    ctx = engine.get_context(0)
    src = T.from_numpy(src_np).cuda()
    out = T.full((src.shape[0], (1 << m) + pad_dst), PAD, dtype=T.float64, device="cuda")
    assert engine.kron2_rows(ctx, src, mats, m, out=out) is out
    got = out.cpu().numpy()
    assert np.all(got[:, 1 << m:] == PAD), "padding columns were written"
    assert T.equal(src, T.from_numpy(src_np).cuda()), "the source was written"
    return got[:, :1 << m]


def _kron_in_place(T, src_np, m, mats):
    """The same in place: the padding columns of the buffer hold PAD and must stay."""
    ctx = engine.get_context(0)
    host = src_np.copy()
    host[:, 1 << m:] = PAD
    buf = T.from_numpy(host).cuda()
    assert engine.kron2_rows(ctx, buf, mats, m, out=buf) is buf
    got = buf.cpu().numpy()
    assert np.all(got[:, 1 << m:] == PAD), "padding columns were written"
    return got[:, :1 << m]


@pytest.mark.parametrize("rows,m", EXACT, ids=[f"{r}-{m}" for r, m in EXACT])
def test_kron2_rows_matches_numpy_exactly(T, rows, m):
    """Integer-valued doubles in [-8, 8] and matrices with entries in {-1, 0, 1, 2} (absolute row sums of at most
    4): every product and partial sum is an integer below 8 * 4^23 = 2^49 < 2^53, so the result equals the int64
    numpy model bit for bit whatever the order of the butterflies and with or without fused multiply-adds;
    ld_src = 2^m + 3, ld_dst = 2^m + 5 with the padding checked; then the same in place."""
    src = _int_rows(rows, m, 3)
    mats = _int_mats(m, 7 * m + rows)
    want = ob.kron2_host(src[:, :1 << m].astype(np.int64), m, mats.astype(np.int64)).astype(np.float64)
    np.testing.assert_array_equal(_kron(T, src, m, mats), want)
    np.testing.assert_array_equal(_kron_in_place(T, src, m, mats), want)


# ----------------------------------------------------------------------------- 2. special matrices
@pytest.mark.parametrize("rows,m", [(5, 0), (3, 6), (5, 13), (2, 16)])
def test_kron2_rows_identity_copies_and_touches_nothing_else(T, rows, m):
    src = _int_rows(rows, m, 3)
    mats = np.tile(EYE, (m, 1, 1))
    np.testing.assert_array_equal(_kron(T, src, m, mats), src[:, :1 << m])
    np.testing.assert_array_equal(_kron_in_place(T, src, m, mats), src[:, :1 << m])


@pytest.mark.parametrize("rows,m", [(5, 3), (37, 9), (5, 13), (3, 14), (2, 16)])
def test_kron2_rows_of_hadamard_matrices_is_wht_rows(T, rows, m):
    src = _int_rows(rows, m, 0)
    want = engine.wht_rows(engine.get_context(0), T.from_numpy(src).cuda(), m).cpu().numpy()
    np.testing.assert_array_equal(_kron(T, src, m, np.tile(HADAMARD, (m, 1, 1))), want)


@pytest.mark.parametrize("rows,m,drop", [(5, 6, 0b010110), (3, 13, 0b1000000100101), (2, 16, 0xA5C3), (2, 16, 0xE000),
                                         (5, 7, 0x7F)])
def test_kron2_rows_summing_bits_out_is_reduce_bits(T, rows, m, drop):
    """[[1, 1], [0, 0]] on the bits of ``drop``, the identity elsewhere: the marginal onto the other bits sits at
    ``pdep(y, keep)`` and every index with a dropped bit set holds 0."""
    src = _int_rows(rows, m, 0)
    keep = ((1 << m) - 1) & ~drop
    mats = np.stack([SUM_OUT if drop >> b & 1 else EYE for b in range(m)])
    got = _kron(T, src, m, mats)
    red = engine.reduce_bits(engine.get_context(0), T.from_numpy(src).cuda(), m, keep, [0]).cpu().numpy()
    at = np.array([ob.pdep(y, keep) for y in range(red.shape[1])], dtype=np.int64)
    want = np.zeros_like(got)
    want[:, at] = red
    np.testing.assert_array_equal(got, want)


def test_kron2_rows_with_work_in_the_last_pass_only(T):
    """m = 16: the identity on the 13 bits of pass 0, three matrices on the strided bits of pass 1. In place only
    that pass is launched; out of place pass 0 copies. Both equal the host model."""
    rows, m = 3, 16
    src = _int_rows(rows, m, 3)
    mats = np.concatenate([np.tile(EYE, (13, 1, 1)), _int_mats(3, 99)])
    want = ob.kron2_host(src[:, :1 << m].astype(np.int64), m, mats.astype(np.int64)).astype(np.float64)
    np.testing.assert_array_equal(_kron(T, src, m, mats), want)
    np.testing.assert_array_equal(_kron_in_place(T, src, m, mats), want)


# ----------------------------------------------------------------------------- 3. rounding, determinism
def _confusion(n, seed, lo=0.0, hi=0.1):
    e = np.random.default_rng(seed).uniform(lo, hi, size=(n, 2))
    return np.stack([ob.readout_matrix(e0, e1) for e0, e1 in e]) if n else np.zeros((0, 2, 2))


@pytest.mark.parametrize("rows,m", [(5, 16), (37, 13), (3, 7), (1, 17)])
def test_kron2_rows_is_deterministic_and_within_the_butterfly_bound(T, rows, m):
    """Standard-normal rows, random confusion matrices with e0, e1 in [0, 0.1]. Two launches give identical bytes;
    rows 0:3 launched alone equal rows 0:3 of the larger launch; in place equals out of place.

    Every stage forms ``c a + c' b`` from two products and one add (or one product and one fused multiply-add): at
    most two roundings on each term, so after the m stages an output lies within
    ``gamma_{2m} * kron2_host(|src|, |mats|)[y]`` of the exact result (here: the model in ``np.longdouble``), with
    ``gamma_k = k u / (1 - k u)``, ``u = 2^-53`` — derived, not measured.

    Round trip with B = invert_channels(A): against the same two maps in ``np.longdouble`` the result lies within the
    sum of the two launches' bounds, the first one carried through ``|B|``. The source itself is further away only
    by what the inverses are rounded by: an entry of B is a product and a difference (the determinant: ad >= 0.81,
    bc <= 0.01, so its relative error is at most (0.82 / 0.80 + 1) u), a quotient and a sign, a relative error below
    4 u, hence ``gamma_{4m} (|B| |A| |src|)[y]`` on top."""
    src = np.random.default_rng(m + rows).standard_normal((rows, (1 << m) + 3))
    A = _confusion(m, 50 + m)
    a = _kron(T, src, m, A)
    assert _kron(T, src, m, A).tobytes() == a.tobytes()
    head = _kron(T, np.ascontiguousarray(src[:3]), m, A)
    assert head.tobytes() == np.ascontiguousarray(a[:3]).tobytes()
    assert _kron_in_place(T, src, m, A).tobytes() == a.tobytes()
    x = src[:, :1 << m].astype(np.longdouble)
    ref = ob.kron2_host(x, m, A)
    bound_a = gamma(2 * m) * ob.kron2_host(np.abs(x), m, np.abs(A))
    err = np.abs(a.astype(np.longdouble) - ref)
    print(f"max err / bound = {float((err / bound_a).max()):.3g}")
    assert np.all(err <= bound_a)

    B = ob.invert_channels(A)
    back = _kron(T, np.ascontiguousarray(a), m, B).astype(np.longdouble)
    bound_b = gamma(2 * m) * ob.kron2_host(np.abs(a).astype(np.longdouble), m, np.abs(B))
    both = bound_b + ob.kron2_host(bound_a, m, np.abs(B))
    err = np.abs(back - ob.kron2_host(ref, m, B))
    print(f"round trip: max err / bound = {float((err / both).max()):.3g}")
    assert np.all(err <= both)
    inverse = gamma(4 * m) * ob.kron2_host(ob.kron2_host(np.abs(x), m, np.abs(A)), m, np.abs(B))
    assert np.all(np.abs(back - x) <= both + inverse)


# ----------------------------------------------------------------------------- 4. bad arguments
def test_kron2_rows_entry_rejects_bad_arguments(T):
    """Every bad argument returns a non-zero status with qk_last_error set, and nothing is launched."""
    import ctypes

    ctx = engine.get_context(0)
    lib = ctx.lib
    buf = T.zeros(200, dtype=T.float64, device="cuda")
    p = buf.data_ptr()
    flip = [0.0, 1.0, 1.0, 0.0]
    good = (ctypes.c_double * 16)(*(flip * 4))

    def call(rows=2, m=4, coef=good, src_p=p, ld_src=16, dst_p=p + 8 * 100, ld_dst=16):
        return lib.qk_kron2_rows(ctx.handle, rows, m, coef, src_p, ld_src, dst_p, ld_dst)

    assert call() == 0
    assert call(dst_p=p) == 0  # in place
    assert call(rows=0, src_p=None, dst_p=None) != 0 and call(rows=0) == 0
    assert call(m=0, coef=None, ld_src=1, ld_dst=1) == 0  # no bit, no matrix
    bad = {"m must be in": dict(m=31), "m must be": dict(m=-1), "null buffer": dict(src_p=None),
           "ld_src": dict(ld_src=15), "ld_dst": dict(ld_dst=15), "rows": dict(rows=-1),
           "overlap": dict(dst_p=p, ld_dst=17), "null coef": dict(coef=None)}
    for value in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 7, 15):
            coef = (ctypes.c_double * 16)(*(flip * 4))
            coef[at] = value
            assert call(coef=coef) != 0, (value, at)
            assert b"finite" in lib.qk_last_error(ctx.handle)
    for msg, kw in bad.items():
        assert call(**kw) != 0, kw
        assert msg.encode() in lib.qk_last_error(ctx.handle), (kw, lib.qk_last_error(ctx.handle))
    assert call(dst_p=None) != 0 and b"null buffer" in lib.qk_last_error(ctx.handle)
    assert call(dst_p=p + 8 * 8) != 0 and b"overlap" in lib.qk_last_error(ctx.handle)  # shifted by half a row
    assert lib.qk_kron2_rows(None, 2, 4, good, p, 16, p, 16) != 0
    T.cuda.synchronize()
    assert not buf.any()


def test_engine_kron2_rows_raises_before_any_launch(T):
    ctx = engine.get_context(0)
    src = T.zeros((4, 16), dtype=T.float64, device="cuda")
    wide = T.zeros((4, 40), dtype=T.float64, device="cuda")
    flips = np.tile(np.array([[0.0, 1.0], [1.0, 0.0]]), (4, 1, 1))
    for kw in (dict(m=31), dict(m=-1), dict(m=5),  # 2^5 columns are not there
               dict(out=T.zeros((4, 8), dtype=T.float64, device="cuda")),
               dict(out=T.zeros((3, 16), dtype=T.float64, device="cuda")),
               dict(out=T.zeros((4, 16), dtype=T.float32, device="cuda")),
               dict(out=T.zeros((4, 32), dtype=T.float64, device="cuda")[:, ::2])):
        with pytest.raises(ValueError):
            engine.kron2_rows(ctx, src, flips, **kw)
    for bad_src in (src.float(), wide[:, ::2], src[0], wide[:, :24]):  # dtype, column stride, rank, 24 columns
        with pytest.raises(ValueError):
            engine.kron2_rows(ctx, bad_src, flips)
    nan, inf = flips.copy(), flips.copy()
    nan[2, 0, 1], inf[3, 1, 1] = np.nan, np.inf
    for bad_mats, msg in ((flips[:3], "shape"), (np.tile(flips[:1], (5, 1, 1)), "shape"), (flips.reshape(4, 4), "shape"),
                          (flips[0], "shape"), (nan, "finite"), (inf, "finite")):
        with pytest.raises(ValueError, match=msg):
            engine.kron2_rows(ctx, src, bad_mats)
    with pytest.raises(ValueError, match="overlap"):
        engine.kron2_rows(ctx, wide[:, :16], flips, out=wide[:, 8:24])
    with pytest.raises(ValueError, match="overlap"):
        engine.kron2_rows(ctx, wide[:, :16], flips, out=wide.view(-1)[:4 * 20].view(4, 20)[:, :16])  # same start, other ld
    assert engine.kron2_rows(ctx, src[:0], flips).shape == (0, 16)
    T.cuda.synchronize()
    assert not src.any() and not wide.any()


# ----------------------------------------------------------------------------- 5. reducer vs oracle
CHANNEL_CASES = ("cx_3cuts", "cx_wide", "three_wide", "partial", "many_traced", "same_fragment", "interleaved",
                 "extra_clbit", "hwe_16_1_p2")


def _measured(cut_clbits):
    return sorted(c for fcl in cut_clbits for c in fcl)


def _case_channels(N, measured, seed):
    """Seeded confusion matrices with e0, e1 in [0.01, 0.05] on the measured clbits, the identity elsewhere."""
    mats = np.tile(EYE, (N, 1, 1))
    mats[measured] = _confusion(len(measured), seed, 0.01, 0.05)
    return mats


def _amplification(mats):
    """The product over the clbits of the largest absolute row sum: an entry of R' is a sum of entries of R weighted
    by a row of the Kronecker product, so an error of TOL per entry of R grows by at most this factor."""
    return float(np.abs(mats).sum(axis=-1).max(axis=-1).prod())


@functools.lru_cache(maxsize=None)
def _expected(case, measured):
    """(matrices, their inverses, R' under either, the two tolerances): once per case, left unchanged."""
    _, cut, ref, _ = _case(case)
    N = cut.num_clbits
    mats = _case_channels(N, list(measured), 1000 + len(case))
    inv = ob.invert_channels(mats)
    noisy, mitigated = ob.kron2_host(ref[None], N, mats)[0], ob.kron2_host(ref[None], N, inv)[0]
    for a in (mats, inv, noisy, mitigated):
        a.setflags(write=False)
    tol_e, tol_m = TOL * _amplification(mats), TOL * _amplification(inv)
    assert TOL <= tol_e <= TOL * 1.04 ** N and TOL <= tol_m <= TOL * (1 / 0.9) ** N  # row sums 1 +- (e0 - e1), 1 / det
    return mats, inv, noisy, mitigated, tol_e, tol_m


def _check_reducer_against(T, red, want, tol, rng, what):
    N = red.N
    order = list(range(N))
    rng.shuffle(order)
    sets = [order, list(range(N)), [order[0]], sorted(order[:max(1, N // 2)]), order[:min(N, 3)]]
    for clbits in sets:
        got = red.marginal(clbits).cpu().numpy()
        np.testing.assert_allclose(got, np_marginal(want, clbits), atol=tol, rtol=0, err_msg=f"{what} clbits {clbits}")
    masks = [0, (1 << N) - 1] + [1 << c for c in range(N)] + [rng.getrandbits(N) for _ in range(24)]
    exp = [np_expectation(want, z) for z in masks]
    for method in ("reduce", "spectrum", "fused"):
        np.testing.assert_allclose(red.expectation(masks, method=method), exp, atol=tol, rtol=0, err_msg=f"{what} {method}")
    keys = np.arange(1 << N) if N <= 10 else np.random.default_rng(N).integers(0, 1 << N, size=500)
    np.testing.assert_allclose(red.probabilities(keys).cpu().numpy(), want[keys], atol=tol, rtol=0, err_msg=what)
    assert abs(red.collision_probability() - float((want * want).sum())) <= _moment_band(want, want, tol, want.size), what
    sc = red.scan()
    lin = want.size * tol
    assert abs(sc.mass - want.sum()) <= lin and abs(sc.l1 - np.abs(want).sum()) <= lin, what


@pytest.mark.parametrize("case,factored", [(c, f) for c in CHANNEL_CASES for f in (False, True)
                                           if not (f and c in DIRECT_ONLY)])
def test_channels_on_the_reducer_match_the_map_on_the_oracle_knit(T, case, factored):
    _, cut, ref, _ = _case(case)
    N = cut.num_clbits
    base = KnitReducer(VirtualCircuit(cut), factored=factored)
    assert base.factored == factored
    measured = _measured(base.clbits)
    mats, inv, want_noisy, want_mitigated, tol_e, tol_m = _expected(case, tuple(measured))
    rows = [q.clone() for q in base.qs]
    everything = list(range(N))
    before = (base.marginal(everything).clone(), base.expectation([0, 1, (1 << N) - 1]), base.collision_probability())
    base.z_spectrum()  # a cache of the base reducer that the new ones must not inherit

    noisy = base.with_readout_error(mats)
    mitigated = base.with_readout_mitigation({c: mats[c] for c in measured})  # the dict form
    for red in (noisy, mitigated):
        assert red is not base and red.ctx is base.ctx and red.frags is base.frags and red.ops is base.ops
        assert red.clbits is base.clbits and red.N == N and red.factored == factored
        assert red._spectrum is None and red._transposed is None and red._moment_specs is None and red._spectrum_t is None
        assert all(q.shape == q0.shape and q.data_ptr() != q0.data_ptr() for q, q0 in zip(red.qs, base.qs))
    rng = random.Random(len(case))
    _check_reducer_against(T, noisy, want_noisy, tol_e, rng, (case, "error"))
    _check_reducer_against(T, mitigated, want_mitigated, tol_m, rng, (case, "mitigation"))

    # mitigation undoes the error model; the error model keeps the mass
    undone = noisy.with_readout_mitigation(mats).marginal(everything)
    np.testing.assert_allclose(undone.cpu().numpy(), before[0].cpu().numpy(), atol=tol_m, rtol=0)
    assert abs(noisy.expectation([0])[0] - before[1][0]) <= tol_e
    # the base reducer is untouched: same rows, same bits in its answers
    for q, q0 in zip(base.qs, rows):
        assert T.equal(q, q0)
    assert T.equal(base.marginal(everything), before[0])
    assert base.expectation([0, 1, (1 << N) - 1]).tobytes() == before[1].tobytes()
    assert base.collision_probability() == before[2]


def test_channel_arguments_are_checked_on_the_reducer(T):
    _, cut, _, _ = _case("extra_clbit")
    red = KnitReducer(VirtualCircuit(cut))
    N = red.N
    unmeasured = sorted(set(range(N)) - set(_measured(red.clbits)))
    assert unmeasured
    A = ob.readout_matrix(0.02, 0.03)
    with pytest.raises(ValueError, match="no fragment measures"):
        red.with_channels({unmeasured[0]: A})
    with pytest.raises(ValueError, match="no fragment measures"):
        red.with_readout_error(np.tile(A, (N, 1, 1)))
    with pytest.raises(ValueError, match="stochastic"):
        red.with_readout_error(2 * A)
    with pytest.raises(ValueError, match="stochastic"):
        red.with_readout_error(np.array([[1.1, 0.0], [-0.1, 1.0]]))
    with pytest.raises(ValueError, match="determinant"):
        red.with_readout_mitigation(ob.readout_matrix(0.5, 0.5))
    with pytest.raises(ValueError, match="shape"):
        red.with_channels(np.zeros((N + 1, 2, 2)))
    # one matrix for all: only the measured clbits take it; any real matrix passes with_channels
    flipped = red.with_channels(np.array([[0.0, 1.0], [1.0, 0.0]]))
    ones = sum(1 << c for c in _measured(red.clbits))
    everything = list(range(N))
    keys = np.arange(1 << N)
    np.testing.assert_allclose(flipped.marginal(everything).cpu().numpy()[keys ^ ones],
                               red.marginal(everything).cpu().numpy(), atol=TOL, rtol=0)


# ----------------------------------------------------------------------------- 6. shots
@pytest.mark.parametrize("case", ["cx_3cuts", "three_wide"])
def test_shots_under_readout_error_replay_against_the_noisy_distribution(T, case):
    _, cut, _, _ = _case(case)
    base = KnitReducer(VirtualCircuit(cut))
    N = base.N
    mats, _, want_noisy, _, tol_e, _ = _expected(case, tuple(_measured(base.clbits)))
    noisy = base.with_readout_error(mats)
    seed = 100 + len(case)
    keys = noisy.sample(SHOTS, seed)
    assert keys.shape == (SHOTS,) and keys.dtype == T.int64 and keys.is_cuda
    worst = replay(keys.cpu().numpy(), want_noisy, [list(cl) for cl in noisy.clbits], seed, 2.0 ** N * tol_e)
    print(f"{case}: worst excursion {worst:.3g} of the band")
    assert T.equal(noisy.sample(SHOTS, seed), keys)
    # the identity on every clbit: another reducer with the same rows, hence the same keys
    same = base.with_channels(np.tile(EYE, (N, 1, 1)))
    assert same is not base and all(T.equal(q, q0) for q, q0 in zip(same.qs, base.qs))
    assert T.equal(same.sample(SHOTS, seed), base.sample(SHOTS, seed))


# ----------------------------------------------------------------------------- 7. run.py
def test_run_virtual_circuit_entry_points_take_readout_and_mitigate(T):
    _, cut, _, _ = _case("cx_wide")
    virt = VirtualCircuit(cut)
    base = KnitReducer(virt)
    N = base.N
    mats, _, want_noisy, want_mitigated, tol_e, tol_m = _expected("cx_wide", tuple(_measured(base.clbits)))
    clbits, masks = [12, 0, 5, 7], [0, 5, 1 << 12, (1 << N) - 1]
    got, info = run_virtual_circuit_marginal(virt, clbits, readout=mats, dense=True)
    assert T.equal(got, base.with_readout_error(mats).marginal(clbits))
    np.testing.assert_allclose(got.cpu().numpy(), np_marginal(want_noisy, clbits), atol=tol_e, rtol=0)
    assert info.run_time > 0 and info.knit_time > 0
    vals, _ = run_virtual_circuit_expectation(virt, masks, readout=mats, mitigate=True)
    assert vals.tobytes() == base.with_readout_mitigation(mats).expectation(masks).tobytes()
    np.testing.assert_allclose(vals, [np_expectation(want_mitigated, z) for z in masks], atol=tol_m, rtol=0)
    plain, _ = run_virtual_circuit_marginal(virt, clbits, dense=True)
    with_none, _ = run_virtual_circuit_marginal(virt, clbits, dense=True, readout=None)
    assert T.equal(plain, with_none) and T.equal(plain, base.marginal(clbits))
    assert run_virtual_circuit_expectation(virt, masks, readout=None)[0].tobytes() == base.expectation(masks).tobytes()
    as_dict, _ = run_virtual_circuit_marginal(virt, clbits, readout=ob.readout_matrix(0.02, 0.04))
    assert isinstance(as_dict, dict) and abs(sum(as_dict.values()) - 1.0) <= 1e-9
    with pytest.raises(ValueError, match="stochastic"):
        run_virtual_circuit_marginal(virt, clbits, readout=np.array([[1.0, 0.2], [0.0, 0.9]]))
    with pytest.raises(ValueError, match="stochastic"):
        run_virtual_circuit_expectation(virt, masks, readout=2 * EYE, mitigate=True)
    with pytest.raises(ValueError, match="readout"):
        run_virtual_circuit_expectation(virt, masks, mitigate=True)


# ----------------------------------------------------------------------------- 8. wide output
def test_wide_36_clbit_readout_error_scales_every_z_string_by_its_closed_form(T):
    """hwe 36 in two 18-qubit fragments with one CX cut (the dense result would be 2^36 fp64 = 550 GB) under a
    symmetric flip e_c per clbit: ``[[1 - e, e], [e, 1 - e]]`` has the eigenvector (1, -1) with eigenvalue 1 - 2 e, so
    ``<Z_mask>`` of the noisy knit is ``prod_{c in mask} (1 - 2 e_c)`` times that of the base knit, and no 2^36 object
    is needed to say so. Memory: the new reducer adds one copy of the swept rows to what the base reducer's own calls
    take (1 MiB of allowance for the allocator's rounding of small blocks), and nothing comes near a 2^N buffer
    (the bound of the other wide tests)."""
    _, cut, _ = cutting.config_cut_circuit("hwe", 36, 1, 2)
    N = 36
    e = np.random.default_rng(36).uniform(0.01, 0.05, size=N)
    mats = np.stack([ob.readout_matrix(x, x) for x in e])
    rng = random.Random(36)
    masks = [0, (1 << N) - 1, 1, 1 << 35, (1 << 17) | (1 << 18)] + [rng.getrandbits(N) for _ in range(195)]
    scale = np.array([np.prod([1 - 2 * e[c] for c in range(N) if z >> c & 1]) for z in masks])

    T.cuda.synchronize()
    T.cuda.reset_peak_memory_stats()
    base = KnitReducer(VirtualCircuit(cut))
    assert [len(cl) for cl in base.clbits] == [18, 18]
    rows_bytes = sum(q.numel() * 8 for q in base.qs)
    T.cuda.synchronize()
    held = T.cuda.memory_allocated()
    T.cuda.reset_peak_memory_stats()
    want = base.expectation(masks)
    T.cuda.synchronize()
    base_extra = T.cuda.max_memory_allocated() - held
    T.cuda.reset_peak_memory_stats()
    noisy = base.with_readout_error(mats)
    got = noisy.expectation(masks)
    T.cuda.synchronize()
    peak = T.cuda.max_memory_allocated()
    print(f"rows {rows_bytes / 2**20:.1f} MiB, base calls {base_extra / 2**20:.1f} MiB, peak {peak / 2**20:.1f} MiB")
    assert peak - held <= rows_bytes + base_extra + (1 << 20)
    assert peak < 1 << 30  # no 2^N buffer anywhere
    np.testing.assert_allclose(got, scale * want, atol=TOL, rtol=0)
    assert abs(got[0] - 1.0) <= TOL
