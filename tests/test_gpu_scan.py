"""The streamed scan on the GPU: ``qk_knit_scan`` / ``qk_knit_collect`` against numpy and the longdouble model, and
``KnitReducer.scan`` / ``top_k`` / ``heavy_outputs`` / ``hellinger_fidelity`` and the ``run_virtual_circuit_scan`` /
``_top_k`` / ``_fidelity`` entry points against the oracle's dense knit."""
import ctypes
import functools
import math

import numpy as np
import pytest

import circuits
import obs_cases
from oracle import dense
from test_gpu_lookup import CASES, DIRECT_ONLY, _case
from test_observables import np_marginal

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (RunTimeInfo, VirtualCircuit, cutting, engine,
                                                                      fidelity, observables,
                                                                      run_virtual_circuit_fidelity,
                                                                      run_virtual_circuit_scan,
                                                                      run_virtual_circuit_top_k)
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.circuit import (ClassicalRegister, QuantumCircuit,
                                                                              QuantumRegister)
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.cutting import CutSpec, cut_circuit
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import (SCAN_BINS, KnitReducer, KnitScan,
                                                                                  histogram_threshold,
                                                                                  knit_scan_host, scan_bin,
                                                                                  scan_group_tiles, scan_shape)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
TOL = 1e-12  # the project's parity tolerance, per entry of the knit
KS = (1, 3, 16, 17, 65)
SHAPES = [(ma, mb) for ma in (0, 1, 6, 7, 8) for mb in (0, 1, 7, 8)]  # the 128 tile edge and both degenerate sides
PAD = 1e300
NAMES = engine.SCAN_STATS


@pytest.fixture(scope="module")
def T(require_gpu):
    import torch

    return torch


def _padded(T, host_rows, pad):
    """The rows on the device inside a wider buffer whose other columns hold 1e300: (buffer, view)."""
    K, W = host_rows.shape
    host = np.full((K, W + pad), PAD)
    host[:, :W] = host_rows
    buf = T.from_numpy(host).cuda()
    return buf, buf[:, :W]


def _raw_scan(T, A, B, A2=None, B2=None, i0=0, i1=None, tau=0.0, entropy=False, hist=True):
    """One ``qk_knit_scan`` call on ``[i0, i1)``: (stats float64 [16], counts int64 [4], hist int64 [128] or None)."""
    ctx = engine.get_context(0)
    K, ma, lda = engine._scan_side("A", A)
    _, mb, ldb = engine._scan_side("B", B, K)
    i1 = 1 << ma if i1 is None else i1
    K2 = lda2 = ldb2 = 0
    if A2 is not None:
        K2, _, lda2 = engine._scan_side("A2", A2)
        _, _, ldb2 = engine._scan_side("B2", B2, K2)
    need = ctypes.c_int64()
    assert ctx.lib.qk_knit_scan_workspace_bytes(ma, mb, i0, i1, ctypes.byref(need)) == 0
    assert need.value == scan_shape(ma, mb, i0, i1)["workspace_bytes"]
    work = T.empty(need.value // 8, dtype=T.float64, device="cuda")
    stats = T.full((16,), 7.0, dtype=T.float64, device="cuda")
    counts = T.full((4,), -7, dtype=T.int64, device="cuda")
    h = T.full((SCAN_BINS,), -7, dtype=T.int64, device="cuda") if hist else None
    ctx.check(ctx.lib.qk_knit_scan(ctx.handle, K, ma, mb, A.data_ptr(), lda, B.data_ptr(), ldb, K2,
                                   None if A2 is None else A2.data_ptr(), lda2, None if B2 is None else B2.data_ptr(),
                                   ldb2, i0, i1, 1 if entropy else 0, tau, stats.data_ptr(), counts.data_ptr(),
                                   h.data_ptr() if hist else None, work.data_ptr(), need.value), "qk_knit_scan")
    return stats.cpu().numpy(), counts.cpu().numpy(), h.cpu().numpy() if hist else None


def _numpy_stats(R, R2=None, tau=0.0):
    """The statistics of a dense float64 knit ``R [2^ma, 2^mb]`` by numpy, named as engine.knit_scan names them."""
    P = np.maximum(R, 0)
    flat = R.reshape(-1)
    out = dict(sum=R.sum(), abs=np.abs(R).sum(), pos=P.sum(), sq=(R * R).sum(), max=R.max(), min=R.min(),
               count_tau=int((R > tau).sum()), count_pos=int((R > 0).sum()), argmax=int(np.argmax(flat)),
               argmin=int(np.argmin(flat)), hist=np.bincount(scan_bin(flat[flat > 0]), minlength=SCAN_BINS))
    if R2 is not None:
        P2 = np.maximum(R2, 0)
        out.update(sum2=R2.sum(), pos2=P2.sum(), cross=(R * R2).sum(), l1d=np.abs(R - R2).sum(),
                   maxd=np.abs(R - R2).max(), hell=np.sqrt(P * P2).sum())
    return out


EXACT = ("sum", "abs", "pos", "sq", "max", "min", "sum2", "pos2", "cross", "l1d", "maxd")


def _assert_exact(got, want, what):
    for name in EXACT + ("count_tau", "count_pos", "argmax", "argmin"):
        if name in want:
            assert got[name] == want[name], (what, name, got[name], want[name])
    assert np.array_equal(got["hist"], want["hist"]), what


# ----------------------------------------------------------------------------- 1. exact on small integers
@pytest.mark.parametrize("K", KS)
def test_scan_is_exact_on_small_integers_for_every_shape(T, K):
    """Entries in -3..3: every sum is an integer far below 2^53, so every statistic, count, histogram bin and index
    equals numpy's bit for bit, in any order of summation. The column of A (of B where A has one) that gives the
    maximum is copied to its neighbour, so the maximum is taken at least twice: the lowest flat index is reported."""
    ctx = engine.get_context(0)
    K2 = max(1, K - 1)
    for ma, mb in SHAPES:
        rng = np.random.default_rng(1000 * K + 10 * ma + mb)
        Ah, Bh = rng.integers(-3, 4, size=(K, 1 << ma)), rng.integers(-3, 4, size=(K, 1 << mb))
        A2h, B2h = rng.integers(-3, 4, size=(K2, 1 << ma)), rng.integers(-3, 4, size=(K2, 1 << mb))
        i, j = np.unravel_index(np.argmax(Ah.T @ Bh), (1 << ma, 1 << mb))
        if ma:  # another row of the knit equals the one that holds the maximum
            Ah[:, (i + 1) % (1 << ma)] = Ah[:, i]
        elif mb:
            Bh[:, (j + 1) % (1 << mb)] = Bh[:, j]
        bufs = [_padded(T, X.astype(np.float64), pad) for X, pad in ((Ah, 3), (Bh, 5), (A2h, 1), (B2h, 2))]
        keep = [b.clone() for b, _ in bufs]
        A, B, A2, B2 = (v for _, v in bufs)
        R, R2 = (Ah.T @ Bh).astype(np.float64), (A2h.T @ B2h).astype(np.float64)
        tau = float(np.sort(R.reshape(-1))[R.size // 2])  # a value the knit takes: the comparison is strict
        want = _numpy_stats(R, R2, tau)
        got = engine.knit_scan(ctx, A, B, A2, B2, tau=tau, entropy=True, hist=True)
        assert all(np.isfinite(got[n]) and abs(got[n]) < 1e100 for n in NAMES), "the padding was read"
        _assert_exact(got, want, (K, ma, mb))
        if ma + mb:
            assert int((R.reshape(-1) == R.max()).sum()) >= 2
        n = R.size
        P, P2 = np.maximum(R, 0), np.maximum(R2, 0)
        lnP = np.log(np.where(P > 0, P, 1.0))
        assert abs(got["ent"] + (P * lnP).sum()) <= (K + n + 8) * EPS * ((np.abs(lnP) + 1) * P).sum()
        assert abs(got["hell"] - want["hell"]) <= (K + n + 8) * EPS * want["hell"]
        single = engine.knit_scan(ctx, A, B, tau=tau)  # no second knit, no entropy, no histogram
        _assert_exact(dict(single, hist=want["hist"]), _numpy_stats(R, None, tau), (K, ma, mb, "single"))
        assert single["hist"] is None and single["ent"] == 0.0 and all(single[s] == 0.0 for s in NAMES[7:])
        for (b, _), k in zip(bufs, keep):
            assert T.equal(b, k), "an input was written"


def test_scan_is_exact_where_a_workgroup_owns_several_tiles(T):
    """2^17 x 2^7 outputs: 1024 tiles on 512 workgroups, two each; the reference blockwise in float64."""
    ctx = engine.get_context(0)
    ma, mb, K = 17, 7, 3
    sh = scan_shape(ma, mb)
    assert sh["tiles"] == 1024 and sh["groups"] == 512 and len(scan_group_tiles(sh, 5)) == 2
    rng = np.random.default_rng(17)
    Ah, Bh = rng.integers(-3, 4, size=(K, 1 << ma)), rng.integers(-3, 4, size=(K, 1 << mb))
    i = int(np.argmax((Ah.T @ Bh).max(axis=1)))
    Ah[:, (i + 70000) % (1 << ma)] = Ah[:, i]  # the maximum again, in another workgroup's tile
    (_, A), (_, B) = _padded(T, Ah.astype(np.float64), 1), _padded(T, Bh.astype(np.float64), 3)
    R = np.concatenate([(Ah[:, i:i + 4096].T @ Bh).astype(np.float64) for i in range(0, 1 << ma, 4096)])
    got = engine.knit_scan(ctx, A, B, A, B, tau=2.0, entropy=False, hist=True)
    _assert_exact(got, _numpy_stats(R, R, 2.0), "two tiles per workgroup")
    assert got["l1d"] == 0.0 and got["maxd"] == 0.0 and got["cross"] == got["sq"]


def test_scan_of_row_ranges_combines_to_the_whole(T):
    ma, mb, K = 8, 7, 17
    rng = np.random.default_rng(8)
    Ah, Bh = rng.integers(-3, 4, size=(K, 1 << ma)), rng.integers(-3, 4, size=(K, 1 << mb))
    (_, A), (_, B) = _padded(T, Ah.astype(np.float64), 1), _padded(T, Bh.astype(np.float64), 1)
    R = (Ah.T @ Bh).astype(np.float64)
    whole = _raw_scan(T, A, B, tau=1.0)
    parts = [(0, 3), (3, 200), (200, 256)]
    raws = [_raw_scan(T, A, B, i0=i0, i1=i1, tau=1.0) for i0, i1 in parts]
    for (i0, i1), (st, ct, h) in zip(parts, raws):
        want = _numpy_stats(R[i0:i1], None, 1.0)
        got = dict(zip(NAMES, st[:13]), count_tau=ct[0], count_pos=ct[1], argmax=ct[2] - (i0 << mb),
                   argmin=ct[3] - (i0 << mb), hist=h)
        _assert_exact(got, want, (i0, i1))
    for slot in (0, 1, 2, 3):
        assert sum(st[slot] for st, _, _ in raws) == whole[0][slot]
    assert max(st[5] for st, _, _ in raws) == whole[0][5] and min(st[6] for st, _, _ in raws) == whole[0][6]
    assert sum(ct[:2] for _, ct, _ in raws).tolist() == whole[1][:2].tolist()
    assert np.array_equal(sum(h for _, _, h in raws), whole[2])
    first = next(i for i, (st, _, _) in enumerate(raws) if st[5] == whole[0][5])
    assert raws[first][1][2] == whole[1][2] == int(np.argmax(R.reshape(-1)))


# ----------------------------------------------------------------------------- 2. random data, derived bands
RANDOM_SHAPES = [(0, 0), (1, 1), (6, 7), (7, 7), (8, 8), (8, 0), (0, 8), (7, 1), (1, 8)]


@pytest.mark.parametrize("K", KS)
def test_scan_of_random_signed_data_within_the_derived_bands(T, K):
    """With u = 2^-53, n outputs and S_ij = sum_k |A_k[i]| |B_k[j]|: an output is within K u S_ij of its exact
    value and a sum of n terms adds n u of the sum of their magnitudes, so SUM, ABS, POS (SUM2, POS2 with S') lie
    within (K + n) u sum S, SQ and CROSS within (2K + 2 + n) u sum S S', MAX and MIN within K u max S.
    L1D and MAXD are the ABS and the extremum of the difference knit D = R - R', a knit of K + K' terms whose S is
    S + S': a difference carries the roundings of both chains and its own, and to first order
    K u S + K' u S' + u |D| <= (K + K') u (S + S') since |D| <= S + S'. So L1D lies within (K + K' + n) u
    sum (S + S') and MAXD within (K + K') u max (S + S'). With S alone and K alone no arithmetic meets them: at
    K = K' = 1, n = 1 the three roundings of fl(fl(a b) - fl(a' b')) reach 1.35 (K + n) u S on the first shape
    here, and 1.44 K u max (S + S') on the 2^6 x 2^7 one."""
    ctx = engine.get_context(0)
    K2 = max(1, K - 1)
    worst = dict.fromkeys(("sum", "abs", "pos", "l1d", "sum2", "pos2", "sq", "cross", "max", "min", "maxd"), 0.0)
    for ma, mb in RANDOM_SHAPES:
        rng = np.random.default_rng(77 * K + 10 * ma + mb)
        hosts = [rng.standard_normal((K, 1 << ma)), rng.standard_normal((K, 1 << mb)),
                 rng.standard_normal((K2, 1 << ma)), rng.standard_normal((K2, 1 << mb))]
        A, B, A2, B2 = (_padded(T, X, 3)[1] for X in hosts)
        model = knit_scan_host([hosts[1], hosts[0]], [hosts[3], hosts[2]], tau=0.1)  # side B in the low bits
        got = engine.knit_scan(ctx, A, B, A2, B2, tau=0.1, hist=True)
        S, S2 = np.abs(hosts[0]).T @ np.abs(hosts[1]), np.abs(hosts[2]).T @ np.abs(hosts[3])
        n = S.size
        bands = dict(sum=(K + n) * EPS * S.sum(), sum2=(K + n) * EPS * S2.sum(), sq=(2 * K + 2 + n) * EPS * (S * S).sum(),
                     cross=(2 * K + 2 + n) * EPS * (S * S2).sum(), max=K * EPS * S.max(),
                     maxd=(K + K2) * EPS * (S + S2).max(), l1d=(K + K2 + n) * EPS * (S + S2).sum())
        bands.update(abs=bands["sum"], pos=bands["sum"], pos2=bands["sum2"], min=bands["max"])
        for name, band in bands.items():
            err = abs(np.longdouble(got[name]) - model[name])
            assert err <= band, (K, ma, mb, name, float(err / band))
            worst[name] = max(worst[name], float(err / band))
        assert got["count_tau"] == model["count_tau"] and got["count_pos"] == model["count_pos"]
        assert np.array_equal(got["hist"], model["hist"])
        assert abs(model["values"][got["argmax"]] - model["max"]) <= bands["max"]
        assert abs(model["values"][got["argmin"]] - model["min"]) <= bands["max"]
    print(f"K = {K}: worst fraction of each band: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("K", KS)
def test_entropy_and_hellinger_sums_of_non_negative_operands(T, K):
    """No cancellation: S = R. ENT within (K + n + 8) u sum (|ln R| + 1) R, HELL within (K + n + 8) u sum
    sqrt(R R'), R and R' the longdouble model's values."""
    ctx = engine.get_context(0)
    worst = [0.0, 0.0]
    for ma, mb in RANDOM_SHAPES:
        rng = np.random.default_rng(91 * K + 10 * ma + mb)
        hosts = [rng.uniform(0, 1, (K, 1 << ma)), rng.uniform(0, 1, (K, 1 << mb)),
                 rng.uniform(0, 1, (K, 1 << ma)), rng.uniform(0, 1, (K, 1 << mb))]
        A, B, A2, B2 = (_padded(T, X, 1)[1] for X in hosts)
        model = knit_scan_host([hosts[1], hosts[0]], [hosts[3], hosts[2]])
        R, R2 = model["values"], model["values2"]
        n = R.size
        got = engine.knit_scan(ctx, A, B, A2, B2, entropy=True)
        b_ent = (K + n + 8) * EPS * ((np.abs(np.log(R)) + 1) * R).sum()
        b_hell = (K + n + 8) * EPS * np.sqrt(R * R2).sum()
        e_ent, e_hell = abs(np.longdouble(got["ent"]) - model["ent"]), abs(np.longdouble(got["hell"]) - model["hell"])
        assert e_ent <= b_ent and e_hell <= b_hell, (K, ma, mb, float(e_ent / b_ent), float(e_hell / b_hell))
        worst = [max(worst[0], float(e_ent / b_ent)), max(worst[1], float(e_hell / b_hell))]
        assert engine.knit_scan(ctx, A, B, A2, B2)["ent"] == 0.0  # only under the flag
    print(f"K = {K}: worst fraction of the band: ENT {worst[0]:.3g}, HELL {worst[1]:.3g}")


# ----------------------------------------------------------------------------- 3. determinism, collect
def test_scan_and_collect_are_deterministic(T):
    ctx = engine.get_context(0)
    rng = np.random.default_rng(3)
    K, ma, mb = 17, 10, 9  # 32 tiles
    Ah, Bh = rng.standard_normal((K, 1 << ma)), rng.standard_normal((K, 1 << mb))
    (_, A), (_, B) = _padded(T, Ah, 3), _padded(T, Bh, 1)
    a = _raw_scan(T, A, B, A, B, tau=0.5, entropy=True)
    b = _raw_scan(T, A, B, A, B, tau=0.5, entropy=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    tau = 6.0
    idx, vals, count = engine.knit_collect(ctx, A, B, tau, 1 << 16)
    st = engine.knit_scan(ctx, A, B, tau=tau)
    assert 0 < count == st["count_tau"] == idx.numel() == vals.numel() <= 1 << 16
    top = int(vals.argmax())
    assert float(vals[top]) == st["max"] and int(idx[top]) == st["argmax"]  # the same mainloop: the same bits
    R = Ah.T @ Bh
    order = np.argsort(idx.cpu().numpy())
    assert np.array_equal(idx.cpu().numpy()[order], np.flatnonzero(R.reshape(-1) > tau))
    idx2, vals2, count2 = engine.knit_collect(ctx, A, B, tau, 1 << 16)
    order2 = np.argsort(idx2.cpu().numpy())
    assert count2 == count and np.array_equal(idx.cpu().numpy()[order], idx2.cpu().numpy()[order2])
    assert vals.cpu().numpy()[order].tobytes() == vals2.cpu().numpy()[order2].tobytes()
    assert np.abs(vals.cpu().numpy()[order] - R.reshape(-1)[idx.cpu().numpy()[order]]).max() <= K * EPS * (
        np.abs(Ah).T @ np.abs(Bh)).max()


def test_collect_overflow_reports_the_count_and_writes_nothing_past_capacity(T):
    ctx = engine.get_context(0)
    rng = np.random.default_rng(4)
    K, ma, mb = 3, 8, 7
    Ah, Bh = rng.integers(-3, 4, size=(K, 1 << ma)), rng.integers(-3, 4, size=(K, 1 << mb))
    (_, A), (_, B) = _padded(T, Ah.astype(np.float64), 1), _padded(T, Bh.astype(np.float64), 1)
    R = (Ah.T @ Bh).reshape(-1)
    true = int((R > 0).sum())
    cap = 100
    assert true > 4 * cap
    idx = T.full((cap + 64,), -5, dtype=T.int64, device="cuda")
    vals = T.full((cap + 64,), -5.0, dtype=T.float64, device="cuda")
    n = T.full((1,), -5, dtype=T.int64, device="cuda")
    assert ctx.lib.qk_knit_collect(ctx.handle, K, ma, mb, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), 0,
                                   1 << ma, 0.0, cap, idx.data_ptr(), vals.data_ptr(), n.data_ptr()) == 0
    assert int(n[0]) == true
    assert bool((idx[cap:] == -5).all()) and bool((vals[cap:] == -5.0).all()), "written past capacity"
    got_i, got_v = idx[:cap].cpu().numpy(), vals[:cap].cpu().numpy()
    assert len(set(got_i.tolist())) == cap and np.array_equal(R[got_i].astype(np.float64), got_v) and (got_v > 0).all()
    # capacity 0 only counts; the wrapper reports the count with what fitted
    assert ctx.lib.qk_knit_collect(ctx.handle, K, ma, mb, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), 0,
                                   1 << ma, 0.0, 0, None, None, n.data_ptr()) == 0 and int(n[0]) == true
    i3, v3, c3 = engine.knit_collect(ctx, A, B, 0.0, cap)
    assert c3 == true and i3.numel() == v3.numel() == cap


def test_scan_entries_reject_bad_arguments(T):
    """Every bad argument returns a non-zero status with qk_last_error set, and nothing is launched."""
    ctx = engine.get_context(0)
    lib = ctx.lib
    A = T.ones((2, 8), dtype=T.float64, device="cuda")
    B = T.ones((2, 4), dtype=T.float64, device="cuda")
    stats = T.full((16,), 7.0, dtype=T.float64, device="cuda")
    counts = T.full((4,), -7, dtype=T.int64, device="cuda")
    work = T.zeros(64, dtype=T.float64, device="cuda")
    idx = T.full((8,), -7, dtype=T.int64, device="cuda")
    vals = T.full((8,), 7.0, dtype=T.float64, device="cuda")
    n = T.full((1,), -7, dtype=T.int64, device="cuda")
    ok = dict(K=2, ma=3, mb=2, A=A.data_ptr(), lda=8, B=B.data_ptr(), ldb=4, K2=0, A2=None, lda2=0, B2=None, ldb2=0,
              i0=0, i1=8, flags=0, tau=0.0, stats=stats.data_ptr(), counts=counts.data_ptr(), hist=None,
              work=work.data_ptr(), wb=work.numel() * 8)

    def scan(**kw):
        a = dict(ok, **kw)
        return lib.qk_knit_scan(ctx.handle, a["K"], a["ma"], a["mb"], a["A"], a["lda"], a["B"], a["ldb"], a["K2"], a["A2"],
                                a["lda2"], a["B2"], a["ldb2"], a["i0"], a["i1"], a["flags"], a["tau"], a["stats"],
                                a["counts"], a["hist"], a["work"], a["wb"])

    def collect(**kw):
        a = dict(ok, cap=8, idx=idx.data_ptr(), vals=vals.data_ptr(), n=n.data_ptr())
        a.update(kw)
        return lib.qk_knit_collect(ctx.handle, a["K"], a["ma"], a["mb"], a["A"], a["lda"], a["B"], a["ldb"], a["i0"],
                                   a["i1"], a["tau"], a["cap"], a["idx"], a["vals"], a["n"])

    common = [dict(K=0), dict(ma=-1), dict(ma=31), dict(mb=-1), dict(mb=31), dict(A=None), dict(B=None), dict(lda=7),
              dict(ldb=3), dict(i0=-1), dict(i0=8), dict(i1=9), dict(i0=5, i1=5), dict(tau=float("nan"))]
    only_scan = [dict(K2=-1), dict(K2=2), dict(K2=2, A2=A.data_ptr(), lda2=8, B2=B.data_ptr(), ldb2=3), dict(flags=2),
                 dict(stats=None), dict(counts=None), dict(work=None), dict(wb=8)]
    only_collect = [dict(cap=-1), dict(n=None), dict(idx=None), dict(vals=None)]
    for call, cases in ((scan, common + only_scan), (collect, common + only_collect)):
        for kw in cases:
            assert call(**kw) != 0, kw
            assert lib.qk_last_error(ctx.handle), kw
    T.cuda.synchronize()
    assert bool((stats == 7.0).all()) and bool((counts == -7).all()) and bool((idx == -7).all()) and int(n[0]) == -7
    assert scan() == 0 and collect() == 0
    T.cuda.synchronize()
    assert float(stats[0]) == 64.0 and int(n[0]) == 32 and sorted(idx.tolist())[0] >= 0
    with pytest.raises(ValueError, match="power of two"):
        engine.knit_scan(ctx, T.ones((2, 3), dtype=T.float64, device="cuda"), B)
    with pytest.raises(ValueError, match="terms"):
        engine.knit_scan(ctx, A, T.ones((3, 4), dtype=T.float64, device="cuda"))
    with pytest.raises(ValueError, match="both"):
        engine.knit_scan(ctx, A, B, A2=A)


# ----------------------------------------------------------------------------- 4. end to end against the oracle
def _entropy_bits(ref):
    p = np.maximum(ref, 0)
    p = p[p > 0] / p.sum()
    return float(-(p * np.log2(p)).sum())


def _entropy_band(ref, tol_entry):
    """H = (ENT / P + ln P) / ln 2. Per entry -p ln p moves by at most delta (|ln delta| + 1) when p moves by delta
    (its modulus of continuity), P by delta; to first order dH <= (dENT / P + |ENT| dP / P^2 + dP / P) / ln 2."""
    n = ref.size
    p = np.maximum(ref, 0)
    P = float(p.sum())
    ENT = float(-(p[p > 0] * np.log(p[p > 0])).sum())
    d_ent, d_p = n * tol_entry * (abs(math.log(tol_entry)) + 1), n * tol_entry
    return (d_ent / P + abs(ENT) * d_p / P ** 2 + d_p / P) / math.log(2) * 1.01


def _check_scan_against(sc, ref, tol_entry, threshold, what):
    """Every field of a KnitScan against the dense reference ``ref`` whose entries carry ``tol_entry``."""
    n = ref.size
    lin = n * tol_entry
    assert isinstance(sc, KnitScan)
    assert abs(sc.mass - ref.sum()) <= lin and abs(sc.l1 - np.abs(ref).sum()) <= lin, what
    assert abs(sc.positive_mass - np.maximum(ref, 0).sum()) <= lin, what
    assert abs(sc.negativity - (np.abs(ref).sum() - ref.sum()) / 2) <= lin, what
    assert abs(sc.collision - (ref * ref).sum()) <= lin * 2 * np.abs(ref).max(), what
    assert abs(sc.shannon_entropy - _entropy_bits(ref)) <= _entropy_band(ref, tol_entry), what
    assert abs(sc.max - ref.max()) <= tol_entry and abs(sc.min - ref.min()) <= tol_entry, what
    top = np.sort(ref)[::-1]
    if n == 1 or top[0] - top[1] > 2 * tol_entry:
        assert sc.argmax == int(np.argmax(ref)), what
    else:
        assert abs(ref[sc.argmax] - ref.max()) <= 2 * tol_entry, what
    assert abs(ref[sc.argmin] - ref.min()) <= 2 * tol_entry, what
    assert int((ref > threshold + tol_entry).sum()) <= sc.count_above <= int((ref > threshold - tol_entry).sum()), what
    assert int((ref > tol_entry).sum()) <= sc.support <= int((ref > -tol_entry).sum()), what
    assert sc.histogram.shape == (SCAN_BINS,) and int(sc.histogram.sum()) == sc.support, what
    cum = np.cumsum(sc.histogram)
    for b in range(0, 40):  # the bins' edges: cum[b] counts the outputs >= 2^-b
        edge = 2.0 ** -b
        assert int((ref >= edge + tol_entry).sum()) <= cum[b] <= int((ref >= edge - tol_entry).sum()), (what, b)


@pytest.mark.parametrize("case,factored", [(c, f) for c in sorted(CASES) for f in (False, True)
                                           if not (f and c in DIRECT_ONLY)])
def test_scan_top_k_and_heavy_outputs_match_the_oracle(T, case, factored):
    cut, ref = _case(case)
    virt = VirtualCircuit(cut)
    N = virt.circuit.num_clbits
    red = KnitReducer(virt, factored=factored)
    assert red.factored == factored
    threshold = max(float(np.sort(ref)[-max(2, ref.size // 8)]) * 0.999, 1e-9)
    sc = red.scan(threshold=threshold)
    _check_scan_against(sc, ref, TOL, threshold, (case, factored))
    again = red.scan(threshold=threshold)
    assert again.mass == sc.mass and again.shannon_entropy == sc.shannon_entropy and again.argmax == sc.argmax
    assert red.mode() == (sc.argmax, sc.max) and red.shannon_entropy() == sc.shannon_entropy
    assert red.negativity() == sc.negativity
    assert math.isnan(red.scan(entropy=False).shannon_entropy)
    # top_k and heavy_outputs
    order = np.sort(ref)[::-1]
    keys, vals = red.top_k(8)
    assert keys.is_cuda and keys.dtype == T.int64 and vals.dtype == T.float64
    k = min(8, sc.support)
    assert keys.numel() == vals.numel() == k
    v = vals.cpu().numpy()
    assert np.all(np.diff(v) <= 0) and np.abs(v - order[:v.size]).max() <= TOL
    assert np.abs(ref[keys.cpu().numpy()] - v).max() <= TOL and len(set(keys.tolist())) == keys.numel()
    hk, hv = red.heavy_outputs(threshold)
    assert hk.numel() == sc.count_above and bool((hv > threshold).all()) and np.all(np.diff(hv.cpu().numpy()) <= 0)
    assert np.abs(ref[hk.cpu().numpy()] - hv.cpu().numpy()).max() <= TOL
    assert float(hv[0]) == sc.max and sc.argmax in hk[hv == hv[0]].tolist()
    ties = np.flatnonzero(np.diff(hv.cpu().numpy()) == 0)
    assert np.all(hk.cpu().numpy()[ties] < hk.cpu().numpy()[ties + 1])  # equal values: ascending keys
    with pytest.raises(ValueError, match=str(sc.count_above)):
        red.heavy_outputs(threshold, capacity=sc.count_above - 1)
    all_k, all_v = red.top_k(1 << N)  # more than the support: every positive outcome
    assert all_k.numel() == sc.support and bool((all_v > 0).all())
    assert red.top_k(0)[0].numel() == 0
    # cross-route consistency, each within the sum of the two routes' bands
    n = ref.size
    assert abs(sc.collision - red.collision_probability()) <= 2 * n * TOL * 2 * np.abs(ref).max()
    assert abs(sc.mass - float(red.expectation([0])[0])) <= 2 * n * TOL
    assert abs(float(red.probabilities([sc.argmax])[0]) - sc.max) <= 2 * TOL
    assert float((red.probabilities(keys) - vals).abs().max()) <= 2 * TOL


@pytest.mark.parametrize("case", ["cx_wide", "three_wide", "interleaved", "extra_clbit", "partial"])
def test_scan_over_chosen_clbits_is_that_of_the_marginal(T, case):
    """A set that straddles the cut, in non-ascending order: bit i of a key is clbits[i]. An entry of a marginal
    sums up to 2^N entries of the knit, so it carries 2^N * 1e-12."""
    cut, ref = _case(case)
    virt = VirtualCircuit(cut)
    N = virt.circuit.num_clbits
    red = KnitReducer(virt)
    fcl = [cl for cl in red.clbits if cl]
    straddle = sorted({fcl[0][0], fcl[0][-1], fcl[1][0], fcl[-1][-1]}, reverse=True)
    assert straddle != sorted(straddle)
    tol = (1 << N) * TOL
    for clbits in (straddle, straddle[:1], []):
        marg = np_marginal(ref, clbits)
        _check_scan_against(red.scan(clbits, threshold=0.01), marg, tol, 0.01, (case, clbits))
        keys, vals = red.top_k(3, clbits)
        order = np.sort(marg)[::-1]
        assert np.abs(vals.cpu().numpy() - order[:vals.numel()]).max() <= tol
        assert np.abs(marg[keys.cpu().numpy()] - vals.cpu().numpy()).max() <= tol
    if case == "extra_clbit":  # clbits 1 and 3 are never written: their keys hold exact zeros
        sc = red.scan()
        assert sc.min <= 0.0 and sc.support <= 8 and red.scan([1, 3]).support == 1
    with pytest.raises(ValueError, match="duplicate"):
        red.scan([0, 0])
    with pytest.raises(ValueError, match="outside"):
        red.top_k(2, [N])


def _fidelity_band(p, q, tol_entry):
    """F = H^2 / (P Q), H = sum sqrt(p q). Per entry sqrt(p q) moves by at most sqrt(delta p) + sqrt(delta q) + delta
    when both move by delta; to first order dF <= 2 H dH / (P Q) + F (dP / P + dQ / Q)."""
    p, q = np.maximum(p, 0), np.maximum(q, 0)
    P, Q, H = float(p.sum()), float(q.sum()), float(np.sqrt(p * q).sum())
    d_h = float((np.sqrt(tol_entry * p) + np.sqrt(tol_entry * q) + tol_entry).sum())
    d_p = p.size * tol_entry
    return (2 * H * d_h / (P * Q) + H * H / (P * Q) * (d_p / P + d_p / Q)) * 1.01


@functools.lru_cache(maxsize=None)
def _pair(seed, straight=False):
    measure = {0: 0, 1: 1, 2: 2, 3: 3} if straight else {0: 0, 1: 2, 2: 1, 3: 3}
    _, cut = obs_cases._two_by_two(seed, 4, measure)
    ref = dense.run_dense(cut)
    ref.setflags(write=False)
    return cut, ref


def _dict(ref):
    return {k: float(v) for k, v in enumerate(ref)}


@pytest.mark.parametrize("factored", [False, True])
def test_fidelity_distance_and_difference_of_two_knits(T, factored):
    (cut_a, ref_a), (cut_b, ref_b) = _pair(22), _pair(23)
    a = KnitReducer(VirtualCircuit(cut_a), factored=factored)
    b = KnitReducer(VirtualCircuit(cut_b), factored=factored)
    want = fidelity.hellinger_fidelity(_dict(ref_a), _dict(ref_b))
    got = a.hellinger_fidelity(b)
    band = _fidelity_band(ref_a, ref_b, TOL)
    print(f"factored={factored}: fidelity {got:.12g}, dense dicts {want:.12g}, {abs(got - want) / band:.3g} of the band")
    assert abs(got - want) <= band and abs(b.hellinger_fidelity(a) - want) <= band and a.hellinger_fidelity(b) == got
    assert abs(a.hellinger_fidelity(a) - 1) <= _fidelity_band(ref_a, ref_a, TOL)
    assert abs(a.total_variation(b) - np.abs(ref_a - ref_b).sum() / 2) <= 16 * TOL
    assert abs(a.max_difference(b) - np.abs(ref_a - ref_b).max()) <= 2 * TOL
    assert a.total_variation(a) == 0.0 and a.max_difference(a) == 0.0
    ma, mb = np_marginal(ref_a, [3, 0]), np_marginal(ref_b, [3, 0])
    assert abs(a.hellinger_fidelity(b, [3, 0]) - fidelity.hellinger_fidelity(_dict(ma), _dict(mb))) <= _fidelity_band(
        ma, mb, 16 * TOL)
    other = KnitReducer(VirtualCircuit(cut_b), factored=not factored)
    assert abs(a.hellinger_fidelity(other) - want) <= band
    value, info = run_virtual_circuit_fidelity(VirtualCircuit(cut_a), VirtualCircuit(cut_b), factored=factored)
    assert value == got and isinstance(info, RunTimeInfo) and info.run_time > 0 and info.knit_time > 0


def test_fidelity_of_two_cuts_of_one_circuit_and_partition_errors(T):
    """One circuit cut into [0, 1] | [2, 3] and into [0] | [1] | [2, 3]. On the clbits 0, 2, 3 the two cuts
    partition alike (the middle fragment of the second keeps nothing and enters by its row sums) and both knits are
    the same distribution: fidelity 1. On all clbits the partitions differ and match_fragments' error surfaces."""
    import random

    rng = random.Random(5)
    qc = QuantumCircuit(QuantumRegister(4, "q"), ClassicalRegister(4, "c"))
    circuits._rand_layer(qc, range(4), rng)
    g01 = len(qc.data)
    qc.cx(0, 1)
    g12 = len(qc.data)
    qc.cx(1, 2)
    qc.cx(3, 2)
    circuits._rand_layer(qc, range(4), rng)
    for q in range(4):
        qc.measure(q, q)
    cut2 = cut_circuit(qc, CutSpec([[0, 1], [2, 3]], [g12]))
    cut3 = cut_circuit(qc, CutSpec([[0], [1], [2, 3]], [g01, g12]))
    ref2, ref3 = dense.run_dense(cut2), dense.run_dense(cut3)
    assert np.abs(ref2 - ref3).max() <= TOL
    a, b = KnitReducer(VirtualCircuit(cut2)), KnitReducer(VirtualCircuit(cut3))
    for clbits in ([0, 2, 3], [3, 0], [2]):
        m2, m3 = np_marginal(ref2, clbits), np_marginal(ref3, clbits)
        band = _fidelity_band(m2, m3, 16 * TOL)
        want = fidelity.hellinger_fidelity(_dict(m2), _dict(m3))
        assert abs(a.hellinger_fidelity(b, clbits) - want) <= band and abs(want - 1) <= band, clbits
        assert abs(b.hellinger_fidelity(a, clbits) - want) <= band, clbits
        assert a.max_difference(b, clbits) <= 2 * 16 * TOL
    for clbits in (None, [0, 1], [0, 1, 2]):
        with pytest.raises(ValueError, match="differently"):
            a.hellinger_fidelity(b, clbits)
        with pytest.raises(ValueError, match="differently"):
            b.total_variation(a, clbits)
    (cut_s, _), (cut_i, _) = _pair(23, straight=True), _pair(22)
    with pytest.raises(ValueError, match="differently"):
        KnitReducer(VirtualCircuit(cut_i)).max_difference(KnitReducer(VirtualCircuit(cut_s)))
    five = KnitReducer(VirtualCircuit(_case("extra_clbit")[0]))
    with pytest.raises(ValueError, match="clbits against"):
        a.hellinger_fidelity(five)
    with pytest.raises(ValueError, match="KnitReducer"):
        a.hellinger_fidelity(ref2)


# ----------------------------------------------------------------------------- 5. entry points, edge cases
def test_scan_and_top_k_entry_points(T):
    cut, ref = _case("cx_wide")
    virt = VirtualCircuit(cut)
    red = KnitReducer(virt)
    sc, info = run_virtual_circuit_scan(virt, threshold=0.001)
    want = red.scan(threshold=0.001)
    assert isinstance(sc, KnitScan) and sc.mass == want.mass and sc.count_above == want.count_above
    assert sc.shannon_entropy == want.shannon_entropy and np.array_equal(sc.histogram, want.histogram)
    assert isinstance(info, RunTimeInfo) and info.run_time > 0 and info.knit_time > 0
    sc, _ = run_virtual_circuit_scan(virt, [5, 1], factored=False)
    assert sc.argmax == KnitReducer(virt, factored=False).scan([5, 1]).argmax
    top, info = run_virtual_circuit_top_k(virt, 5)
    keys, vals = red.top_k(5)
    assert list(top) == keys.tolist() and list(top.values()) == vals.tolist() and info.knit_time > 0
    for call in (lambda **kw: run_virtual_circuit_scan(virt, **kw), lambda **kw: run_virtual_circuit_top_k(virt, 3, **kw),
                 lambda **kw: run_virtual_circuit_fidelity(virt, virt, **kw)):
        with pytest.raises(ValueError, match="exact"):
            call(sample=True)
        with pytest.raises(ValueError, match="one GPU"):
            call(group="WORLD")


def test_no_fragment_at_all_is_one_outcome(T):
    virt = VirtualCircuit(QuantumCircuit(QuantumRegister(0, "q"), ClassicalRegister(3, "c")))
    red = KnitReducer(virt)
    assert not red.frags
    s = red._scalar
    sc = red.scan()
    assert sc.mass == s == sc.max and sc.argmax == 0 and sc.support == 1 and sc.collision == s * s
    assert sc.shannon_entropy == 0.0 and sc.min == 0.0 and sc.argmin == 1  # seven keys hold exact zeros
    assert red.mode() == (0, s) and red.top_k(4)[0].tolist() == [0] and red.top_k(4)[1].tolist() == [s]
    assert red.hellinger_fidelity(red) == 1.0 and red.total_variation(red, [2, 0]) == 0.0
    value, info = run_virtual_circuit_scan(virt)
    assert value.mass == s and isinstance(info, RunTimeInfo)


def test_a_side_beyond_scan_side_bytes_is_refused(T, monkeypatch):
    cut, _ = _case("cx_wide")
    red = KnitReducer(VirtualCircuit(cut))
    monkeypatch.setattr(observables, "SCAN_SIDE_BYTES", 1 << 8)
    with pytest.raises(ValueError, match=r"K = \d+ terms of \d+ bits"):
        red.scan()
    with pytest.raises(ValueError, match="SCAN_SIDE_BYTES"):
        red.top_k(3)
    monkeypatch.undo()
    assert red.scan().support > 0


def test_top_k_names_the_count_when_a_binade_exceeds_the_capacity(T):
    """The count that top_k would have to collect is known from the histogram before anything is collected."""
    virt = VirtualCircuit(CASES["cx_3cuts"]()[1])
    red = KnitReducer(virt)
    sc = red.scan()
    b = int(np.flatnonzero(np.cumsum(sc.histogram) >= 1)[0])
    with pytest.raises(ValueError, match=str(int(np.cumsum(sc.histogram)[b]))):
        red.top_k(1, capacity=int(np.cumsum(sc.histogram)[b]) - 1)
    with pytest.raises(ValueError, match="negative"):
        red.heavy_outputs(-1.0)


# ----------------------------------------------------------------------------- 6. wide output
def test_wide_output_36_clbits_scan_and_top_k(T):
    """hwe 36 in two 18-qubit fragments: 2^36 outcomes, which nothing can form. The mass is 1, the collision
    probability that of the Gram route, every output is visited exactly once (a threshold of -inf counts them all),
    and the top 16 are the knit at their keys; none of 2^16 drawn shots beats the top one, and none outside the
    top 16 beats the 16th."""
    _, cut, _ = cutting.config_cut_circuit("hwe", 36, 1, 2)
    virt = VirtualCircuit(cut)
    T.cuda.synchronize()
    T.cuda.reset_peak_memory_stats()
    red = KnitReducer(virt)
    assert [len(cl) for cl in red.clbits] == [18, 18]
    K = red.ops.num_terms
    sc = red.scan(threshold=-math.inf, entropy=False)
    n = 1 << 36
    assert sc.count_above == n and 0 < sc.support <= n and int(sc.histogram.sum()) == sc.support
    # an entry within K u S of exact, the sum of n of them within n u sum S: S <= |A|^T |B| summed = prod of l1 norms
    mats = red._operands([(1 << 18) - 1] * 2, [[0]] * 2)
    s_sum = float((mats[0].abs().sum(1) * mats[1].abs().sum(1)).sum())
    assert abs(sc.mass - 1.0) <= (K + n) * EPS * s_sum
    # SQ within (2K + 2 + n) u sum S^2, sum_ij S_ij^2 = sum_kk' (|A||A|^T)[k,k'] (|B||B|^T)[k,k']; the Gram route
    # within 2 * 2^18 * 2^-52 of the same sum (a Gram entry is a dot product of 2^18 terms, per fragment)
    s_sq = float(((mats[0].abs() @ mats[0].abs().T) * (mats[1].abs() @ mats[1].abs().T)).sum())
    coll = red.collision_probability()
    assert abs(sc.collision - coll) <= ((2 * K + 2 + n) * EPS + 2 * (1 << 18) * 2.0 ** -52) * s_sq
    keys, vals = red.top_k(16)
    assert keys.numel() == 16 and float(vals[0]) == sc.max and sc.argmax in keys[vals == vals[0]].tolist()
    Xabs = [X.abs() for X in red.transposed_operands()]
    drawn = red.sample(1 << 16, seed=1)
    every = T.cat([keys, drawn])
    band = 2 * (K + 2) * EPS * engine.knit_at(red.ctx, Xabs, red.clbits, every, 0)
    p = red.probabilities(every)
    assert bool(((p[:16] - vals).abs() <= band[:16]).all())
    # no drawn key beats the top one, and a drawn key outside the top 16 does not beat the 16th
    assert bool((p[16:] <= vals[0] + band[16:]).all())
    outside = ~T.isin(drawn, keys)
    assert bool((p[16:][outside] <= vals[15] + band[16:][outside]).all())
    T.cuda.synchronize()
    peak = T.cuda.max_memory_allocated()
    print(f"hwe 36: mass {sc.mass:.15g}, collision {sc.collision:.6g} (Gram route {coll:.6g}), support {sc.support}, "
          f"max {sc.max:.6g} at {sc.argmax:#x}, peak device memory {peak / 2 ** 20:.1f} MiB")
    assert peak < 1 << 30
