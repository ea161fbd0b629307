#!/usr/bin/env python3
"""Marginals and Z-string expectation values of syc 32 5 without the 2^32 output, against the dense
route (run_virtual_circuit_dense + a torch reduction of the 2^32 output), same process, same box.

HIP events, 3 warm-up rounds, 20 timed repeats each (median and min-max): KnitReducer.marginal onto
16 clbits (0..7 and 16..23), KnitReducer.expectation of 64 and of 1024 masks, the dense route for each
of them, and qk_reduce_bits alone on the larger fragment's swept rows with its achieved read rate
(rows * 2^m * 8 bytes over its time; the rows are cache resident). ``--out FILE`` writes the JSON.

``--shots`` runs the shots leg instead (``--out``: e.g. profiles/obs_bench_shots.json): 20000 shots of
syc 32 5 through KnitReducer.sample (the whole chain, and qk_sample_rows alone on the widest step's
operands), beside the only other route to the same thing in the same process: the dense step, a
torch.cumsum over its 2^32 output and torch.searchsorted of the same number of targets. The three
kernels of qk_sample_rows are timed separately from a kernel trace of a child process
(``rocprofv3 --kernel-trace -- python tools/obs_bench.py --shots-child``): per sample() call the sum of
each kernel's dispatches, median over the calls.

``--spectrum`` runs the all-Z-strings leg instead (``--out``: e.g. profiles/obs_bench_spectrum.json):
qk_wht_rows alone on [64, 2^16] and [256, 2^16] with its achieved bytes/s, the one-off cost of
KnitReducer.z_spectrum(), expectation(method="spectrum") for 16 to 2^20 masks beside the unchanged
expectation(method="reduce") for 16, 64 and 1024, and the smallest measured M at which the spectrum
route with its one-off cost wins.

``--lookup`` runs the probabilities-at-chosen-keys leg instead (``--out``: e.g.
profiles/obs_bench_lookup.json): see lookup_leg.

``--moments`` runs the second-moments leg instead (``--out``: e.g. profiles/obs_bench_moments.json): see
moments_leg.

``--scan`` runs the streamed-scan leg instead (``--out``: e.g. profiles/obs_bench_scan.json): see scan_leg.

``--channels`` runs the per-clbit channels leg instead (``--out``: e.g. profiles/obs_bench_channels.json): see
channels_leg.

``--projection`` runs the nearest-probability-distribution leg instead (``--out``: e.g.
profiles/obs_bench_projection.json): see projection_leg. ``--projected`` the projection as a distribution (``--out``:
profiles/obs_bench_projected.json): see projected_leg. ``--parametric`` the run-time parameter leg (``--out``:
profiles/obs_bench_parametric.json): see parametric_leg. ``--gradient`` the parameter-shift gradient leg (``--out``:
profiles/obs_bench_gradient.json): see gradient_leg."""
import argparse
import glob
import json
import os
import random
import shutil
import sqlite3
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, reps=20, warm=3):
    ms = []
    for i in range(warm + reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(s.elapsed_time(e))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


SHOTS, SHOTS_SEED, CHILD_WARM, CHILD_REPS = 20000, 1, 3, 20
SHOT_KERNELS = ("sr_tile_sums", "sr_tile_scan", "sr_locate")


def shots_child():
    """What the kernel trace sees: CHILD_WARM + CHILD_REPS calls of KnitReducer.sample, nothing else timed."""
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer

    red = KnitReducer(VirtualCircuit(cutting.config_cut_circuit("syc", 32, 5, 2)[1]))
    for _ in range(CHILD_WARM + CHILD_REPS):
        red.sample(SHOTS, SHOTS_SEED)
    torch.cuda.synchronize()


def kernel_split():
    """Per kernel of qk_sample_rows: dispatches per sample() call and the median over the timed calls
    of their summed durations (ms), from the rocpd database of a traced child process."""
    tmp = tempfile.mkdtemp(prefix="obs_bench_shots_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--shots-child"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        dbs = glob.glob(os.path.join(tmp, "**", "*_results.db"), recursive=True)
        if proc.returncode != 0 or not dbs:
            raise RuntimeError(f"kernel trace failed (rc {proc.returncode}): {proc.stderr[-500:]}")
        out = {}
        for db in dbs:
            rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
            for kern in SHOT_KERNELS:
                durs = [d / 1e6 for name, d in rows if kern in name]
                if not durs:
                    continue
                per_call, rest = divmod(len(durs), CHILD_WARM + CHILD_REPS)
                if rest:
                    raise RuntimeError(f"{kern}: {len(durs)} dispatches over {CHILD_WARM + CHILD_REPS} calls")
                calls = sorted(sum(durs[i * per_call:(i + 1) * per_call]) for i in range(CHILD_WARM, CHILD_WARM + CHILD_REPS))
                out[kern] = {"dispatches_per_call": per_call, "median_ms": calls[len(calls) // 2], "min_ms": calls[0],
                             "max_ms": calls[-1]}
        if set(out) != set(SHOT_KERNELS):
            raise RuntimeError(f"kernel trace holds {sorted(out)} of {SHOT_KERNELS}")
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def shots_leg(args):
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20, "shots": SHOTS}
    res["qk_sample_rows_kernels"] = kernel_split()  # first: the child needs the memory the dense route takes later
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    red = KnitReducer(virt)
    ctx = engine.get_context(0)
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    res["terms"] = int(red.ops.num_terms)
    keys = red.sample(SHOTS, SHOTS_SEED)
    res["distinct_keys"] = int(torch.unique(keys).numel())
    res["sample_chain"] = timed(torch, lambda: red.sample(SHOTS, SHOTS_SEED))

    # qk_sample_rows alone on the last step's operands: one row per distinct prefix, K terms, 2^m outcomes
    mats = red._operands([(1 << len(cl)) - 1 for cl in red.clbits], [[0]] * len(red.clbits))
    f = len(mats) - 1
    lead = sum(1 << c for cl in red.clbits[:f] for c in cl)
    pre, inv, counts = torch.unique(keys & lead, return_inverse=True, return_counts=True)
    by_row = torch.argsort(inv, stable=True)
    off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(counts, 0)
    C = torch.rand((counts.numel(), mats[f].shape[0]), dtype=torch.float64, device="cuda")
    u = engine.uniforms(ctx, SHOTS_SEED, f, 0, SHOTS)[by_row]
    t = timed(torch, lambda: engine.sample_rows(ctx, mats[f], C, off, u))
    t.update(rows=int(counts.numel()), K=int(mats[f].shape[0]), m=len(red.clbits[f]), draws=SHOTS)
    t["product_bytes_never_stored"] = t["rows"] * (8 << t["m"])
    t["fma_per_s"] = t["rows"] * t["K"] * (1 << t["m"]) / t["median_ms"] * 1e3
    res["qk_sample_rows_last_step"] = t

    if not args.no_dense:
        u0 = engine.uniforms(ctx, SHOTS_SEED, 0, 0, SHOTS)
        cdf = torch.empty(1 << 32, dtype=torch.float64, device="cuda")

        def dense_shots():
            full, _ = run_virtual_circuit_dense(virt)
            torch.cumsum(full, 0, out=cdf)
            return torch.searchsorted(cdf, u0 * cdf[-1], right=True)

        def tail_only(full):
            torch.cumsum(full, 0, out=cdf)
            return torch.searchsorted(cdf, u0 * cdf[-1], right=True)

        got = dense_shots()
        res["dense_check"] = {"keys_below_2^32": bool((got < (1 << 32)).all()), "total": float(cdf[-1])}
        res["dense_step_only"] = timed(torch, lambda: run_virtual_circuit_dense(virt))
        res["dense_step_cumsum_searchsorted"] = timed(torch, dense_shots)
        full, _ = run_virtual_circuit_dense(virt)
        res["cumsum_searchsorted_only"] = timed(torch, lambda: tail_only(full))
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def spectrum_leg(args):
    """All Z strings at once (``--out``: e.g. profiles/obs_bench_spectrum.json): qk_wht_rows alone, the
    one-off cost of KnitReducer.z_spectrum(), and expectation(method="spectrum") beside the unchanged
    expectation(method="reduce") of the same reducer in the same process."""
    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, observables as ob
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20}
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    red = KnitReducer(VirtualCircuit(cut))
    ctx = engine.get_context(0)
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    res["terms"] = int(red.ops.num_terms)

    kernel = {}
    m = 16
    passes = len(ob.wht_pass_bits(m))
    for rows in (64, 256):
        src = torch.randn((rows, 1 << m), dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)
        for name, fn in (("out_of_place", lambda: engine.wht_rows(ctx, src, m, out=dst)),
                         ("in_place", lambda: engine.wht_rows(ctx, dst, m, out=dst))):
            t = timed(torch, fn)
            t["bytes_moved"] = 2 * passes * rows * (1 << m) * 8
            t["GBs"] = t["bytes_moved"] / t["median_ms"] / 1e6
            kernel[f"rows_{rows}_{name}"] = t
    res["qk_wht_rows"] = {"m": m, "passes": passes, "pass_bits": ob.wht_pass_bits(m), **kernel}

    def spectrum_once():
        red._spectrum = None
        return red.z_spectrum()

    res["z_spectrum_once"] = timed(torch, spectrum_once)
    res["z_spectrum_bytes"] = int(sum(h.numel() * 8 for h in red.z_spectrum()))
    rng = np.random.default_rng(0)
    masks = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.int64)
    for M in (16, 64, 1024, 1 << 17, 1 << 20):
        res[f"spectrum_{M}"] = timed(torch, lambda: red.expectation(masks[:M], method="spectrum"))
    for M in (16, 64, 1024):
        zs = masks[:M].tolist()
        res[f"reduce_{M}"] = timed(torch, lambda: red.expectation(zs, method="reduce"))
    res["check"] = {"spectrum_vs_reduce_max_abs_diff_1024": float(abs(
        red.expectation(masks[:1024], method="spectrum") - red.expectation(masks[:1024].tolist())).max())}
    w = rng.standard_normal(1 << 20)
    res["expectation_sum_2^20"] = timed(torch, lambda: red.expectation_sum(masks, w))
    once = res["z_spectrum_once"]["median_ms"]
    wins = [M for M in (16, 64, 1024) if res[f"spectrum_{M}"]["median_ms"] + once < res[f"reduce_{M}"]["median_ms"]]
    res["crossover"] = {"smallest_measured_M_where_spectrum_plus_once_beats_reduce": wins[0] if wins else None,
                        "measured_M": [16, 64, 1024]}
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def lookup_leg(args):
    """Probabilities at chosen keys (``--out``: e.g. profiles/obs_bench_lookup.json): for M = 2^10, 2^17, 2^20
    uniformly random keys KnitReducer.probabilities, qk_knit_at alone with its achieved bytes/s against
    M * sum_f 8 * ldt bytes, qk_transpose_rows alone, the one-off cost of the transposed operands, and beside
    them in the same process the torch gather route on the same operands (index_select + product + tree,
    KnitReducer._spectrum_chunks applied to X_f), and expectation(method="spectrum") against method="fused" on
    the same masks. At M = 2^10 the dense route as well: run_virtual_circuit_dense(...)[keys]."""
    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20}
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    red = KnitReducer(virt)
    ctx = engine.get_context(0)
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    res["terms"] = int(red.ops.num_terms)

    def transposed_once():
        red._transposed = None
        return red.transposed_operands()

    res["transposed_operands_once"] = timed(torch, transposed_once)
    Xts = red.transposed_operands()
    res["transposed_bytes"] = int(sum(x.numel() * 8 for x in Xts))
    res["ldt"] = int(Xts[0].shape[1])
    mats = engine.fragment_operands(ctx, red.ops, red.qs)
    f = max(range(len(mats)), key=lambda i: mats[i].numel())
    dst = torch.empty_like(Xts[f])
    t = timed(torch, lambda: engine.transpose_rows(ctx, mats[f], len(red.clbits[f]), out=dst))
    t.update(K=int(mats[f].shape[0]), m=len(red.clbits[f]), bytes_moved=int(mats[f].numel() * 8 + dst.numel() * 8))
    t["GBs"] = t["bytes_moved"] / t["median_ms"] / 1e6
    res["qk_transpose_rows"] = t

    class OnOperands:  # KnitReducer._spectrum_chunks with X_f in the place of H_f: the gather route that exists today
        device, clbits = red.device, red.clbits
        z_spectrum = staticmethod(lambda: mats)

    def torch_gather(zs):
        return torch.cat([v for _, v in KnitReducer._spectrum_chunks(OnOperands, zs)])

    rng = np.random.default_rng(0)
    keys = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.int64)
    keys_d = torch.from_numpy(keys).cuda()
    row_bytes = sum(8 * x.shape[1] for x in Xts)
    for M in (1 << 10, 1 << 17, 1 << 20):
        kd, out = keys_d[:M].contiguous(), torch.empty(M, dtype=torch.float64, device="cuda")
        res[f"probabilities_{M}"] = timed(torch, lambda: red.probabilities(kd))
        res[f"probabilities_host_keys_{M}"] = timed(torch, lambda: red.probabilities(keys[:M]))
        t = timed(torch, lambda: engine.knit_at(ctx, Xts, red.clbits, kd, 0, out=out))
        t["bytes_gathered"] = M * row_bytes
        t["GBs"] = t["bytes_gathered"] / t["median_ms"] / 1e6
        res[f"qk_knit_at_{M}"] = t
        res[f"torch_gather_{M}"] = timed(torch, lambda: torch_gather(keys[:M]))
        res[f"expectation_spectrum_{M}"] = timed(torch, lambda: red.expectation(keys[:M], method="spectrum"))
        res[f"expectation_fused_{M}"] = timed(torch, lambda: red.expectation(keys[:M], method="fused"))
    a, b = res[f"qk_knit_at_{1 << 20}"], res[f"torch_gather_{1 << 20}"]
    res["verdict_2^20"] = {"kernel_median_ms": a["median_ms"], "torch_median_ms": b["median_ms"],
                           "kernel_spread_ms": a["max_ms"] - a["min_ms"], "torch_spread_ms": b["max_ms"] - b["min_ms"],
                           "kernel_faster_beyond_both_spreads": b["median_ms"] - a["median_ms"] > max(
                               a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])}
    k10 = keys_d[:1 << 10]
    res["check"] = {
        "kernel_vs_torch_gather_max_abs_diff_2^17": float((red.probabilities(keys_d[:1 << 17])
                                                           - torch_gather(keys[:1 << 17])).abs().max()),
        "fused_vs_spectrum_max_abs_diff_2^17": float(abs(red.expectation(keys[:1 << 17], method="fused")
                                                         - red.expectation(keys[:1 << 17], method="spectrum")).max())}
    if not args.no_dense:
        red._spectrum = red._spectrum_t = None  # the 2^32 output needs the room
        torch.cuda.empty_cache()
        full, _ = run_virtual_circuit_dense(virt)
        res["check"]["kernel_vs_dense_max_abs_diff_2^10"] = float((red.probabilities(k10) - full[k10]).abs().max())
        del full
        res[f"dense_{1 << 10}"] = timed(torch, lambda: run_virtual_circuit_dense(virt)[0][k10])
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def moments_leg(args):
    """Second moments (``--out``: e.g. profiles/obs_bench_moments.json): (a) qk_gram_rows alone on each
    fragment's swept rows of syc 32 5 (the symmetric call, as collision_probability makes it, and the
    two-operand call on a copy), with the bytes it has to read and the flops it issues; (b)
    KnitReducer.collision_probability() end to end; (c) torch's ``A @ A.T`` on the same rows in the same process;
    (d) the only other route to the number: the dense step plus ``(R * R).sum()`` over its 2^32 output."""
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, observables as ob
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20}
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    red = KnitReducer(virt)
    ctx = engine.get_context(0)
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    res["terms"] = int(red.ops.num_terms)

    for q, cl in zip(red.qs, red.clbits):
        R, m = int(q.shape[0]), len(cl)
        sh = ob.gram_split(R, R, m)
        G, copy = torch.empty((R, R), dtype=torch.float64, device="cuda"), q.clone()
        blocks = sh["ba"] * sh["bb"]
        entry = {"rows": R, "m": m, "split": sh["split"], "workgroups": blocks * sh["split"],
                 "workspace_bytes": sh["workspace_bytes"], "source_bytes": R * (8 << m),
                 "mfma_flops": 2 * (blocks * 64 * 64) * (1 << m)}
        for name, fn in (("symmetric", lambda: engine.gram_rows(ctx, q, None, m, out=G)),
                         ("two_operands", lambda: engine.gram_rows(ctx, q, copy, m, out=G))):
            t = timed(torch, fn)
            # a diagonal block reads its rows once, every other block both row sets
            diag = min(sh["ba"], sh["bb"]) if name == "symmetric" else 0
            t["bytes_read"] = (2 * blocks - diag) * 64 * (8 << m) + sh["workspace_bytes"]
            t["bytes_written"] = sh["workspace_bytes"] + R * R * 8
            t["GBs"] = (t["bytes_read"] + t["bytes_written"]) / t["median_ms"] / 1e6
            t["TFLOPs"] = entry["mfma_flops"] / t["median_ms"] / 1e9
            entry[name] = t
        entry["torch_A_At"] = timed(torch, lambda: torch.matmul(q, q.T, out=G))
        entry["torch_A_Bt"] = timed(torch, lambda: torch.matmul(q, copy.T, out=G))
        # a single call is a few launches long: 50 calls between one pair of events, per call
        for name, fn in (("symmetric_50_calls", lambda: engine.gram_rows(ctx, q, None, m, out=G)),
                         ("torch_A_At_50_calls", lambda: torch.matmul(q, q.T, out=G))):
            t = timed(torch, lambda: [fn() for _ in range(50)])
            entry[name] = {k: v / 50 for k, v in t.items()}
        entry["kernel_over_torch_symmetric"] = entry["symmetric"]["median_ms"] / entry["torch_A_At"]["median_ms"]
        entry["kernel_over_torch_two_operands"] = entry["two_operands"]["median_ms"] / entry["torch_A_Bt"]["median_ms"]
        entry["max_abs_diff_vs_torch"] = float((engine.gram_rows(ctx, q, None, m) - q @ q.T).abs().max())
        res[f"qk_gram_rows_{R}x2^{m}"] = entry

    res["collision_probability"] = timed(torch, lambda: red.collision_probability())
    res["collision"] = red.collision_probability()
    res["ideal_xeb"] = red.ideal_xeb()
    res["renyi2_entropy_bits"] = red.renyi2_entropy()
    half = [c for cl in red.clbits for c in cl[:len(cl) // 2]]
    res["collision_probability_16_clbits"] = timed(torch, lambda: red.collision_probability(half))
    if not args.no_dense:
        torch.cuda.empty_cache()

        def dense_collision():
            full, _ = run_virtual_circuit_dense(virt)
            return float((full * full).sum())

        res["check"] = {"collision_vs_dense_abs_diff": abs(dense_collision() - res["collision"])}
        res["dense_step_only"] = timed(torch, lambda: run_virtual_circuit_dense(virt))
        res["dense_step_sum_of_squares"] = timed(torch, dense_collision)
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def scan_leg(args):
    """Nonlinear functionals (``--out``: e.g. profiles/obs_bench_scan.json) on syc 32 5: (a) qk_knit_scan alone on
    the prebuilt side operands: plain, with the histogram, with the entropy term, and the pair scan of the knit
    against itself, each with its achieved TF/s (2 K 2^32 flops per knit formed); (b) KnitReducer.scan from the
    swept rows, with and without the entropy term, and top_k(16); (c) sweep + scan; (d) the route they replace, in
    the same process: the dense step plus the same statistics by torch over its 2^32 output."""
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, observables as ob
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20}
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    red = KnitReducer(virt)
    ctx = engine.get_context(0)
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    K = res["terms"] = int(red.ops.num_terms)
    sides = red._scan_operands(list(range(red.N)))
    A, B, wa, wb = sides.A, sides.B, sides.where_a, sides.where_b
    res["sides"] = {"bits_a": len(wa), "bits_b": len(wb)}
    flops = 2.0 * K * 2.0 ** (len(wa) + len(wb))
    for name, knits, fn in (("plain", 1, lambda: engine.knit_scan(ctx, A, B)),
                            ("hist", 1, lambda: engine.knit_scan(ctx, A, B, hist=True)),
                            ("entropy", 1, lambda: engine.knit_scan(ctx, A, B, entropy=True)),
                            ("entropy_hist", 1, lambda: engine.knit_scan(ctx, A, B, entropy=True, hist=True)),
                            ("pair_with_itself", 2, lambda: engine.knit_scan(ctx, A, B, A, B))):
        t = timed(torch, fn)
        t["TFLOPs"] = knits * flops / t["median_ms"] / 1e9
        res[f"qk_knit_scan_{name}"] = t
        print(name, t, flush=True)
    res["scan_no_entropy"] = timed(torch, lambda: red.scan(entropy=False))
    print("scan_no_entropy", res["scan_no_entropy"], flush=True)
    res["scan_entropy"] = timed(torch, lambda: red.scan())
    res["pair_scan_with_itself"] = timed(torch, lambda: red.hellinger_fidelity(red))
    # depth 5 is far from Porter-Thomas: millions of outcomes share the binade of the 16th largest value, more
    # than the default capacity of 2^24
    tau, count = ob.histogram_threshold(red.scan(entropy=False).histogram, 16)
    res["top_k_16_collected"] = count
    res["top_k_16"] = timed(torch, lambda: red.top_k(16, capacity=count))
    res["sweep_plus_scan_no_entropy"] = timed(torch, lambda: KnitReducer(virt).scan(entropy=False))
    sc = red.scan()
    res["values"] = {"mass": sc.mass, "l1": sc.l1, "negativity": sc.negativity, "collision": sc.collision,
                     "shannon_entropy_bits": sc.shannon_entropy, "max": sc.max, "argmax": sc.argmax, "min": sc.min,
                     "support": sc.support, "top_16": [float(v) for v in red.top_k(16, capacity=count)[1].tolist()]}
    if not args.no_dense:
        del A, B
        torch.cuda.empty_cache()

        def dense_stats(entropy):
            full, _ = run_virtual_circuit_dense(virt)
            p = full.clamp(min=0.0)
            out = [full.sum(), full.abs().sum(), p.sum(), (full * full).sum(), full.max(), full.argmax(), full.min(),
                   full.argmin(), (full > 0).sum()]
            if entropy:
                out.append(-torch.special.xlogy(p, p).sum())
            return [float(v) for v in out]

        def dense_top():
            full, _ = run_virtual_circuit_dense(virt)  # torch.topk takes at most 2^31 - 1 elements: 64 rows first
            vals, at = torch.topk(full.view(64, -1), 16, dim=1)
            best, pick = torch.topk(vals.reshape(-1), 16)
            return best, (pick // 16) * (full.numel() // 64) + at.reshape(-1)[pick]

        vals = dense_stats(True)
        res["check"] = {"top_16_max_abs_diff": float((dense_top()[0].cpu() - torch.tensor(res["values"]["top_16"])).abs().max()),
                        "mass_abs_diff": abs(vals[0] - sc.mass), "collision_abs_diff": abs(vals[3] - sc.collision),
                        "max_abs_diff": abs(vals[4] - sc.max), "argmax_equal": int(vals[5]) == sc.argmax,
                        "support_diff": int(vals[8]) - sc.support}
        res["dense_step_only"] = timed(torch, lambda: run_virtual_circuit_dense(virt))
        res["dense_step_stats_no_entropy"] = timed(torch, lambda: dense_stats(False))
        res["dense_step_stats_entropy"] = timed(torch, lambda: dense_stats(True))
        res["dense_step_topk_16"] = timed(torch, dense_top)
        res["scan_over_dense_no_entropy"] = (res["sweep_plus_scan_no_entropy"]["median_ms"]
                                             / res["dense_step_stats_no_entropy"]["median_ms"])
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def channels_leg(args):
    """Per-clbit channels (``--out``: e.g. profiles/obs_bench_channels.json): on [64, 2^16] and [256, 2^16], the
    fragment shapes of syc 32 5, (a) qk_kron2_rows with 16 non-identity bits, out of place and in place, with its
    achieved bytes/s (two passes, each reading and writing every element) and flop/s (a product and a fused
    multiply-add per element and bit); (b) qk_wht_rows on the same buffers in the same process; (c) the torch route
    on the same source: a ``[rows * 2^(15 - b), 2, 2^b]`` view and one einsum per bit. A single call is two short
    launches, so (a)-(c) are also timed as 50 calls between one pair of events, the three routes taking turns for
    three rounds; the ratios come from those windows. Then (d) KnitReducer.with_readout_error on syc 32 5 end to end
    and a marginal of 10 clbits of the reducer it returns, beside the same marginal of the base reducer."""
    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, observables as ob
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20}
    ctx = engine.get_context(0)
    m, calls, rounds = 16, 50, 3
    passes = len(ob.wht_pass_bits(m))
    rng = np.random.default_rng(0)
    mats = np.stack([ob.readout_matrix(e0, e1) for e0, e1 in rng.uniform(0.01, 0.05, size=(m, 2))])
    mats_d = [torch.from_numpy(A).cuda() for A in mats]

    def torch_route(src):
        x = src
        for b in range(m):
            x = torch.einsum("yx,axb->ayb", mats_d[b], x.reshape(-1, 2, 1 << b))
        return x.reshape(src.shape)

    for rows in (64, 256):
        src = torch.randn((rows, 1 << m), dtype=torch.float64, device="cuda")
        dst, buf = torch.empty_like(src), src.clone()
        entry = {"rows": rows, "m": m, "passes": passes, "non_identity_bits": m,
                 "bytes_moved": 2 * passes * rows * (1 << m) * 8, "flops": 3 * m * rows * (1 << m)}
        routes = {"qk_kron2_rows": lambda: engine.kron2_rows(ctx, src, mats, m, out=dst),
                  "qk_wht_rows": lambda: engine.wht_rows(ctx, src, m, out=dst),
                  "torch_einsum_per_bit": lambda: torch_route(src)}
        for name, fn in routes.items():
            entry[f"{name}_out_of_place"] = timed(torch, fn)
        entry["qk_kron2_rows_in_place"] = timed(torch, lambda: engine.kron2_rows(ctx, buf, mats, m, out=buf))
        buf.copy_(src)
        entry["qk_wht_rows_in_place"] = timed(torch, lambda: engine.wht_rows(ctx, buf, m, out=buf))
        windows = {name: [] for name in routes}
        for _ in range(rounds):  # the routes take turns
            for name, fn in routes.items():
                t = timed(torch, lambda: [fn() for _ in range(calls)], reps=7, warm=1)
                windows[name].append(t["median_ms"] / calls)
        for name, per_call in windows.items():
            per_call.sort()
            entry[f"{name}_per_call_in_{calls}_call_windows"] = {"median_ms": per_call[len(per_call) // 2],
                                                                "min_ms": per_call[0], "max_ms": per_call[-1]}
        k = entry[f"qk_kron2_rows_per_call_in_{calls}_call_windows"]
        k["GBs"] = entry["bytes_moved"] / k["median_ms"] / 1e6
        k["GFLOPs"] = entry["flops"] / k["median_ms"] / 1e6
        w = entry[f"qk_wht_rows_per_call_in_{calls}_call_windows"]
        w["GBs"] = entry["bytes_moved"] / w["median_ms"] / 1e6
        entry["kron2_over_wht"] = k["median_ms"] / w["median_ms"]
        entry["torch_over_kron2"] = entry[f"torch_einsum_per_bit_per_call_in_{calls}_call_windows"]["median_ms"] / k["median_ms"]
        engine.kron2_rows(ctx, src, mats, m, out=dst)
        entry["max_abs_diff_vs_torch"] = float((dst - torch_route(src)).abs().max())
        res[f"rows_{rows}"] = entry
        print(rows, json.dumps(entry), flush=True)

    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    red = KnitReducer(VirtualCircuit(cut))
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    res["terms"] = int(red.ops.num_terms)
    confusion = np.stack([ob.readout_matrix(e0, e1) for e0, e1 in rng.uniform(0.01, 0.05, size=(red.N, 2))])
    clbits = [0, 3, 5, 9, 14, 16, 20, 23, 27, 31]
    res["with_readout_error"] = timed(torch, lambda: red.with_readout_error(confusion))
    res["with_readout_mitigation"] = timed(torch, lambda: red.with_readout_mitigation(confusion))
    noisy = red.with_readout_error(confusion)
    res["rows_bytes"] = int(sum(q.numel() * 8 for q in noisy.qs))
    res["marginal_10_after_readout_error"] = timed(torch, lambda: noisy.marginal(clbits))
    res["marginal_10_base"] = timed(torch, lambda: red.marginal(clbits))
    undone = noisy.with_readout_mitigation(confusion)
    res["check"] = {"mass_after_readout_error": float(noisy.expectation([0])[0]),
                    "mitigation_of_error_vs_base_marginal_max_abs_diff": float(
                        (undone.marginal(clbits) - red.marginal(clbits)).abs().max())}
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def projection_leg(args):
    """Nearest probability distribution (``--out``: e.g. profiles/obs_bench_projection.json) on syc 32 5: (a) one
    qk_knit_project_scan pass beside one qk_knit_scan pass on the same operands, alternating in rounds so that both
    see the same clocks (per kernel the median of the rounds' medians and their spread), also with the entropy
    launch and as the pair pass against itself; (b) KnitReducer.project end to end under a 2 % symmetric readout
    mitigation on every clbit: passes, theta, kept, negativity, and beside it (unless --no-dense) the dense step plus
    the same iteration in torch on the 2^32 tensor; (c) run_virtual_circuit_npd at the default accuracy beside
    run_virtual_circuit(dense=False); (d) hwe 36 under the same mitigation: passes, time, peak device memory."""
    import time

    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import (VirtualCircuit, cutting, engine,
                                                                          observables as ob, run_virtual_circuit,
                                                                          run_virtual_circuit_npd)
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "rounds": 5, "reps_per_round": 10}
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    base = KnitReducer(virt)
    conf = ob.readout_matrix(0.02, 0.02)
    red = base.with_readout_mitigation(conf)
    ctx = engine.get_context(0)
    K = res["terms"] = int(red.ops.num_terms)
    sides = red._scan_operands(list(range(red.N)))
    A, B, wa, wb = sides.A, sides.B, sides.where_a, sides.where_b
    res["sides"] = {"bits_a": len(wa), "bits_b": len(wb)}
    theta = red.project().theta
    legs = {"qk_knit_scan_plain": lambda: engine.knit_scan(ctx, A, B),
            "qk_knit_project_scan": lambda: engine.knit_project_scan(ctx, A, B, theta=theta),
            "qk_knit_project_scan_entropy": lambda: engine.knit_project_scan(ctx, A, B, theta=theta, entropy=True),
            "qk_knit_scan_pair_with_itself": lambda: engine.knit_scan(ctx, A, B, A, B),
            "qk_knit_project_scan_pair_with_itself": lambda: engine.knit_project_scan(ctx, A, B, A, B, theta=theta,
                                                                                     theta2=theta)}
    rounds = {name: [] for name in legs}
    for _ in range(res["rounds"]):
        for name, fn in legs.items():
            rounds[name].append(timed(torch, fn, reps=res["reps_per_round"])["median_ms"])
    for name, ms in rounds.items():
        ms = sorted(ms)
        res[name] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
        print(name, res[name], flush=True)
    res["project_pass_over_scan_pass"] = res["qk_knit_project_scan"]["median_ms"] / res["qk_knit_scan_plain"]["median_ms"]
    res["pair_project_pass_over_pair_scan_pass"] = (res["qk_knit_project_scan_pair_with_itself"]["median_ms"]
                                                    / res["qk_knit_scan_pair_with_itself"]["median_ms"])
    # (b)
    pr = red.project()
    res["project"] = dict(timed(torch, lambda: red.project(), reps=10), passes=pr.passes, theta=pr.theta, kept=pr.kept,
                          members=pr.members, mass=pr.mass, dropped_mass=pr.dropped_mass,
                          negativity=red.negativity())
    print("project", res["project"], flush=True)
    res["projected_scan_entropy"] = timed(torch, lambda: red.projected_scan(pr), reps=10)
    # (c)
    now = time.perf_counter()
    got, _ = run_virtual_circuit_npd(virt)
    res["run_virtual_circuit_npd"] = {"seconds": time.perf_counter() - now, "entries": len(got)}
    now = time.perf_counter()
    want, _ = run_virtual_circuit(virt, dense=False)
    res["run_virtual_circuit_dict"] = {"seconds": time.perf_counter() - now, "entries": len(want)}
    res["npd_vs_dict"] = {"same_keys_in_order": list(got) == list(want),
                          "max_abs_diff": max((abs(got[k] - want[k]) for k in want if k in got), default=0.0)}
    print({k: res[k] for k in ("run_virtual_circuit_npd", "run_virtual_circuit_dict", "npd_vs_dict")}, flush=True)
    # (d), before the dense comparator takes its 100 GB
    torch.cuda.empty_cache()
    _, cut, _ = cutting.config_cut_circuit("hwe", 36, 1, 2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    wide = KnitReducer(VirtualCircuit(cut)).with_readout_mitigation(conf)
    now = time.perf_counter()
    pw = wide.project()
    res["hwe_36_project"] = {"seconds": time.perf_counter() - now, "passes": pw.passes, "theta": pw.theta, "kept": pw.kept,
                             "members": pw.members, "dropped_mass": pw.dropped_mass,
                             "peak_device_MiB": torch.cuda.max_memory_allocated() / 2 ** 20}
    del wide
    torch.cuda.empty_cache()
    if args.out:  # what is measured so far, should the comparator run out of memory
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    if not args.no_dense and red.N == 32 and len(red._measured()) == 32:
        del A, B
        torch.cuda.empty_cache()
        inv = ob.invert_channels(ob.bit_channels(conf, 32, red._measured()))
        top = torch.from_numpy(np.kron(inv[31], inv[30])).cuda()  # the two bits beyond qk_kron2_rows' 30

        def dense_project():
            full, _ = run_virtual_circuit_dense(virt)
            full = full.view(4, -1)
            engine.kron2_rows(ctx, full, inv[:30], 30, out=full)
            full = (top @ full).view(-1)
            m, th, last = float(full.sum()), 0.0, None
            zero = torch.zeros((), dtype=full.dtype, device=full.device)
            for passes in range(1, 33):
                kept = full > th
                n = int(kept.sum())
                if n == last:
                    break
                th, last = (float(torch.where(kept, full, zero).sum()) - m) / n, n  # a mask index stops at 2^31
            return th, n, passes

        th, n, passes = dense_project()
        res["dense_project"] = dict(timed(torch, dense_project, reps=3, warm=0), theta=th, kept=n, passes=passes,
                                    theta_abs_diff=abs(th - pr.theta), kept_diff=n - pr.kept)
        print("dense_project", res["dense_project"], flush=True)
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def projected_leg(args):
    """The projection as a distribution (``--out``: e.g. profiles/obs_bench_projected.json) on syc 32 5 under the 2 %
    symmetric readout mitigation of projection_leg: (a) qk_knit_project_tiles with 1 and with 8 masks beside one
    qk_knit_project_scan pass on the same operands, alternating in rounds (per kernel the median of the rounds' medians
    and their spread); (b) qk_knit_project_draw for 20000 draws; (c) KnitReducer.projected_sample of 20000 shots and
    projected_expectation of 8 masks end to end from the swept rows (project included), and beside them (unless
    --no-dense) the dense step, the same Newton iteration in torch on the 2^32 tensor, then row-wise cumsum +
    searchsorted (20000 draws) or a signed sum (8 masks)."""
    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, observables as ob
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    shots = 20000
    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "rounds": 5, "reps_per_round": 10,
           "shots": shots}
    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    conf = ob.readout_matrix(0.02, 0.02)
    red = KnitReducer(virt).with_readout_mitigation(conf)
    ctx = engine.get_context(0)
    res["terms"] = K = int(red.ops.num_terms)
    sides = red._scan_operands(list(range(red.N)))
    A, B, wa, wb = sides.A, sides.B, sides.where_a, sides.where_b
    res["sides"] = {"bits_a": len(wa), "bits_b": len(wb)}
    pr = red.project()
    theta = pr.theta
    res["projection"] = {"theta": theta, "kept": pr.kept, "members": pr.members, "passes": pr.passes}
    rng = random.Random(1)
    pairs = [(0, 0)] + [(rng.getrandbits(len(wa)), rng.getrandbits(len(wb))) for _ in range(7)]
    # (a)
    legs = {"qk_knit_project_scan": lambda: engine.knit_project_scan(ctx, A, B, theta=theta),
            "qk_knit_project_tiles_1_mask": lambda: engine.knit_project_tiles(ctx, A, B, theta, 0.0, pairs[:1]),
            "qk_knit_project_tiles_8_masks": lambda: engine.knit_project_tiles(ctx, A, B, theta, 0.0, pairs)}
    rounds = {name: [] for name in legs}
    for _ in range(res["rounds"]):
        for name, fn in legs.items():
            rounds[name].append(timed(torch, fn, reps=res["reps_per_round"])["median_ms"])
    for name, ms in rounds.items():
        ms = sorted(ms)
        res[name] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
        print(name, res[name], flush=True)
    scan_ms = res["qk_knit_project_scan"]
    res["tiles_1_mask_over_project_scan"] = res["qk_knit_project_tiles_1_mask"]["median_ms"] / scan_ms["median_ms"]
    res["tiles_8_masks_over_project_scan"] = res["qk_knit_project_tiles_8_masks"]["median_ms"] / scan_ms["median_ms"]
    res["tiles_1_mask_within_1p1_of_the_scan_spread"] = bool(
        res["qk_knit_project_tiles_1_mask"]["median_ms"] <= 1.1 * scan_ms["max_ms"])
    # (b)
    W = engine.knit_project_tiles(ctx, A, B, theta, 0.0)[0].contiguous()
    u = engine.uniforms(ctx, 0, ob.PROJ_DRAW_LABEL, 0, shots)
    res["qk_knit_project_draw_20000"] = timed(torch, lambda: engine.knit_project_draw(ctx, A, B, theta, 0.0, W, u), reps=10)
    res["qk_knit_project_draw_20000"]["GFLOP"] = shots * 2 * 128 * 128 * K / 1e9
    print("draw", res["qk_knit_project_draw_20000"], flush=True)
    # (c)
    masks = [0] + [rng.getrandbits(red.N) for _ in range(7)]
    res["projected_sample_20000_end_to_end"] = timed(torch, lambda: red.projected_sample(shots, red.project(), 0), reps=10)
    res["projected_expectation_8_end_to_end"] = timed(torch, lambda: red.projected_expectation(masks, red.project()),
                                                      reps=10)
    got_e = red.projected_expectation(masks, pr)
    keys = red.projected_sample(shots, pr, 0)
    res["check"] = {"mass": float(got_e[0]), "projection_mass": pr.mass,
                    "every_shot_in_the_support": bool((red.projected_probabilities(keys, pr) > 0).all())}
    print({k: res[k] for k in ("projected_sample_20000_end_to_end", "projected_expectation_8_end_to_end", "check")},
          flush=True)
    if args.out:  # what is measured so far, should the comparator run out of memory
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    if not args.no_dense and red.N == 32 and len(red._measured()) == 32:
        del A, B, W
        torch.cuda.empty_cache()
        inv = ob.invert_channels(ob.bit_channels(conf, 32, red._measured()))
        top = torch.from_numpy(np.kron(inv[31], inv[30])).cuda()  # the two bits beyond qk_kron2_rows' 30
        lo = torch.arange(1 << 16, device="cuda")

        def dense_projection():
            full, _ = run_virtual_circuit_dense(virt)
            full = full.view(4, -1)
            engine.kron2_rows(ctx, full, inv[:30], 30, out=full)
            full = (top @ full).view(-1)
            m, th, last = float(full.sum()), 0.0, None
            zero = torch.zeros((), dtype=full.dtype, device=full.device)
            for _ in range(32):
                kept = full > th
                n = int(kept.sum())
                if n == last:
                    break
                th, last = (float(torch.where(kept, full, zero).sum()) - m) / n, n
            return torch.where(full > th, full - th, zero).view(1 << 16, 1 << 16)

        def dense_sample():
            p = dense_projection()
            rows = torch.cumsum(p.sum(dim=1), 0)
            target = engine.uniforms(ctx, 0, ob.PROJ_DRAW_LABEL, 0, shots) * rows[-1]
            r = torch.clamp(torch.searchsorted(rows, target, right=True), max=(1 << 16) - 1)
            rest = target - torch.where(r > 0, rows[torch.clamp(r - 1, min=0)], torch.zeros_like(target))
            out = torch.empty(shots, dtype=torch.int64, device="cuda")
            for s in range(0, shots, 2000):  # [2000, 2^16] doubles at a time
                c = torch.cumsum(p[r[s:s + 2000]], dim=1)
                x = torch.searchsorted(c, rest[s:s + 2000, None], right=True).view(-1)
                out[s:s + 2000] = (r[s:s + 2000] << 16) | torch.clamp(x, max=(1 << 16) - 1)
            return out

        def signs(shift):  # [2^16, 8] of +-1: the parity of the masks' 16 bits from `shift` on
            z = torch.tensor([(v >> shift) & 0xFFFF for v in masks], device="cuda")
            par = torch.zeros((1 << 16, len(masks)), dtype=torch.int64, device="cuda")
            for b in range(16):
                par ^= ((lo >> b) & 1).view(-1, 1) * ((z >> b) & 1).view(1, -1)
            return 1.0 - 2.0 * par.double()

        s_lo, s_hi = signs(0), signs(16)

        def dense_expectation():
            return ((dense_projection().T @ s_hi) * s_lo).sum(0).cpu().numpy()  # key = row << 16 | column

        res["dense_projected_expectation_8"] = dict(timed(torch, dense_expectation, reps=3, warm=1),
                                                    max_abs_diff=float(np.abs(dense_expectation() - got_e).max()))
        print("dense expectation", res["dense_projected_expectation_8"], flush=True)
        res["dense_projected_sample_20000"] = timed(torch, dense_sample, reps=3, warm=1)
        print("dense sample", res["dense_projected_sample_20000"], flush=True)
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def parametric_leg(args):
    """Run-time parameters (``--out``: profiles/obs_bench_parametric.json) on the parametric hwea ansatz, 16 qubits
    cut into 2 x 8 (PACKED programs) and 36 qubits cut into 2 x 18 (SPLIT programs), one cx cut each, depth 1, one
    process, HIP events, medians of 20: (a) ``ParametricKnit.bind(v)`` against the constant route to the same
    reducer, ``KnitReducer(VirtualCircuit(cut.bind(v)))`` with a fresh ``v`` per call and an empty jit cache
    directory (programs of these sizes stay on the interpreter there; with per-program kernels forced,
    ``prepare_fragments(jit=True)`` plus the sweeps of a fresh ``v``, 3 repeats: every call compiles); (b) per fragment the bound sweep of one binding (``sweep_fragment_bound``) against the constant-folded
    sweep of the same angles (``sweep_fragment``), interpreter and, for the SPLIT programs, per-program kernels
    (event windows around the two calls: at these sizes they hold the launches' host side too, and the constant
    call uploads its job tables each time; kernel-only times need a kernel trace and are not taken here);
    (c) ``bind_many`` of 64 bindings against 64 ``bind`` calls."""
    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, generators
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.circuit import Parameter
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.parametric import ParametricKnit

    os.environ["QKNIT_JIT_CACHE"] = engine.JIT_CACHE_DIR = tempfile.mkdtemp(prefix="qk_jit_empty_")
    res = {"device": torch.cuda.get_device_name(0), "reps": 20, "cases": {}}
    ctx = engine.get_context(0)
    rng = np.random.default_rng(0)
    for label, n in (("hwe_16_1_p2", 16), ("hwe_36_1_2x18", 36)):
        params = [Parameter(f"t{i}") for i in range(2 * n * 2)]
        qc = cutting.decompose(generators.hwea(n, 1, theta=params))
        mid = n // 2
        spec = cutting.CutSpec([list(range(mid)), list(range(mid, n))], cutting.two_qubit_gate_indices(qc, mid - 1, mid)[:1])
        cut = cutting.cut_circuit(qc, spec)
        P = len(params)
        fresh = lambda: rng.uniform(-np.pi, np.pi, P)  # noqa: E731
        entry = {"qubits": n, "parameters": P}
        for jit in ((None,) if n == 16 else (None, True)):
            tag = "default" if jit is None else "jit"
            pk = ParametricKnit(VirtualCircuit(cut), jit=jit)
            e = {"fragments": [{"n": fs.prog.n, "ops": len(fs.prog.ops), "param_ops": fs.prog.num_params,
                                "jobs": fs.jobs.n_jobs, "compiled": fs.dprog.module is not None} for fs in pk.frags]}
            # (a)
            e["bind"] = timed(torch, lambda: pk.bind(fresh()))
            if jit is None:
                e["constant_route_fresh_values"] = timed(torch, lambda: KnitReducer(VirtualCircuit(cut.bind(fresh()))))
            else:
                def constant_compiled():
                    frags = engine.prepare_fragments(VirtualCircuit(cut.bind(fresh())), 0, basis=True, jit=True)
                    assert all(f.dprog.module is not None for f in frags)
                    return [engine.sweep_fragment(ctx, f) for f in frags]

                e["constant_route_compiled_fresh_values"] = timed(torch, constant_compiled, reps=3, warm=0)
                e["bound_sweeps_fresh_values"] = timed(torch, lambda: pk.sweep(fresh()[None]))
            # (b): the same angles, swept as a binding and as constants
            v = fresh()
            const = engine.prepare_fragments(VirtualCircuit(cut.bind(v)), 0, basis=True, jit=jit)
            bound_ms = const_ms = 0.0
            per = []
            for fs, fc in zip(pk.frags, const):
                mats = fs.prog.bind_matrices(v[None])
                tb = timed(torch, lambda: engine.sweep_fragment_bound(ctx, fs, mats))
                tc = timed(torch, lambda: engine.sweep_fragment(ctx, fc))
                diff = float((engine.sweep_fragment_bound(ctx, fs, mats)[0] - engine.sweep_fragment(ctx, fc)).abs().max())
                per.append({"bound": tb, "constant": tc, "constant_ops": len(fc.prog.ops), "max_abs_diff": diff,
                            "constant_compiled": fc.dprog.module is not None})
                bound_ms += tb["median_ms"]
                const_ms += tc["median_ms"]
            e["sweep_one_binding"] = {"per_fragment": per, "bound_ms": bound_ms, "constant_ms": const_ms,
                                      "bound_over_constant": bound_ms / const_ms}
            # (c)
            V = rng.uniform(-np.pi, np.pi, (64, P))
            e["bind_many_64"] = timed(torch, lambda: pk.bind_many(V))
            e["bind_x64"] = timed(torch, lambda: [pk.bind(r) for r in V])
            e["bind_x64_over_bind_many_64"] = e["bind_x64"]["median_ms"] / e["bind_many_64"]["median_ms"]
            if jit is None:
                e["constant_over_bind"] = e["constant_route_fresh_values"]["median_ms"] / e["bind"]["median_ms"]
            entry[tag] = e
            print(label, tag, json.dumps(e), flush=True)
        res["cases"][label] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def alternated(torch, routes: dict, rounds: int) -> dict:
    """Each route of ``routes`` (name -> callable) once per round, the rounds taking the routes in turn, after one
    untimed pass: per route the median of the rounds and their spread (HIP events around the call, host side
    included: every route ends by reading its result back)."""
    for fn in routes.values():
        fn()
    ms = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            ms[name].append(timed(torch, fn, reps=1, warm=0)["median_ms"])
    out = {}
    for name, t in ms.items():
        t.sort()
        out[name] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "spread_ms": t[-1] - t[0]}
    return out


GRADIENT_BASELINE_MAX_BYTES = 48 << 30  # rows the 2P whole-circuit shifted bindings of the baseline may hold


def gradient_leg(args):
    """Parameter-shift gradients (``--out``: profiles/obs_bench_gradient.json) on the circuits of
    :func:`parametric_leg`, the parametric hwea ansatz of 16 qubits cut into 2 x 8 and of 36 qubits cut into 2 x 18,
    with random Z strings and random weights, M in {1, 64, 1024} and B in {1, 16}. End to end, routes alternated per
    round (5 rounds at 16 qubits, 3 at 36), median and spread: ``value_and_gradient`` by the cotangent route
    (weights) and by the reduce route (per mask, then weighted on the host), and what there was before:
    ``ParametricKnit.expectation`` at the ``2 P`` whole-circuit shifted bindings of every binding (valid here: every
    ansatz parameter is one angle), skipped where those bindings' rows would exceed GRADIENT_BASELINE_MAX_BYTES.
    Then, for the first chunk of the wider fragment at B = 16, ``qk_rows_dot`` alone (20 launches, GB/s of the
    shifted rows and the cotangents read) beside the bound sweep that made the chunk's rows."""
    import numpy as np
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine, generators
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.circuit import Parameter
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.parametric import ParametricKnit

    res = {"device": torch.cuda.get_device_name(0), "cases": {}}
    ctx = engine.get_context(0)
    rng = np.random.default_rng(0)
    prng = random.Random(0)
    for label, n, rounds in (("hwe_16_1_p2", 16, 5), ("hwe_36_1_2x18", 36, 3)):
        params = [Parameter(f"t{i}") for i in range(2 * n * 2)]
        qc = cutting.decompose(generators.hwea(n, 1, theta=params))
        mid = n // 2
        spec = cutting.CutSpec([list(range(mid)), list(range(mid, n))], cutting.two_qubit_gate_indices(qc, mid - 1, mid)[:1])
        pk = ParametricKnit(VirtualCircuit(cutting.cut_circuit(qc, spec)))
        P = pk.num_parameters
        shapes = [tuple(q.shape[1:]) for q in pk.sweep(np.zeros((1, P)))]
        occs = [len(fs.prog.shift_occurrences()) for fs in pk.frags]
        entry = {"qubits": n, "parameters": P, "rounds": rounds, "runs": {},
                 "fragments": [{"n": fs.prog.n, "rows": s[0], "width": s[1], "occurrences": o,
                                "compiled": fs.dprog.module is not None} for fs, s, o in zip(pk.frags, shapes, occs)]}
        row_bytes = sum(s[0] * s[1] * 8 for s in shapes)
        shifts = (np.pi / 2) * np.concatenate([np.eye(P), -np.eye(P)])  # [2P, P]
        for B in (1, 16):
            V = rng.uniform(-np.pi, np.pi, (B, P))
            for M in (1, 64, 1024):
                masks = [prng.getrandbits(n) for _ in range(M)]
                w = rng.uniform(-1, 1, M)

                def cotangent():
                    return pk.value_and_gradient(V, masks, w)[1]

                def reduce_route():
                    return np.einsum("bmp,m->bp", pk.value_and_gradient(V, masks)[1], w)

                def baseline():
                    E = pk.expectation((V[:, None, :] + shifts[None]).reshape(-1, P), masks, w).reshape(B, 2, P)
                    return 0.5 * (E[:, 0] - E[:, 1])

                routes = {"cotangent": cotangent, "reduce": reduce_route}
                if 2 * P * B * row_bytes <= GRADIENT_BASELINE_MAX_BYTES:
                    routes["expectation_at_2P_shifts"] = baseline
                got = {name: fn() for name, fn in routes.items()}
                run = alternated(torch, routes, rounds)
                run["max_abs_diff_to_cotangent"] = {k: float(np.abs(g - got["cotangent"]).max()) for k, g in got.items()}
                run["reduce_over_cotangent"] = run["reduce"]["median_ms"] / run["cotangent"]["median_ms"]
                if "expectation_at_2P_shifts" in run:
                    run["baseline_over_cotangent"] = run["expectation_at_2P_shifts"]["median_ms"] / run["cotangent"]["median_ms"]
                entry["runs"][f"B{B}_M{M}"] = run
                print(label, f"B={B} M={M}", json.dumps(run), flush=True)
        # the kernel beside the sweep, on one chunk's rows
        f = max(range(len(shapes)), key=lambda i: shapes[i][0] * shapes[i][1])
        fs, (rows, width) = pk.frags[f], shapes[f]
        nel = rows * width
        olist = fs.prog.shift_occurrences()
        b0, b1, o0, o1 = pk.shift_chunks(16, len(olist), nel * 8, engine.GRADIENT_ROW_BYTES)[0]
        nb, no = b1 - b0, o1 - o0
        mats = fs.prog.bind_matrices_shifted(V[b0:b1], olist[o0:o1]).reshape(nb * no * 2, fs.prog.num_params, 2, 2)
        Q = engine.sweep_fragment_bound(ctx, fs, mats).view(nb * no * 2, nel)
        D = torch.randn((nb, nel), dtype=torch.float64, device="cuda")
        out = torch.empty(nb * no * 2, dtype=torch.float64, device="cuda")
        t_dot = timed(torch, lambda: engine.rows_dot(ctx, Q, D, 2 * no, out=out))
        t_sweep = timed(torch, lambda: engine.sweep_fragment_bound(ctx, fs, mats), reps=5, warm=1)
        read = (Q.numel() + D.numel()) * 8
        entry["chunk"] = {"fragment": f, "bindings": nb, "occurrences": no, "units": nb * no * 2, "n": nel,
                          "bytes_read": read, "qk_rows_dot": dict(t_dot, read_GBs=read / t_dot["median_ms"] / 1e6),
                          "sweep_fragment_bound": t_sweep,
                          "sweep_over_dot": t_sweep["median_ms"] / t_dot["median_ms"]}
        print(label, "chunk", json.dumps(entry["chunk"]), flush=True)
        del Q, D
        res["cases"][label] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gradient", action="store_true", help="the parameter-shift gradient leg only (see gradient_leg)")
    ap.add_argument("--parametric", action="store_true", help="the run-time parameter leg only (see parametric_leg)")
    ap.add_argument("--projection", action="store_true",
                    help="the nearest-probability-distribution leg only (see projection_leg)")
    ap.add_argument("--projected", action="store_true",
                    help="the projection-as-a-distribution leg only (see projected_leg)")
    ap.add_argument("--channels", action="store_true", help="the per-clbit channels leg only (see channels_leg)")
    ap.add_argument("--scan", action="store_true", help="the streamed-scan leg only (see scan_leg)")
    ap.add_argument("--moments", action="store_true", help="the second-moments leg only (see moments_leg)")
    ap.add_argument("--lookup", action="store_true", help="the probabilities-at-chosen-keys leg only (see lookup_leg)")
    ap.add_argument("--spectrum", action="store_true", help="the Walsh-Hadamard spectrum leg only (see spectrum_leg)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense route (needs 34 GB for the output)")
    ap.add_argument("--shots", action="store_true", help="the shots leg only (see the module docstring)")
    ap.add_argument("--shots-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.shots_child:
        return shots_child()
    if args.parametric:
        return parametric_leg(args)
    if args.gradient:
        return gradient_leg(args)
    if args.shots:
        return shots_leg(args)
    if args.spectrum:
        return spectrum_leg(args)
    if args.lookup:
        return lookup_leg(args)
    if args.moments:
        return moments_leg(args)
    if args.scan:
        return scan_leg(args)
    if args.projection:
        return projection_leg(args)
    if args.projected:
        return projected_leg(args)
    if args.channels:
        return channels_leg(args)
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.observables import KnitReducer
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.run import run_virtual_circuit_dense

    _, cut, _ = cutting.config_cut_circuit("syc", 32, 5, 2)
    virt = VirtualCircuit(cut)
    N = 32
    clbits = list(range(0, 8)) + list(range(16, 24))
    rng = random.Random(0)
    masks = [rng.getrandbits(N) for _ in range(1024)]
    res = {"config": "syc_32_5_p2", "device": torch.cuda.get_device_name(0), "reps": 20}

    red = KnitReducer(virt)
    res["fragments"] = [{"rows": int(q.shape[0]), "m": len(cl)} for q, cl in zip(red.qs, red.clbits)]
    res["terms"] = int(red.ops.num_terms)
    res["sweep_once"] = timed(torch, lambda: KnitReducer(virt), reps=5, warm=1)
    res["marginal_16"] = timed(torch, lambda: red.marginal(clbits))
    res["expectation_64"] = timed(torch, lambda: red.expectation(masks[:64]))
    res["expectation_1024"] = timed(torch, lambda: red.expectation(masks))

    # the reduction kernel alone, on the fragment with the most swept rows
    ctx = engine.get_context(0)
    f = max(range(len(red.qs)), key=lambda i: red.qs[i].numel())
    q, m = red.qs[f], len(red.clbits[f])
    nbytes = q.shape[0] * (1 << m) * 8
    kernel = {}
    for name, keep, flips in (("marginal_keep_low8", 0xFF, [0]), ("marginal_keep_high8", 0xFF << (m - 8), [0]),
                              ("parity_1_mask", 0, [masks[0] & ((1 << m) - 1)]),
                              ("parity_16_masks", 0, [z & ((1 << m) - 1) for z in masks[:16]]),
                              ("parity_1024_masks", 0, [z & ((1 << m) - 1) for z in masks])):
        out = torch.empty((q.shape[0], len(flips) << bin(keep).count("1")), dtype=torch.float64, device="cuda")
        t = timed(torch, lambda: engine.reduce_bits(ctx, q, m, keep, flips, out=out))
        passes = -(-len(flips) // engine.REDUCE_BITS_BATCH)
        t["source_reads"] = passes
        t["read_GBs"] = passes * nbytes / t["median_ms"] / 1e6
        kernel[name] = t
    res["qk_reduce_bits"] = {"rows": int(q.shape[0]), "m": m, "source_bytes": nbytes, **kernel}

    if not args.no_dense:
        lo = torch.arange(1 << 16, device="cuda")

        def signs(zs, shift):  # [2^16, M] of +-1: the parity of the masks' 16 bits from `shift` on
            z = torch.tensor([(v >> shift) & 0xFFFF for v in zs], device="cuda")
            par = torch.zeros((1 << 16, len(zs)), dtype=torch.int64, device="cuda")
            for b in range(16):
                par ^= ((lo >> b) & 1).view(-1, 1) * ((z >> b) & 1).view(1, -1)
            return 1.0 - 2.0 * par.double()

        s64, s1024 = (signs(masks[:64], 0), signs(masks[:64], 16)), (signs(masks, 0), signs(masks, 16))

        def dense_marginal():
            full, _ = run_virtual_circuit_dense(virt)
            return full.view(256, 256, 256, 256).sum(dim=(0, 2)).reshape(-1)

        def dense_expectation(s):
            full, _ = run_virtual_circuit_dense(virt)
            return ((full.view(1 << 16, 1 << 16) @ s[0]) * s[1]).sum(0).cpu().numpy()

        got_m, got_e = dense_marginal(), dense_expectation(s64)
        res["check"] = {"marginal_max_abs_diff": float((got_m - red.marginal(clbits)).abs().max()),
                        "expectation_max_abs_diff": float(abs(got_e - red.expectation(masks[:64])).max())}
        res["dense_step_only"] = timed(torch, lambda: run_virtual_circuit_dense(virt))
        res["dense_marginal_16"] = timed(torch, dense_marginal)
        res["dense_expectation_64"] = timed(torch, lambda: dense_expectation(s64))
        res["dense_expectation_1024"] = timed(torch, lambda: dense_expectation(s1024), reps=5, warm=1)
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
