#!/usr/bin/env python3
"""Marginals and Z-string expectation values of syc 32 5 without the 2^32 output, against the dense
route (run_virtual_circuit_dense + a torch reduction of the 2^32 output), same process, same box.

HIP events, 3 warm-up rounds, 20 timed repeats each (median and min-max): KnitReducer.marginal onto
16 clbits (0..7 and 16..23), KnitReducer.expectation of 64 and of 1024 masks, the dense route for each
of them, and qk_reduce_bits alone on the larger fragment's swept rows with its achieved read rate
(rows * 2^m * 8 bytes over its time; the rows are cache resident). ``--out FILE`` writes the JSON."""
import argparse
import json
import os
import random
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense route (needs 34 GB for the output)")
    args = ap.parse_args()
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
