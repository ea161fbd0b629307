#!/usr/bin/env python3
"""Write speed of the bench's knit into successive qk_out_alloc mappings: fresh ones held together,
then after frees (retired ranges, released physical chunks), to see which allocations write fast.

    python tools/out_mapping_probe.py [--steps 4]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--plan", default="a b c -a -b d e -c -d -e f g")
    args = ap.parse_args()
    import torch

    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd import VirtualCircuit, cutting, engine
    from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.pipeline import KnitPipeline

    name, n, d, p, var = cutting.BASELINE_CONFIGS["syc_32_5_p2"]
    cut = cutting.config_cut_circuit(name, n, d, p, var)[1]
    pipe = KnitPipeline(VirtualCircuit(cut), factored=True)
    qs = pipe.sweep()
    p_ = pipe._prep_dev_rank(qs)
    torch.cuda.synchronize()
    A2, B2, k = p_.A2, p_.B2, p_.k_eff
    cA, cB = pipe.ops.clbits[pipe.order[0]], pipe.ops.clbits[pipe.order[-1]]
    N = pipe.N
    del pipe
    torch.cuda.empty_cache()
    ctx = engine.get_context(0)
    held = {}
    for op in args.plan.split():
        if op.startswith("-"):
            del held[op[1:]]
            continue
        out, owner = engine.out_buffer(ctx, 1 << N)
        held[op] = (out, owner)
        ts = []
        for _ in range(args.steps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            engine.knit_outer_stream(ctx, A2, B2, cA, cB, N, out, k_dev=k)
            b.record()
            ts.append((a, b))
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ts[1:]]
        print(json.dumps({"buffer": op, "ptr": hex(out.data_ptr()), "write_ms": round(sum(ms) / len(ms), 3),
                          "held": sorted(held)}), flush=True)


if __name__ == "__main__":
    main()
