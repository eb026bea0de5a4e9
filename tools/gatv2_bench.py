#!/usr/bin/env python
"""GATv2Conv against GATConv of the same (in, H, C) on the soft batch of the headline - the rest meshes of
``synth.make_batch(32)``, the batch ``bench.py`` and ``tools/kbench.py`` use (N = 32,768, E = 196,224), features of width
in = 256: device-event medians of forward and forward + backward for (H, C) = (4, 64), (8, 32), (2, 128), (1, 256), with
``share_weights`` both ways.  No target: GATv2 gathers H*C floats per edge for its scores where GAT reads H, and runs a
second dense block (``lin_r``) unless the weights are shared - the ratio on one machine is the figure.  The byte model
next to it counts what the kernels behind the linears must move (``model_bytes``): rows gathered and written, per-edge
vectors, adjacency.  Prints one JSON line; ``--out`` also writes it.  Needs a HIP device (no fallback).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deformcontact_amd as dc  # noqa: E402
from deformcontact_amd import synth  # noqa: E402

FIN = 256


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def model_bytes(N, E, nh, c):
    """compulsory bytes behind the linears: (GATv2 forward, GATv2 backward, GAT forward)"""
    ep, f = E + N, nh * c
    row, vec, adj = f * 4, nh * 4, 4
    agg = ep * (row + vec + adj) + N * row                       # gather xl rows, alpha, other; write the output rows
    v2_fwd = ep * (row + adj) + N * row + 3 * ep * vec + agg      # score: gather xl, read xr; alpha written, read, written
    gat_fwd = N * row + 2 * N * vec + ep * (2 * vec + adj) + agg  # dot products over h; softmax on [N, H] operands
    sddmm = ep * (row + adj + vec) + N * row
    dst = ep * (row + adj + vec) + 2 * N * row + 3 * ep * vec     # ge formed (alpha, galpha read), xl gathered, g_xr written
    src = ep * (2 * row + 2 * adj + 2 * vec) + 2 * N * row        # gm and xr gathered, alpha / ge through to_fwd
    return v2_fwd, sddmm + dst + src, gat_fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("gatv2_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    ei = rest.edge_index.to(dev)
    N, E = int(rest.x.size(0)), int(ei.size(1))
    x = torch.from_numpy(rng.uniform(-1, 1, (N, FIN)).astype(np.float32)).to(dev).requires_grad_(True)

    def timed(layer, gup):
        def fwd():
            with torch.no_grad():
                layer(x, ei, relu=True)

        def fwd_bwd():
            torch.autograd.grad(layer(x, ei, relu=True), [x] + list(layer.parameters()), gup)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    result = {"tool": "gatv2_bench", "N": N, "E": E, "in": FIN, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "shapes": []}
    for nh, c in ((4, 64), (8, 32), (2, 128), (1, 256)):
        torch.manual_seed(0)
        gup = torch.from_numpy(rng.uniform(0.5, 1.5, (N, nh * c)).astype(np.float32)).to(dev)
        gat = timed(dc.nn.GATConv(FIN, c, heads=nh).to(dev), gup)
        v2 = timed(dc.nn.GATv2Conv(FIN, c, heads=nh).to(dev), gup)
        v2s = timed(dc.nn.GATv2Conv(FIN, c, heads=nh, share_weights=True).to(dev), gup)
        mf, mb, gf = model_bytes(N, E, nh, c)
        result["shapes"].append({
            "H": nh, "C": c, "gat_ms": gat, "gatv2_ms": v2, "gatv2_shared_ms": v2s,
            "gatv2_over_gat": {k: v2[k] / gat[k] for k in gat},
            "gatv2_shared_over_gat": {k: v2s[k] / gat[k] for k in gat},
            "model_bytes": {"gatv2_fwd": mf, "gatv2_bwd": mb, "gat_fwd": gf, "fwd_ratio": mf / gf}})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
