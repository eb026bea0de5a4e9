#!/usr/bin/env python
"""Multi-head GATConv on the soft batch of the headline (N = 32,768, E = 196,224, in = 256): device-event medians of

  (a) the fused multi-head layer (``GATConv(256, C, heads=H)``),
  (b) what the single-head kernels can do for the same layer: H ``heads=1`` layers over the weight slices + ``cat``,
  (c) the existing ``heads=1, C=256`` layer - same total width, same gathered bytes,

forward and forward + backward, for (H, C) = (4, 64), (8, 32), (2, 128).  ``--edge-dim D`` adds a leg per shape: the
same (H, C) layer with ``edge_dim=D`` fed ``edge_attr`` [E, D] (gradient of ``edge_attr`` included) against the layer
without edge features, with the byte model of the edge-term forward next to it (it reads E*D*4 B of attributes once
and writes (E+N)*H*4 B; the softmax then reads those once more).  Prints one JSON line; ``--out`` also writes it.
Needs a HIP device (no fallback).  Bytes model of (a)/(c) for the aggregation: both gather E' rows of 1 KiB and write N
rows; (a) reads H weights per edge where (c) reads one - ``model_bytes_ratio`` below.
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

N, E, FIN = 32768, 196224, 256


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--edge-dim", type=int, default=0, help="also time the layers with edge features of this width")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("gat_heads_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    # a block-diagonal batch of 32 graphs of 1,024 nodes, as the headline's soft batch
    per, b = N // 32, 32
    src = rng.integers(0, per, E) + np.repeat(np.arange(b), E // b) * per
    dst = rng.integers(0, per, E) + np.repeat(np.arange(b), E // b) * per
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64)).to(dev)
    x = torch.from_numpy(rng.uniform(-1, 1, (N, FIN)).astype(np.float32)).to(dev).requires_grad_(True)
    gup = torch.from_numpy(rng.uniform(0.5, 1.5, (N, 256)).astype(np.float32)).to(dev)
    ep = E + N                                                    # edges with the self loops

    ea = None
    if args.edge_dim > 0:
        ea = torch.from_numpy(rng.uniform(-1, 1, (E, args.edge_dim)).astype(np.float32)).to(dev).requires_grad_(True)

    def timed(layer_fn, params):
        def fwd():
            with torch.no_grad():
                layer_fn()

        def fwd_bwd():
            out = layer_fn()
            torch.autograd.grad(out, [x] + params, gup)
        return median_ms(fwd, args.iters, args.warmup), median_ms(fwd_bwd, args.iters, args.warmup)

    torch.manual_seed(0)
    one = dc.nn.GATConv(FIN, 256).to(dev)
    c_f, c_fb = timed(lambda: one(x, ei, relu=True), list(one.parameters()))
    result = {"tool": "gat_heads_bench", "N": N, "E": E, "in": FIN, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "c_heads1_c256_ms": {"fwd": c_f, "fwd_bwd": c_fb}, "shapes": []}
    for nh, c in ((4, 64), (8, 32), (2, 128)):
        multi = dc.nn.GATConv(FIN, c, heads=nh).to(dev)
        singles = [dc.nn.GATConv(FIN, c).to(dev) for _ in range(nh)]
        # aggregation traffic: gathered rows + written rows + adjacency (other, ptr) + weights per edge
        rows = (ep + N) * 256 * 4 + ep * 4 + N * 4
        a_f, a_fb = timed(lambda: multi(x, ei, relu=True), list(multi.parameters()))
        b_f, b_fb = timed(lambda: torch.cat([s(x, ei, relu=True) for s in singles], 1),
                          [p for s in singles for p in s.parameters()])
        edge = {}
        if ea is not None:
            with_e = dc.nn.GATConv(FIN, c, heads=nh, edge_dim=args.edge_dim).to(dev)
            e_f, e_fb = timed(lambda: with_e(x, ei, ea, relu=True), list(with_e.parameters()) + [ea])
            # forward traffic of the layer behind lin without edge features (aggregation + softmax: the logits' operands,
            # alpha written and read) and what the edge term adds (attributes read once, a_edge written, read by the softmax)
            base = rows + ep * nh * 4 + 2 * ep * nh * 4 + 2 * N * nh * 4
            extra = E * args.edge_dim * 4 + 2 * ep * nh * 4 + ep * 4
            edge = {"edge_dim": args.edge_dim, "e_edge_features_ms": {"fwd": e_f, "fwd_bwd": e_fb},
                    "e_over_a": {"fwd": e_f / a_f, "fwd_bwd": e_fb / a_fb},
                    "model_bytes_ratio_fwd_e_over_a": (base + extra) / base}
        result["shapes"].append({
            "H": nh, "C": c, **edge,
            "a_fused_heads_ms": {"fwd": a_f, "fwd_bwd": a_fb},
            "b_single_head_slices_ms": {"fwd": b_f, "fwd_bwd": b_fb},
            "a_over_b": {"fwd": a_f / b_f, "fwd_bwd": a_fb / b_fb},
            "a_over_c": {"fwd": a_f / c_f, "fwd_bwd": a_fb / c_fb},
            "model_bytes_ratio_aggregation_a_over_c": (rows + ep * nh * 4) / (rows + ep * 4)})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
