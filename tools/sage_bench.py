#!/usr/bin/env python
"""SAGEConv's aggregations on the soft batch of the headline - the rest meshes of ``synth.make_batch(32)``, the batch
``bench.py`` and ``tools/transformer_bench.py`` use (N = 32,768, E = 196,224): device-event medians of forward and
forward + backward at F = 21 and F = 256.  No target and no pass / fail threshold: nothing depends on this layer's
speed yet.

Three comparisons per width.  ``mean``: ``ops.aggregate(g, x, "mean")`` (one launch each way) against
``ops.propagate(g, x, weighted=False)`` followed by a torch division by the in-degree (the degree vector built once,
outside the timed region).  ``max``: ``ops.aggregate(g, x, "max")`` against ``torch.scatter_reduce_(amax)`` on the
gathered rows ``x[src]`` [E, F]; the unweighted hop is timed beside them (the max forward is expected within the hop's
time plus the store of the counts).  ``layer``: ``SAGEConv(F, 256)`` with each aggregation against ``GCNConv(F, 256)``.
The byte model next to it (``model_bytes``) counts what the kernels must move.  Prints one JSON line; ``--out`` also
writes it.  Needs a HIP device (no fallback).
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
from deformcontact_amd import ops, synth  # noqa: E402

FOUT = 256


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


def model_bytes(N, E, f):
    """compulsory bytes per launch: rows gathered and written, adjacency (ptr per row, one id per edge)"""
    row, adj = f * 4, 4
    hop = E * (row + adj) + N * (row + 2 * adj)
    return {"hop": hop, "mean_fwd": hop, "mean_bwd": hop + E * 2 * adj,          # + the destination's two ptr entries
            "max_fwd": hop + N * row,                                             # + the counts
            "max_bwd": E * (3 * row + adj) + N * (2 * row + 2 * adj),             # m, cnt, g_m gathered; x read, g_x written
            "max_materialised_fwd": E * (row + adj) + 2 * E * row + N * row}      # x[src] written and read again [E, F]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("sage_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    ei = rest.edge_index.to(dev)
    N, E = int(rest.x.size(0)), int(ei.size(1))
    g = dc.nn.SAGEConv(4, 4).graph(ei, N)
    deg = torch.bincount(ei[1], minlength=N).clamp(min=1).to(torch.float32).unsqueeze(-1)

    def both(fwd_fn, leaves, gup):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), leaves, gup, allow_unused=True)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    result = {"tool": "sage_bench", "N": N, "E": E, "out": FOUT, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "widths": []}
    for f in (21, 256):
        torch.manual_seed(0)
        x = torch.from_numpy(rng.uniform(-1, 1, (N, f)).astype(np.float32)).to(dev).requires_grad_(True)
        gup = torch.from_numpy(rng.uniform(0.5, 1.5, (N, f)).astype(np.float32)).to(dev)
        gout = torch.from_numpy(rng.uniform(0.5, 1.5, (N, FOUT)).astype(np.float32)).to(dev)
        idx = ei[1].unsqueeze(-1).expand(E, f)

        def torch_amax():
            return torch.zeros((N, f), device=dev).scatter_reduce_(0, idx, x[ei[0]], "amax", include_self=False)

        agg = {"hop": both(lambda: ops.propagate(g, x, weighted=False), [x], gup),
               "mean": both(lambda: ops.aggregate(g, x, "mean"), [x], gup),
               "hop_then_divide": both(lambda: ops.propagate(g, x, weighted=False) / deg, [x], gup),
               "max": both(lambda: ops.aggregate(g, x, "max"), [x], gup),
               "torch_scatter_amax": both(torch_amax, [x], gup)}
        # the max forward WITH the counts (a gradient wanted) alone: the figure the expectation speaks of
        agg["max"]["fwd_with_counts"] = median_ms(lambda: ops._sage_max_fwd(g, x.detach(), True), args.iters, args.warmup)

        def layer(mod):
            return both(lambda: mod(x, ei, relu=True), [x] + list(mod.parameters()), gout)
        layers = {"gcn": layer(dc.nn.GCNConv(f, FOUT).to(dev))}
        for aggr in ("mean", "max", "sum"):
            layers["sage_" + aggr] = layer(dc.nn.SAGEConv(f, FOUT, aggr=aggr).to(dev))
        result["widths"].append({
            "F": f, "aggregate_ms": agg, "layer_ms": layers,
            "mean_over_hop_then_divide": {p: agg["mean"][p] / agg["hop_then_divide"][p] for p in ("fwd", "fwd_bwd")},
            "max_over_torch_scatter_amax": {p: agg["max"][p] / agg["torch_scatter_amax"][p] for p in ("fwd", "fwd_bwd")},
            "max_fwd_with_counts_over_hop": agg["max"]["fwd_with_counts"] / agg["hop"]["fwd"],
            "layer_sage_mean_over_gcn": {p: layers["sage_mean"][p] / layers["gcn"][p] for p in ("fwd", "fwd_bwd")},
            "model_bytes": model_bytes(N, E, f)})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
