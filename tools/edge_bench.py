#!/usr/bin/env python
"""EdgeConv's two primitives ``ops.edge_pairs`` + ``ops.edge_aggregate`` (dc_edge.hip) around a fixed elementwise
stand-in for the user's module, on two graphs - the soft batch of the headline, the rest meshes of
``synth.make_batch(32)`` (N = 32,768, E = 196,224), and a kNN cloud (k = 16, ``knn_graph``) over the same vertices - at
F = 3, 21 and 64 (pair rows of 2F columns, reduced at that width): device-event medians of forward and forward +
backward (the gradient of x) for max, mean and sum.  No target and no pass / fail threshold: nothing depends on this
layer's speed yet.

The baseline is the torch composition on the same GPU: ``index_select`` of the destination and of the source rows, a
subtraction, ``cat`` and, behind the same stand-in, ``scatter_reduce_(amax / mean / sum, include_self=False)`` - three
``[E, F..2F]`` temporaries before the module has seen a row where ``edge_pairs`` writes ``z`` once.  Its backward adds
with float atomics (``index_add_``), so its bits change from run to run where the kernels' do not, and its max sends
the whole gradient of a tie to every edge that attains it where the kernels split it evenly: the
two are compared forward only (``max_rel_distance_to_torch``).  The byte model next to it (``model_bytes``) counts
what the four entries must move.  Prints one JSON line; ``--out`` (default ``profiles/edge_bench.json``) also writes
it.  Needs a HIP device (no fallback).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deformcontact_amd as dc  # noqa: E402
from deformcontact_amd import ops, synth  # noqa: E402

WIDTHS = (3, 21, 64)
KNN = 16
REDUCES = {"max": "amax", "mean": "mean", "sum": "sum"}


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
    """compulsory bytes per launch (computed, not measured) with C = 2F reduced columns: rows read and written, the
    adjacency (two ptr entries per row, one edge id per edge), the int64 endpoints of the per-edge entries"""
    row, c, idx = f * 4, 2 * f * 4, 4
    return {"pair_fwd": E * (2 * row + 2 * row + 2 * 8),                          # x[dst], x[src] in, 2F out
            "pair_bwd": E * (2 * row + row + 2 * idx) + N * (row + 4 * idx),      # both halves by dst, one by src; g_x out
            "reduce_fwd": E * (c + idx) + N * (c + 2 * idx),                      # (+ N * c for the max: cnt)
            "reduce_bwd": E * (2 * c + 2 * 8),                                    # g_y[dst] in, g_m out (+ m, y, cnt: max)
            "torch_pairs_materialised": E * (2 * 2 * row + 3 * row + 2 * c + 2 * 8)}   # x_i, x_j written and read, the
                                                                                  # difference written and read, cat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("edge_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    N = int(rest.x.size(0))
    graphs = {"soft_mesh": rest.edge_index.to(dev),
              "knn16": dc.nn.knn_graph(rest.pos.to(dev).contiguous(), KNN, rest.batch.to(dev))}

    def both(fwd_fn, leaf, gup):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), [leaf], gup)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    result = {"tool": "edge_bench", "N": N, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "graphs": []}
    for name, ei in graphs.items():
        E = int(ei.size(1))
        g = dc.nn.EdgeConv(torch.nn.Identity()).graph(ei, N)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        entry = {"graph": name, "E": E, "widths": []}
        for f in WIDTHS:
            x = torch.from_numpy(rng.uniform(-1, 1, (N, f)).astype(np.float32)).to(dev).requires_grad_(True)
            scale = torch.from_numpy(rng.uniform(0.5, 1.5, (2 * f,)).astype(np.float32)).to(dev)
            gup = torch.from_numpy(rng.uniform(0.5, 1.5, (N, 2 * f)).astype(np.float32)).to(dev)
            per_reduce = {}
            for reduce, torch_reduce in REDUCES.items():
                def kernels():
                    return ops.edge_aggregate(g, ops.edge_pairs(g, x) * scale, reduce)

                def torch_composition():
                    xi = x.index_select(0, dst)
                    m = torch.cat([xi, x.index_select(0, src) - xi], dim=1) * scale
                    return torch.zeros((N, 2 * f), device=dev).scatter_reduce_(
                        0, dst.unsqueeze(1).expand(-1, 2 * f), m, torch_reduce, include_self=False)

                with torch.no_grad():                            # same maths forward: they agree to summation order
                    a, b = kernels(), torch_composition()
                    dist = float((a - b).abs().max() / b.abs().max())
                ms = {"kernels": both(kernels, x, gup), "torch_composition": both(torch_composition, x, gup)}
                per_reduce[reduce] = {
                    "ms": ms, "max_rel_distance_to_torch": dist,
                    "kernels_over_torch": {p: ms["kernels"][p] / ms["torch_composition"][p] for p in ("fwd", "fwd_bwd")}}
            entry["widths"].append({"F": f, "C": 2 * f, "reduce": per_reduce, "model_bytes": model_bytes(N, E, f)})
        result["graphs"].append(entry)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
