#!/usr/bin/env python
"""GINEConv's aggregation ``ops.gine_aggregate`` (``(1 + eps) x_i + sum relu(x_j + e_ji)``, dc_gine.hip) on two graphs
- the soft batch of the headline, the rest meshes of ``synth.make_batch(32)`` (N = 32,768, E = 196,224), and a kNN
graph (k = 16, ``knn_graph``) over the same vertices - at F = 21, 64 and 256: device-event medians of forward and
forward + backward (gradients of x and of e).  No target and no pass / fail threshold: nothing depends on this
layer's speed yet.

The baseline is the torch composition on the same GPU: ``index_select`` of the source rows + add + ``relu`` +
``index_add_`` into ``(1 + eps) x``, which materialises ``[E, F]`` twice forward (the gathered rows, the messages) and
again in backward; ``index_add_`` adds with float atomics, so its bits change from run to run where the kernel's do
not.  The byte model next to it (``model_bytes``) counts what the three entries must move.  Prints one JSON line;
``--out`` (default ``profiles/gine_bench.json``) also writes it.  Needs a HIP device (no fallback).
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

WIDTHS = (21, 64, 256)
KNN = 16


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
    """compulsory bytes per launch (computed, not measured): rows read and written, the adjacency (two ptr entries per
    row; per edge one neighbour id and one edge id), the int64 endpoints of dc_gine_bwd_e, eps"""
    row, idx = f * 4, 4
    return {"fwd": E * (2 * row + 2 * idx) + N * (2 * row + 2 * idx) + 4,        # x_j and e per edge; x_i in, y out
            "bwd_x": E * (2 * row + 2 * idx) + N * (3 * row + 2 * idx) + 4,      # g_y[i] and e per edge; x_j, g_y[j] in, g_x out
            "bwd_e": E * (4 * row + 2 * 8),                                      # x[src], e, g_y[dst] in, g_e out
            "torch_fwd_materialised": E * (5 * row + 2 * 8) + N * 3 * row}      # x[src] written; read with e, msg written; msg read


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gine_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("gine_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    N = int(rest.x.size(0))
    graphs = {"soft_mesh": rest.edge_index.to(dev),
              "knn16": dc.nn.knn_graph(rest.pos.to(dev).contiguous(), KNN, rest.batch.to(dev))}
    eps = torch.full((1,), 0.3, device=dev)

    def both(fwd_fn, leaves, gup):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), leaves, gup)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    result = {"tool": "gine_bench", "N": N, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "graphs": []}
    for name, ei in graphs.items():
        E = int(ei.size(1))
        g = dc.nn.GINEConv(torch.nn.Identity()).graph(ei, N)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        entry = {"graph": name, "E": E, "widths": []}
        for f in WIDTHS:
            x = torch.from_numpy(rng.uniform(-1, 1, (N, f)).astype(np.float32)).to(dev).requires_grad_(True)
            e = torch.from_numpy(rng.uniform(-1, 1, (E, f)).astype(np.float32)).to(dev).requires_grad_(True)
            gup = torch.from_numpy(rng.uniform(0.5, 1.5, (N, f)).astype(np.float32)).to(dev)

            def torch_composition():
                return ((1 + eps) * x).index_add_(0, dst, torch.relu(x.index_select(0, src) + e))

            with torch.no_grad():                                # same maths: the two agree to summation order
                a, b = ops.gine_aggregate(g, x, e, eps), torch_composition()
                dist = float((a - b).abs().max() / b.abs().max())
            ms = {"gine_aggregate": both(lambda: ops.gine_aggregate(g, x, e, eps), [x, e], gup),
                  "torch_composition": both(torch_composition, [x, e], gup)}
            entry["widths"].append({
                "F": f, "ms": ms, "max_rel_distance_to_torch": dist,
                "kernel_over_torch": {p: ms["gine_aggregate"][p] / ms["torch_composition"][p] for p in ("fwd", "fwd_bwd")},
                "model_bytes": model_bytes(N, E, f)})
        result["graphs"].append(entry)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
