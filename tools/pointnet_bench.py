#!/usr/bin/env python
"""PointNetConv's two autograd nodes ``ops.pointnet_pairs`` + ``ops.pointnet_aggregate`` and the three global pools
(dc_pointnet.hip, the forward reduction of dc_edge.hip) on a set-abstraction shape built from the soft batch of the
headline - the rest meshes of ``synth.make_batch(32)``, 32 x 1,024 points: ``fps`` at ratio 0.5 picks the 16,384
destinations, ``radius`` with at most 64 neighbours (r = 4 mean mesh-edge lengths) the bipartite edges - at F = 3 and
64 source features (message rows of F + 3 columns), reduced at C = 64.  Device-event medians of forward and forward +
backward (gradients of x and of both positions; of x for the pools).  No target and no pass / fail threshold.

The baselines are the torch compositions on the same GPU: ``index_select`` of the source rows and of both positions, a
subtraction and ``cat`` for the pair rows; ``scatter_reduce_(amax / mean / sum, include_self=False)`` by destination
for the reduction and by ``batch`` for the pools.  Their backward adds with float atomics, and their max sends the
whole gradient of a tie to every row that attains it: the two are compared forward only.

``z_layout`` answers whether ``z`` should be contiguous ``[E', F + 3]`` or have its row stride padded to a multiple of
4 floats (16-byte stores in the pair kernel where F % 4 == 0; ``local_nn``'s first GEMM then reads a strided operand):
the pair node alone and the whole layer with ``local_nn = Linear(F + 3, 64)`` under both layouts.  Prints one JSON
line; ``--out`` (default ``profiles/r10/pointnet_bench.json``) also writes it.  Needs a HIP device (no fallback).
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
from deformcontact_amd import ops, pointops, synth  # noqa: E402

WIDTHS = (3, 64)
C = 64
REDUCES = {"max": "amax", "mean": "mean", "sum": "sum"}
POOLS = {"add": ("sum", pointops.global_add_pool), "mean": ("mean", pointops.global_mean_pool),
         "max": ("amax", pointops.global_max_pool)}


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


def model_bytes(ns, nd, E, f, c):
    """compulsory bytes per launch (computed, not measured): rows read and written, the adjacency (two ptr entries per
    row, an edge id and an endpoint per edge), the int64 endpoints of the per-edge entries"""
    row, pos, idx = f * 4, 12, 4
    return {"pair_fwd": E * (row + 2 * pos + 2 * 8 + row + pos),                    # x[src], both positions in; F + 3 out
            "pair_bwd": E * (row + pos + 2 * idx) + E * (pos + 2 * idx) + ns * (row + pos + 2 * idx) + nd * (pos + 2 * idx),
            "reduce_fwd": E * (c * 4 + idx) + nd * (c * 4 + 2 * idx),               # (+ nd * c * 4 for the max: cnt)
            "reduce_bwd": E * (2 * c * 4 + 2 * 8),                                  # g_y[dst] in, g_m out (+ m, y, cnt: max)
            "torch_pairs_materialised": E * (2 * row + 4 * pos + 2 * pos + 2 * (row + pos) + 2 * 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "pointnet_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("pointnet_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    pos = rest.pos.to(dev).contiguous()
    batch = rest.batch.to(dev)
    nb = int(batch[-1]) + 1
    mesh = rest.edge_index.to(dev)
    r = 4.0 * float((pos[mesh[0]] - pos[mesh[1]]).norm(dim=1).mean())
    idx = dc.nn.fps(pos, batch, ratio=0.5, random_start=False)
    pos_d = pos[idx].contiguous()
    row, col = dc.nn.radius(pos, pos_d, r, batch, batch[idx], max_num_neighbors=64)
    ei = torch.stack([col, row], dim=0).contiguous()
    ns, nd, E = int(pos.size(0)), int(pos_d.size(0)), int(ei.size(1))
    g = ops.pointnet_graph(ei, ns, nd)
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    deg = torch.bincount(dst, minlength=nd)

    def t(shape, lo=-1.0, hi=1.0):
        return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32)).to(dev)

    def both(fwd_fn, leaves, gup):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), leaves, gup)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    def ratio(ms):
        return {p: ms["kernels"][p] / ms["torch_composition"][p] for p in ("fwd", "fwd_bwd")}

    result = {"tool": "pointnet_bench", "Ns": ns, "Nd": nd, "E": E, "radius": r, "graphs": nb,
              "in_degree": {"mean": float(deg.float().mean()), "max": int(deg.max())}, "C": C, "iters": args.iters,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "widths": []}
    ps, pd = pos.clone().requires_grad_(True), pos_d.clone().requires_grad_(True)
    for f in WIDTHS:
        x = t((ns, f)).requires_grad_(True)
        leaves = [x, ps, pd]
        gz = t((E, f + 3), 0.5, 1.5)

        def torch_pairs():
            return torch.cat([x.index_select(0, src), ps.index_select(0, src) - pd.index_select(0, dst)], dim=1)

        with torch.no_grad():
            assert torch.equal(ops.pointnet_pairs(g, x, ps, pd), torch_pairs())
        pairs = {"kernels": both(lambda: ops.pointnet_pairs(g, x, ps, pd, pad=False), leaves, gz),
                 "kernels_padded_z": both(lambda: ops.pointnet_pairs(g, x, ps, pd, pad=True), leaves, gz),
                 "torch_composition": both(torch_pairs, leaves, gz)}
        # the whole layer around local_nn = Linear(F + 3, C), max: both layouts of z against the torch composition
        lin = torch.nn.Linear(f + 3, C).to(dev)
        gup = t((nd, C), 0.5, 1.5)
        params = leaves + list(lin.parameters())

        def layer(pad):
            return ops.pointnet_aggregate(g, lin(ops.pointnet_pairs(g, x, ps, pd, pad=pad)), "max", nd)

        def torch_layer():
            return torch.zeros((nd, C), device=dev).scatter_reduce_(
                0, dst.unsqueeze(1).expand(-1, C), lin(torch_pairs()), "amax", include_self=False)

        layers = {"kernels": both(lambda: layer(False), params, gup), "kernels_padded_z": both(lambda: layer(True), params, gup),
                  "torch_composition": both(torch_layer, params, gup)}
        result["widths"].append({"F": f, "pairs_ms": pairs, "pairs_kernels_over_torch": ratio(pairs),
                                 "layer_linear_max_ms": layers, "layer_kernels_over_torch": ratio(layers),
                                 "model_bytes": model_bytes(ns, nd, E, f, C)})
    # the reduction alone, C columns on the edges
    m = t((E, C)).requires_grad_(True)
    gup = t((nd, C), 0.5, 1.5)
    result["aggregate"] = {}
    for reduce, torch_reduce in REDUCES.items():
        def kernels():
            return ops.pointnet_aggregate(g, m, reduce, nd)

        def torch_composition():
            return torch.zeros((nd, C), device=dev).scatter_reduce_(0, dst.unsqueeze(1).expand(-1, C), m, torch_reduce,
                                                                    include_self=False)

        with torch.no_grad():
            a, b = kernels(), torch_composition()
            dist = float((a - b).abs().max() / b.abs().max())
        ms = {"kernels": both(kernels, [m], gup), "torch_composition": both(torch_composition, [m], gup)}
        result["aggregate"][reduce] = {"ms": ms, "max_rel_distance_to_torch": dist, "kernels_over_torch": ratio(ms)}
    # the pools: [Ns, C] rows of 32 graphs of 1,024
    h = t((ns, C)).requires_grad_(True)
    gup = t((nb, C), 0.5, 1.5)
    result["pools"] = {}
    for name, (torch_reduce, fn) in POOLS.items():
        def kernels():
            return fn(h, batch, nb)

        def torch_composition():
            return torch.zeros((nb, C), device=dev).scatter_reduce_(0, batch.unsqueeze(1).expand(-1, C), h, torch_reduce,
                                                                    include_self=False)

        with torch.no_grad():
            a, b = kernels(), torch_composition()
            dist = float((a - b).abs().max() / b.abs().max())
        ms = {"kernels": both(kernels, [h], gup), "torch_composition": both(torch_composition, [h], gup)}
        result["pools"][name] = {"ms": ms, "max_rel_distance_to_torch": dist, "kernels_over_torch": ratio(ms)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
