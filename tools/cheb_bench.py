#!/usr/bin/env python
"""ChebConv's fused recurrence step (dc_cheb.hip) against the hop plus separate elementwise launches, on two graphs -
the soft batch of the headline, the rest meshes of ``synth.make_batch(32)`` (N = 32,768, E = 196,224), and a kNN graph
(k = 16, ``knn_graph``) over the same vertices - at F = 32 and 256: device-event medians of forward and forward +
backward.  No target and no pass / fail threshold: no test asserts a time.

Three comparisons, K = 4 (three steps each way), ``lambda_max`` at its default:

* ONE step on the device alone (``step_us``): 20 steps captured into a hipGraph, so that no host launch cost sits between
  them - the fused launch against ``ops.hop`` with pre-doubled weights plus one elementwise launch, forward
  (``2 L^ x - z``) and backward (``z += 2 L^T x`` through the hop's addend, ``z2 -= x``).  This is the claim to check:
  the fused step is not slower than the hop plus its separate elementwise launch.

* ``ops.cheb_basis`` against the same maths composed from ``ops.propagate`` and torch elementwise ops.  The
  composition is given every advantage the existing hop allows: the Laplacian weights sit pre-scaled in two copies of
  the adjacency (``wl`` for Tx_1, ``2 wl`` for the later steps), the diagonal term is dropped (it is 0 at
  ``lambda_max = 2``; the fused step computes it regardless), a step is one hop launch plus ONE elementwise launch
  (``hop - Tx_{k-2}``), and the blocks are not concatenated into a slab.  Autograd replays it as one hop and one or two
  elementwise launches per step.
* ``ChebConv(F, 256, K=4)`` against ``TAGConv(F, 256, K=3)``: the same number of hops and of weight blocks.  TAGConv
  runs its own slab, hop-chain and dense paths; the figure says what the new layer costs next to the default one, not
  which kernel is faster.

The two eager comparisons run a handful of short launches per call and are bound by the host's launch rate as much as
by the kernels; ``cheb_basis`` also recomputes the Laplacian weights on every forward (two small launches), which the
composition, whose weights are prepared once outside the timed region, does not.

``model_bytes`` is the algorithmic traffic of one step, computed from the shapes, not measured.  Prints one JSON line;
``--out`` (default ``profiles/cheb_bench.json``) also writes it.  Needs a HIP device (no fallback).
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
from deformcontact_amd.graph import GraphIndex  # noqa: E402

WIDTHS = (32, 256)
KNN = 16
K = 4
OUT = 256


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


def captured_us(fn, reps, iters, warmup):
    """device time of one ``fn()`` in microseconds: ``reps`` calls captured into one hipGraph on one stream (no host
    launch cost between them), the median replay divided by ``reps``"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return 1000.0 * median_ms(graph.replay, iters, warmup) / reps


def model_bytes(N, E, f):
    """compulsory bytes of one recurrence step (computed, not measured): per edge one neighbour row, one id and one
    weight; per node two ptr entries and the rows of the epilogue"""
    row, idx = f * 4, 4
    edges = E * (row + 2 * idx) + N * 2 * idx
    return {"fused_step": edges + N * 3 * row,                  # x_i and z_i in, y out
            "fused_step_second_output": edges + N * 5 * row,    # ... and z2_i in, y2 out
            "hop_plus_elementwise": edges + N * row + N * 3 * row}   # hop: out; elementwise: two in, one out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheb_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("cheb_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    N = int(rest.x.size(0))
    graphs = {"soft_mesh": rest.edge_index.to(dev),
              "knn16": dc.nn.knn_graph(rest.pos.to(dev).contiguous(), KNN, rest.batch.to(dev))}

    def both(fwd_fn, leaves, gup):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), leaves, gup)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    result = {"tool": "cheb_bench", "N": N, "K": K, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "graphs": []}
    for name, ei in graphs.items():
        E = int(ei.size(1))
        g = GraphIndex(ei, N, self_loops=False, normalize=False)
        # the composition's adjacencies: the same sorted set with the Laplacian weights in place of gcn_norm's
        wl_fwd, wl_bwd = ops._cheb_norm(g, ops.CHEB_MODES["sym"], 2.0)
        scaled = []
        for s in (1.0, 2.0):
            gs = GraphIndex(ei, N, self_loops=False, normalize=True)
            gs.fwd.w.copy_(wl_fwd * s)
            gs.bwd.w.copy_(wl_bwd * s)
            scaled.append(gs)
        g1, g2 = scaled
        entry = {"graph": name, "E": E, "widths": []}
        for f in WIDTHS:
            x = torch.from_numpy(rng.uniform(-1, 1, (N, f)).astype(np.float32)).to(dev).requires_grad_(True)
            gslab = torch.from_numpy(rng.uniform(0.5, 1.5, (N, K * f)).astype(np.float32)).to(dev)
            gblocks = [gslab[:, i * f:(i + 1) * f] for i in range(K)]
            gout = torch.from_numpy(rng.uniform(0.5, 1.5, (N, OUT)).astype(np.float32)).to(dev)

            def composition():
                tx = [x, ops.propagate(g1, x)]
                for _ in range(2, K):
                    tx.append(ops.propagate(g2, tx[-1]) - tx[-2])
                return tx

            with torch.no_grad():                                # same maths: the two agree to rounding
                a, b = ops.cheb_basis(g, x, K), torch.cat(composition(), 1)
                dist = float((a - b).abs().max() / b.abs().max())
            ms = {"cheb_basis": both(lambda: ops.cheb_basis(g, x, K), [x], gslab),
                  "propagate_composition": both(composition, [x], gblocks)}
            # one step on its own, without the host: buffers allocated once, 20 steps per captured graph
            with torch.no_grad():
                xs, z, y, t, z2 = (torch.from_numpy(rng.uniform(-1, 1, (N, f)).astype(np.float32)).to(dev) for _ in range(5))

                def fused_fwd():
                    ops._cheb_hop(g.fwd, wl_fwd, xs, y, 0.0, 2, -1, z=z)

                def hop_sub_fwd():
                    ops.hop(g2.fwd, xs, out=t)
                    torch.sub(t, z, out=y)

                def fused_bwd():
                    ops._cheb_hop(g.bwd, wl_bwd, xs, z, 0.0, 2, 1, z=z, z2=z2, y2=z2)

                def hop_sub_bwd():
                    ops.hop(g2.bwd, xs, out=z, addend=z)
                    z2.sub_(xs)
                step_us = {label: captured_us(fn, 20, args.iters, args.warmup) for label, fn in (
                    ("fused_forward_step", fused_fwd), ("hop_plus_sub_forward_step", hop_sub_fwd),
                    ("fused_backward_step", fused_bwd), ("hop_plus_sub_backward_step", hop_sub_bwd))}
            torch.manual_seed(0)
            cheb, tag = dc.nn.ChebConv(f, OUT, K).to(dev), dc.nn.TAGConv(f, OUT, K - 1).to(dev)
            layers = {}
            for label, conv in (("ChebConv_K4", cheb), ("TAGConv_K3", tag)):
                leaves = [x] + list(conv.parameters())
                layers[label] = both(lambda: ops.resolve(conv(x, ei)), leaves, gout)
            entry["widths"].append({
                "F": f, "ms": ms, "max_rel_distance_to_composition": dist,
                "fused_over_composition": {p: ms["cheb_basis"][p] / ms["propagate_composition"][p]
                                           for p in ("fwd", "fwd_bwd")},
                "step_us": step_us,
                "fused_step_over_hop_plus_sub": {
                    "forward": step_us["fused_forward_step"] / step_us["hop_plus_sub_forward_step"],
                    "backward": step_us["fused_backward_step"] / step_us["hop_plus_sub_backward_step"]},
                "layer_ms": layers,
                "cheb_over_tag": {p: layers["ChebConv_K4"][p] / layers["TAGConv_K3"][p] for p in ("fwd", "fwd_bwd")},
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
