#!/usr/bin/env python
"""GMMConv's aggregation ``ops.gmm_aggregate`` (``mean_j sum_k w_k(e_ji) h[j, k*M:(k+1)*M]``, dc_gmm.hip) on two graphs
- the soft batch of the headline, the rest meshes of ``synth.make_batch(32)`` (N = 32,768, E = 196,224), and a kNN
graph (k = 16, ``knn_graph``) over the same vertices - at (K, D, M) = (3, 3, 64), (10, 3, 64), (25, 2, 16) and
(3, 3, 256): device-event medians of forward and forward + backward (gradients of h, edge_attr, mu and sigma), the
two sides alternating within one process.  Then the whole layer, ``GMMConv`` against ``GINEConv(Linear)`` with
``edge_dim = D`` at the same widths.  No target and no pass / fail threshold: nothing depends on this layer's speed yet.

The baseline is the torch composition on the same GPU: the broadcast ``exp`` for the weights, ``index_select`` of the
source rows, ``(h[j].view(E, K, M) * w[..., None]).sum(-2)``, ``index_add_`` and the division by the degree, which
materialises ``[E, K*M]`` twice forward (the gathered rows, the product) and again in backward; ``index_add_`` adds
with float atomics, so its bits change from run to run where the kernel's do not.  The byte model next to it
(``model_bytes``) counts what the entries must move.  Prints one JSON line; ``--out`` (default
``profiles/gmm_bench.json``) also writes it.  Needs a HIP device (no fallback).
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

SHAPES = ((3, 3, 64), (10, 3, 64), (25, 2, 16), (3, 3, 256))     # (K, D, M)
KNN = 16
LAYER_IN = 64


def alternating_median_ms(fns, iters, warmup):
    """{name: median ms} of the callables of ``fns``, timed with device events in turns (a, b, a, b, ...), so that
    whatever else the machine does falls on both"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: statistics.median(t) for name, t in times.items()}


def model_bytes(N, E, k, d, m):
    """compulsory bytes per launch (computed, not measured): rows read and written, the adjacency (two ptr entries per
    row; per edge one neighbour id and one edge id), the int64 endpoints of dc_gmm_bwd_w, the [K, D] tables"""
    f, idx, tab = 4, 4, 2 * k * d * 4
    return {"weights": E * (d + k) * f + tab,                                            # a in, w out
            "fwd": E * (k * m * f + k * f + 2 * idx) + N * (m * f + 2 * idx),            # h_j and w per edge; y out
            "bwd_h": E * (m * f + k * f + 2 * idx + 2 * idx) + N * (k * m * f + 2 * idx),   # g_y[i], w, deg per edge; g_h out
            "bwd_w": E * (k * m * f + m * f + k * f + 2 * 8 + 2 * idx),                  # h[src], g_y[dst] in, g_w out
            "bwd_params": 2 * E * (2 * k + d) * f + E * d * f + 2 * tab,                # g_w, w, a twice; g_a out
            "torch_fwd_materialised": E * (5 * k * m * f + 2 * m * f + 2 * 8) + N * 2 * m * f}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("gmm_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    N = int(rest.x.size(0))
    pos = rest.pos.to(dev).contiguous()
    graphs = {"soft_mesh": rest.edge_index.to(dev), "knn16": dc.nn.knn_graph(pos, KNN, rest.batch.to(dev))}

    def dev_f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    def both(fns, leaves, gup):
        """forward (no grad) and forward + backward of every callable of ``fns``, the callables alternating"""
        def no_grad(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run
        fwd = alternating_median_ms({n: no_grad(fn) for n, fn in fns.items()}, args.iters, args.warmup)
        fb = alternating_median_ms({n: (lambda fn=fn, n=n: torch.autograd.grad(fn(), leaves[n], gup))
                                    for n, fn in fns.items()}, args.iters, args.warmup)
        return {n: {"fwd": fwd[n], "fwd_bwd": fb[n]} for n in fns}

    result = {"tool": "gmm_bench", "N": N, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "graphs": []}
    for name, ei in graphs.items():
        E = int(ei.size(1))
        g = dc.nn.GMMConv(1, 1, 1, 1).graph(ei, N)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        deg = torch.bincount(dst, minlength=N).clamp(min=1).to(torch.float32).unsqueeze(-1)
        cart = pos[src] - pos[dst]
        cart3 = cart / (2 * cart.abs().max()) + 0.5              # PyG's Cartesian transform: [0, 1]^3
        entry = {"graph": name, "E": E, "shapes": []}
        for k, d, m in SHAPES:
            a = cart3[:, :d].contiguous().requires_grad_(True)
            h = dev_f32(rng.standard_normal((N, k * m))).requires_grad_(True)
            mu = dev_f32(rng.uniform(0, 1, (k, d))).requires_grad_(True)
            sigma = dev_f32(rng.uniform(0.5, 1.5, (k, d))).requires_grad_(True)
            gup = dev_f32(rng.uniform(0.5, 1.5, (N, m)))

            def torch_composition():
                w = torch.exp((-0.5 * (a.view(E, 1, d) - mu.view(1, k, d)).pow(2)
                               / (1e-15 + sigma.view(1, k, d).pow(2))).sum(-1))
                msg = (h.index_select(0, src).view(E, k, m) * w.unsqueeze(-1)).sum(-2)
                return torch.zeros((N, m), device=dev).index_add_(0, dst, msg) / deg

            def kernels():
                return ops.gmm_aggregate(g, h, a, mu, sigma, "mean")

            with torch.no_grad():                                # same maths: the two agree to summation order
                ya, yb = kernels(), torch_composition()
                dist = float((ya - yb).abs().max() / yb.abs().max())
            leaves = [h, a, mu, sigma]
            ms = both({"gmm_aggregate": kernels, "torch_composition": torch_composition},
                      {"gmm_aggregate": leaves, "torch_composition": leaves}, gup)
            entry["shapes"].append({
                "K": k, "D": d, "M": m, "ms": ms, "max_rel_distance_to_torch": dist,
                "kernel_over_torch": {p: ms["gmm_aggregate"][p] / ms["torch_composition"][p] for p in ("fwd", "fwd_bwd")},
                "model_bytes": model_bytes(N, E, k, d, m)})
            # the whole layer against GINEConv(Linear) with edge_dim = D at the same widths
            torch.manual_seed(0)
            gmm = dc.nn.GMMConv(LAYER_IN, m, d, k).to(dev)
            gine = dc.nn.GINEConv(dc.nn.conv._Lin(LAYER_IN, m, bias=True), edge_dim=d).to(dev)
            x = dev_f32(rng.standard_normal((N, LAYER_IN))).requires_grad_(True)
            ad = a.detach()
            layers = {"GMMConv": lambda: ops.resolve(gmm(x, ei, ad)), "GINEConv": lambda: gine(x, ei, ad)}
            lms = both(layers, {"GMMConv": [x] + list(gmm.parameters()), "GINEConv": [x] + list(gine.parameters())}, gup)
            entry["shapes"][-1]["layer"] = {"in_channels": LAYER_IN, "ms": lms,
                                            "gmm_over_gine": {p: lms["GMMConv"][p] / lms["GINEConv"][p]
                                                              for p in ("fwd", "fwd_bwd")}}
        result["graphs"].append(entry)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
