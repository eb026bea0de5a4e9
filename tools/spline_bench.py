#!/usr/bin/env python
"""SplineConv's route - ``h = ops.dense_linear(x, W2)`` (``[N, K*M]``: every node row times every weight matrix) and
``ops.spline_aggregate`` (``mean_j sum_s b_s(e_ji) h[j, wi_s(e_ji)*M:+M]``, dc_spline.hip) - on two graphs - the soft
batch of the headline, the rest meshes of ``synth.make_batch(32)``, and a kNN graph (k = 16, ``knn_graph``) over the same
vertices - at (kernel_size, D, degree, M) = (5, 3, 1, 64), (5, 2, 1, 64), (3, 3, 2, 32) and (5, 3, 1, 16), open splines,
``in_channels = 16``: device-event medians of forward, and of forward + backward with and without the ``edge_attr``
gradient (gradients of x and weight either way), the two sides alternating within one process.  No target and no pass /
fail threshold: nothing depends on this layer's speed yet.

The baseline is upstream's per-edge form as a torch composition on the same GPU: the basis in torch, then per slot s a
``bmm`` of the gathered source rows ``x[j] [E, 1, in]`` with the gathered weights ``weight[wi[:, s]] [E, in, M]``, scaled
by ``b[:, s]``, summed over s, ``index_add_`` and the division by the degree.  It costs ``2 E S in M`` FLOP and
materialises ``[E, in, M]`` per slot (kept for the backward) where the h route costs ``2 N in K M`` FLOP and ``N K M``
floats whatever E is; ``index_add_`` adds with float atomics, so its bits change from run to run where the kernels' do
not.  The byte model next to it (``model_bytes``) counts what the entries must move.  Prints one JSON line; ``--out``
(default ``profiles/spline_bench.json``) also writes it.  Needs a HIP device (no fallback).
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

SHAPES = ((5, 3, 1, 64), (5, 2, 1, 64), (3, 3, 2, 32), (5, 3, 1, 16))     # (kernel_size, D, degree, M)
KNN = 16
IN = 16


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


def torch_basis(a, ks, degree):
    """(b [E, S], wi [E, S] int64) of open splines in torch ops: the contract of INTEGRATION.md 1.9"""
    E, D = a.shape
    s = torch.arange((degree + 1) ** D, device=a.device)
    b = torch.ones((E, s.numel()), device=a.device)
    wi = torch.zeros((E, s.numel()), dtype=torch.long, device=a.device)
    off = 1
    for d in range(D):
        k = ((s // (degree + 1) ** d) % (degree + 1)).unsqueeze(0)
        v = a[:, d] * float(ks - degree)
        fl = v.detach().floor()
        f = (v - fl).unsqueeze(1)
        wi = wi + torch.remainder(fl.long().unsqueeze(1) + k, ks) * off
        off *= ks
        if degree == 1:
            b = b * (1 - f - k + 2 * f * k)
        else:
            b = b * torch.where(k == 0, 0.5 * f * f - f + 0.5, torch.where(k == 1, -f * f + f + 0.5, 0.5 * f * f))
    return b, wi


def model(N, E, ks, d, degree, m):
    """computed, not measured: compulsory bytes per launch (rows read and written, the adjacency - two ptr entries per
    row; per edge one neighbour id and one edge id -, the int64 endpoints of dc_spline_bwd_b), and the floats and FLOP
    of the h route against upstream's per-edge form"""
    f, idx, k, s = 4, 4, ks ** d, (degree + 1) ** d
    return {"bytes": {"dense_h": N * (IN + k * m) * f + k * m * IN * f,                  # x in, h out, the weights
                      "basis": E * (d * f + s * (f + idx)),                              # a in, b and wi out
                      "fwd": E * (s * (m * f + f + idx) + 2 * idx) + N * (m * f + 2 * idx),    # a column block, b, wi per slot
                      "bwd_h": E * (m * f + s * (f + idx) + 4 * idx) + N * (k * m * f + 2 * idx),   # g_y[i], b, wi, deg; g_h out
                      "bwd_b": E * (s * (m * f + idx + f) + m * f + 2 * 8 + 2 * idx),     # h blocks, g_y[dst] in, g_b out
                      "bwd_a": E * (s * f + 2 * d * f),
                      "torch_fwd_materialised": E * (s * (IN * m * f + 2 * m * f) + IN * f + 2 * 8) + N * 2 * m * f},
            "h_route": {"floats": N * k * m, "flop": 2 * N * IN * k * m},
            "per_edge_form": {"floats_per_slot": E * IN * m, "flop": 2 * E * s * IN * m}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spline_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("spline_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    N = int(rest.x.size(0))
    pos = rest.pos.to(dev).contiguous()
    graphs = {"soft_mesh": rest.edge_index.to(dev), "knn16": dc.nn.knn_graph(pos, KNN, rest.batch.to(dev))}

    def dev_f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    result = {"tool": "spline_bench", "N": N, "in_channels": IN, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "graphs": []}
    for name, ei in graphs.items():
        E = int(ei.size(1))
        g = dc.nn.SplineConv(1, 1, 1, 1).graph(ei, N)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        deg = torch.bincount(dst, minlength=N).clamp(min=1).to(torch.float32).unsqueeze(-1)
        cart = pos[src] - pos[dst]
        cart3 = cart / (2 * cart.abs().max()) + 0.5              # PyG's Cartesian transform: [0, 1]^3
        entry = {"graph": name, "E": E, "shapes": []}
        for ks, d, degree, m in SHAPES:
            k, s = ks ** d, (degree + 1) ** d
            a = cart3[:, :d].contiguous().requires_grad_(True)
            x = dev_f32(rng.standard_normal((N, IN))).requires_grad_(True)
            weight = dev_f32(rng.uniform(-1, 1, (k, IN, m)) / np.sqrt(k * IN)).requires_grad_(True)
            gup = dev_f32(rng.uniform(0.5, 1.5, (N, m)))

            def per_edge_form():
                b, wi = torch_basis(a, ks, degree)
                xj = x.index_select(0, src).unsqueeze(1)
                msg = torch.zeros((E, m), device=dev)
                for t in range(s):
                    msg = msg + b[:, t, None] * torch.bmm(xj, weight.index_select(0, wi[:, t])).squeeze(1)
                return torch.zeros((N, m), device=dev).index_add_(0, dst, msg) / deg

            def h_route():
                h = ops.dense_linear(x, weight.permute(0, 2, 1).reshape(k * m, IN))
                return ops.spline_aggregate(g, h, a, [ks] * d, [True] * d, degree, "mean")

            with torch.no_grad():                                # same maths: the two agree to summation order
                ya, yb = h_route(), per_edge_form()
                dist = float((ya - yb).abs().max() / yb.abs().max())
            fns = {"h_route": h_route, "per_edge_form": per_edge_form}

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        fn()
                return run
            ms = {"fwd": alternating_median_ms({n: no_grad(fn) for n, fn in fns.items()}, args.iters, args.warmup)}
            for mode, leaves in (("fwd_bwd", [x, weight]), ("fwd_bwd_edge_attr", [x, weight, a])):
                a.requires_grad_(mode == "fwd_bwd_edge_attr")
                ms[mode] = alternating_median_ms(
                    {n: (lambda fn=fn: torch.autograd.grad(fn(), leaves, gup)) for n, fn in fns.items()},
                    args.iters, args.warmup)
            entry["shapes"].append({
                "kernel_size": ks, "D": d, "degree": degree, "M": m, "K": k, "S": s, "ms": ms,
                "max_rel_distance_to_torch": dist,
                "h_route_over_per_edge_form": {p: ms[p]["h_route"] / ms[p]["per_edge_form"] for p in ms},
                "model": model(N, E, ks, d, degree, m)})
            print(f"{name} {ks, d, degree, m}: {ms}", file=sys.stderr, flush=True)
        result["graphs"].append(entry)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
