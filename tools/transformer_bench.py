#!/usr/bin/env python
"""TransformerConv against GATConv and GATv2Conv of the same (in, H, C) on the soft batch of the headline - the rest
meshes of ``synth.make_batch(32)``, the batch ``bench.py`` and ``tools/gatv2_bench.py`` use (N = 32,768, E = 196,224),
features of width in = 256: device-event medians of forward and forward + backward for (H, C) = (4, 64), (8, 32),
(2, 128), (1, 256).  No target and no pass / fail threshold: nothing depends on this layer's speed yet.

Two comparisons per shape.  ``layer``: the whole modules - TransformerConv runs four dense blocks (query, key, value,
skip; three with ``root_weight=False``) where GATv2Conv runs two and GATConv one, so the layer figures carry that.
``attention``: the autograd nodes behind the linears on the same operands (``ops.transformer_conv`` against
``ops.gatv2_conv``, no bias, no activation) - the kernels of dc_transformer.hip against those of dc_gatv2.hip; both
scores gather H*C floats per edge, and TransformerConv takes the edge set without the N self loops the GAT layers add.
The byte model next to it (``model_bytes``) counts what the kernels behind the linears must move: rows gathered and
written, per-edge vectors, adjacency.  Prints one JSON line; ``--out`` also writes it.  Needs a HIP device (no
fallback).
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
    """compulsory bytes behind the linears: (TransformerConv forward, TransformerConv backward, GATv2 forward); the
    TransformerConv terms over the E edges as given, GATv2's over E + N (its self loops)"""
    f = nh * c
    row, vec, adj = f * 4, nh * 4, 4

    def agg(ep):
        return ep * (row + vec + adj) + N * row                  # gather the value rows, alpha, other; write the output rows

    def score(ep):
        return ep * (row + adj) + N * row + 3 * ep * vec + agg(ep)   # gather k / xl, read q / xr; alpha written, read, written
    sddmm = E * (row + adj + vec) + N * row
    dst = E * (row + adj) + 4 * E * vec + E * vec + N * row       # alpha, galpha read twice; gl written; k gathered; g_q written
    src = E * (2 * row + 2 * adj + 2 * vec) + 2 * N * row         # q and gm gathered, alpha / gl through to_fwd; g_k, g_v written
    return score(E), sddmm + dst + src, score(E + N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("transformer_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rest = synth.make_batch(32)[0]                               # the headline's soft batch: 32 meshes of 1,024 vertices
    ei = rest.edge_index.to(dev)
    N, E = int(rest.x.size(0)), int(ei.size(1))
    x = torch.from_numpy(rng.uniform(-1, 1, (N, FIN)).astype(np.float32)).to(dev).requires_grad_(True)

    def both(fwd_fn, leaves, gup):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), leaves, gup, allow_unused=True)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}

    def layer(mod, gup):
        return both(lambda: mod(x, ei, relu=True), [x] + list(mod.parameters()), gup)

    result = {"tool": "transformer_bench", "N": N, "E": E, "in": FIN, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "shapes": []}
    for nh, c in ((4, 64), (8, 32), (2, 128), (1, 256)):
        torch.manual_seed(0)
        f = nh * c
        gup = torch.from_numpy(rng.uniform(0.5, 1.5, (N, f)).astype(np.float32)).to(dev)
        tc_mod = dc.nn.TransformerConv(FIN, c, heads=nh).to(dev)
        v2_mod = dc.nn.GATv2Conv(FIN, c, heads=nh).to(dev)
        times = {"gat": layer(dc.nn.GATConv(FIN, c, heads=nh).to(dev), gup), "gatv2": layer(v2_mod, gup),
                 "transformer": layer(tc_mod, gup),
                 "transformer_noroot": layer(dc.nn.TransformerConv(FIN, c, heads=nh, root_weight=False).to(dev), gup)}
        # the nodes behind the linears, on the same operands
        q, k, v = (torch.from_numpy(rng.standard_normal((N, f)).astype(np.float32)).to(dev).requires_grad_(True)
                   for _ in range(3))
        att = v2_mod.att.detach().clone().requires_grad_(True)
        g_tc, g_v2 = tc_mod.graph(ei, N), v2_mod.graph(ei, N)
        node = {"transformer": both(lambda: ops.transformer_conv(g_tc, q, k, v, None, False, nh, False), [q, k, v], gup),
                "gatv2": both(lambda: ops.gatv2_conv(g_v2, v, q, att, None, 0.2, False, nh, False), [v, q, att], gup)}
        mf, mb, v2f = model_bytes(N, E, nh, c)
        result["shapes"].append({
            "H": nh, "C": c, "layer_ms": times, "attention_ms": node,
            "layer_transformer_over_gatv2": {p: times["transformer"][p] / times["gatv2"][p] for p in ("fwd", "fwd_bwd")},
            "layer_transformer_over_gat": {p: times["transformer"][p] / times["gat"][p] for p in ("fwd", "fwd_bwd")},
            "attention_transformer_over_gatv2": {p: node["transformer"][p] / node["gatv2"][p] for p in ("fwd", "fwd_bwd")},
            "model_bytes": {"transformer_fwd": mf, "transformer_bwd": mb, "gatv2_fwd": v2f, "fwd_ratio": mf / v2f}})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
