"""Time the width-F kNN kernel (``neighbors.knn_padded_nd``, csrc/dc_neighbors_nd.hip) and ``DynamicEdgeConv``, in one
process on one box.

Cases:
* ``knn_padded_nd`` on the DGCNN shape - B = 32 clouds x 1,024 points, F = 64 and F = 128, k = 20 - against the torch
  composition a user would write without it: per graph ``torch.cdist`` (and, as a second form, explicit pairwise
  differences squared and summed), then ``topk(k, largest=False)``;
* on the soft-mesh batch (``synth.make_batch(32)``, F = 3) ``knn_padded_nd`` against the grid path ``knn_padded``:
  where brute force loses to the grid (informational);
* one ``DynamicEdgeConv(MLP(128 -> 64), k = 20)`` forward + backward on the F = 64 shape against ``EdgeConv`` with the
  same ``nn`` on a prebuilt graph: the cost of the search (and of the adjacency build of a new graph) inside the layer.

Device events around every call; median of ``--reps`` after ``--warmup``.

    python tools/dynamic_edge_bench.py [--reps 50] [--warmup 5] [--out profiles/r08/dynamic_edge_bench.json]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/dynamic_edge_bench.py --reps 20
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import deformcontact_amd as dc  # noqa: E402
from deformcontact_amd import neighbors, synth  # noqa: E402

B, POINTS, K = 32, 1024, 20


def _event_time(fn, reps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def _commit() -> str:
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True,
                              timeout=10).stdout.strip() or "unknown"
    except Exception:
        return "unknown"


def _torch_cdist_topk(x3: torch.Tensor, k: int):
    """[B, n, F] -> [B, n, k] indices: the batched form of the per-graph loop (equal sizes: one call)"""
    return torch.cdist(x3, x3).topk(k, dim=-1, largest=False).indices


def _torch_diff_topk(x3: torch.Tensor, k: int):
    """pairwise differences, squared and summed over the columns, one graph at a time (B x n x n x F floats at once
    would be 8 GiB at F = 64)"""
    return torch.stack([((g[:, None, :] - g[None, :, :]) ** 2).sum(-1).topk(k, dim=-1, largest=False).indices
                        for g in x3])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dynamic_edge_bench needs a HIP device")
    dev = torch.device("cuda:0")
    reps, warmup = args.reps, args.warmup
    res = {"device": torch.cuda.get_device_name(0), "commit": _commit(), "reps": reps, "warmup": warmup, "cases": {}}
    torch.manual_seed(0)
    batch = torch.arange(B, device=dev).repeat_interleave(POINTS)

    for f in (64, 128):
        x = torch.relu(torch.randn(B * POINTS, f, device=dev))      # post-ReLU features, as a DGCNN layer sees them
        x3 = x.view(B, POINTS, f)
        case = {"graphs": B, "points_per_graph": POINTS, "width": f, "k": K,
                "lane_ops": 3 * B * POINTS * POINTS * f,
                "knn_padded_nd_ms": _event_time(lambda: neighbors.knn_padded_nd(x, x, K, batch, batch), reps, warmup),
                "torch_cdist_topk_ms": _event_time(lambda: _torch_cdist_topk(x3, K), reps, warmup),
                "torch_diff_topk_ms": _event_time(lambda: _torch_diff_topk(x3, K), max(reps // 5, 3), 2)}
        case["cdist_over_nd"] = case["torch_cdist_topk_ms"] / case["knn_padded_nd_ms"]
        case["diff_over_nd"] = case["torch_diff_topk_ms"] / case["knn_padded_nd_ms"]
        case["lane_ops_per_s"] = case["lane_ops"] / (case["knn_padded_nd_ms"] * 1e-3)
        res["cases"][f"knn_B{B}x{POINTS}_F{f}_k{K}"] = case

    rest, _, _ = synth.make_batch(32)
    gp, gb = rest.pos.to(dev), rest.batch.to(dev)
    for k in (5, K):
        case = {"points": int(gp.shape[0]), "graphs": 32, "width": 3, "k": k,
                "knn_padded_nd_ms": _event_time(lambda: neighbors.knn_padded_nd(gp, gp, k, gb, gb, True), reps, warmup),
                "grid_knn_padded_ms": _event_time(lambda: neighbors.knn_padded(gp, gp, k, gb, gb, True), reps, warmup)}
        case["nd_over_grid"] = case["knn_padded_nd_ms"] / case["grid_knn_padded_ms"]
        res["cases"][f"knn_soft_B32_F3_k{k}"] = case

    f = 64
    x = torch.relu(torch.randn(B * POINTS, f, device=dev)).requires_grad_(True)
    mlp = torch.nn.Sequential(torch.nn.Linear(2 * f, 64), torch.nn.ReLU()).to(dev)       # MLP(128 -> 64)
    dyn, static = dc.nn.DynamicEdgeConv(mlp, K), dc.nn.EdgeConv(mlp)
    ei = dc.nn.knn_graph(x.detach(), K, batch, loop=True)

    def step(fn):
        x.grad = None
        for p in mlp.parameters():
            p.grad = None
        fn().sum().backward()
    case = {"graphs": B, "points_per_graph": POINTS, "width": f, "k": K, "edges": int(ei.shape[1]),
            "dynamic_edge_conv_fwd_bwd_ms": _event_time(lambda: step(lambda: dyn(x, batch)), reps, warmup),
            "edge_conv_prebuilt_fwd_bwd_ms": _event_time(lambda: step(lambda: static(x, ei)), reps, warmup),
            "knn_graph_ms": _event_time(lambda: dc.nn.knn_graph(x.detach(), K, batch, loop=True), reps, warmup)}
    case["search_share"] = 1.0 - case["edge_conv_prebuilt_fwd_bwd_ms"] / case["dynamic_edge_conv_fwd_bwd_ms"]
    res["cases"][f"dynamic_edge_conv_B{B}x{POINTS}_F{f}_k{K}"] = case

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
