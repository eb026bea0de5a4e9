#!/usr/bin/env python
"""``fps`` and ``knn_interpolate`` (``deformcontact_amd.pointops``, dc_pointops.hip) against their torch compositions on
the same GPU.  No target and no pass / fail threshold: nothing depends on these calls' speed yet.

``fps``, ``random_start=False``, between two synchronises (the batched call reads the node offsets on the host):

* the soft meshes of ``synth.make_batch(32)`` (32 x 1,024 points), ``ratio`` 0.25: 32 chains of 256 picks, one workgroup
  each;
* one cloud of 100,000 uniform points, ``ratio`` 0.05: one chain of 5,000 picks on the workspace kernel;
* one of the soft meshes alone (no batch, so no host read: device events): the latency of one chain of 256 picks.

The baseline is a Python loop per graph and pick of ``torch.minimum`` over the squared distances to the last pick and
``argmax`` (no host read inside the loop); for the equal-sized batch also the same loop over all graphs at once
(``[B, n]`` tensors), which is the most a torch user can do without a kernel.  The picks are compared
(``same_picks``): torch sums the three squares in another order, so a near-tie may legitimately differ.

``knn_interpolate``, rigid -> soft at B = 32 (24,384 sources, 32,768 queries), F = 256, k = 3: device-event medians of
the whole call (neighbour search included) forward and forward + backward, and of its neighbour search alone.  The
baseline is PyG's composition over the compacted ``knn`` result: ``index_select``, the weights, a multiply, two
``index_add_`` and a divide; its backward adds with float atomics.  It is timed with the edges given (``interp``) and
with its ``knn`` call (``total``).

Prints one JSON line; ``--out`` (default ``profiles/pointops_bench.json``) also writes it.  ``--timeout`` seconds (default
600) end a run that hangs.  Needs a HIP device (no fallback).
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deformcontact_amd as dc  # noqa: E402
from deformcontact_amd import neighbors, synth  # noqa: E402


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


def wall_ms(fn, iters, warmup):
    """host clock between two synchronises: the calls that read on the host"""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def torch_fps(p, m):
    """p [..., n, 3] -> the m picks [..., m] of every cloud, started at its first point; no host read"""
    lead = p.shape[:-2]
    dist = torch.full(lead + (p.shape[-2],), float("inf"), device=p.device)
    j = torch.zeros(lead + (1,), dtype=torch.int64, device=p.device)
    out = torch.empty(lead + (m,), dtype=torch.int64, device=p.device)
    for t in range(m):
        out[..., t:t + 1] = j
        c = torch.gather(p, -2, j.unsqueeze(-1).expand(lead + (1, 3)))
        d = p - c
        dist = torch.minimum(dist, (d * d).sum(-1))
        j = dist.argmax(-1, keepdim=True)
    return out


def torch_interpolate(x, pos_x, pos_y, assign):
    yi, xi = assign[0], assign[1]
    d = pos_x.index_select(0, xi) - pos_y.index_select(0, yi)
    w = 1.0 / (d * d).sum(-1, keepdim=True).clamp(min=1e-16)
    num = torch.zeros(pos_y.size(0), x.size(1), device=x.device).index_add_(0, yi, x.index_select(0, xi) * w)
    den = torch.zeros(pos_y.size(0), 1, device=x.device).index_add_(0, yi, w)
    return num / den


def bench_fps(args, dev, result):
    rest = synth.make_batch(32)[0]
    pos, batch = rest.pos.to(dev).contiguous(), rest.batch.to(dev)
    nb, n = 32, pos.size(0) // 32
    m = dc.pointops.fps_count(n, 0.25)
    clouds = pos.view(nb, n, 3)

    def per_graph():
        return torch.cat([g * n + torch_fps(clouds[g], m) for g in range(nb)])

    def batched():
        return (torch_fps(clouds, m) + torch.arange(nb, device=dev).unsqueeze(1) * n).reshape(-1)
    ours = dc.nn.fps(pos, batch, 0.25, random_start=False, batch_size=nb)
    ms = {"kernel": wall_ms(lambda: dc.nn.fps(pos, batch, 0.25, random_start=False, batch_size=nb), args.iters, args.warmup),
          "torch_loop_per_graph": wall_ms(per_graph, args.torch_iters, 1),
          "torch_loop_batched": wall_ms(batched, args.torch_iters, 1)}
    result["fps"].append({"case": "soft_meshes_b32", "graphs": nb, "points_per_graph": n, "ratio": 0.25, "picks": int(ours.numel()),
                          "ms": ms, "torch_over_kernel": {k: v / ms["kernel"] for k, v in ms.items() if k != "kernel"},
                          "same_picks": {"per_graph": bool(torch.equal(ours, per_graph())),
                                         "batched": bool(torch.equal(ours, batched()))}})
    one = clouds[0].contiguous()                                     # no batch: no host read, device events
    ms_one = median_ms(lambda: dc.nn.fps(one, ratio=0.25, random_start=False), args.iters, args.warmup)
    result["fps"].append({"case": "one_soft_mesh", "graphs": 1, "points_per_graph": n, "ratio": 0.25, "picks": m,
                          "ms": {"kernel": ms_one}, "us_per_pick": ms_one * 1e3 / m})
    n = 100_000
    cloud = torch.from_numpy(np.random.default_rng(0).random((n, 3), dtype=np.float32)).to(dev)
    m = dc.pointops.fps_count(n, 0.05)
    ours = dc.nn.fps(cloud, ratio=0.05, random_start=False)
    ms = {"kernel": wall_ms(lambda: dc.nn.fps(cloud, ratio=0.05, random_start=False), args.iters, args.warmup),
          "torch_loop_per_graph": wall_ms(lambda: torch_fps(cloud, m), args.torch_iters, 1)}
    theirs = torch_fps(cloud, m)
    result["fps"].append({"case": "cloud_100k", "graphs": 1, "points_per_graph": n, "ratio": 0.05, "picks": int(ours.numel()),
                          "ms": ms, "us_per_pick": ms["kernel"] * 1e3 / m,
                          "torch_over_kernel": {"torch_loop_per_graph": ms["torch_loop_per_graph"] / ms["kernel"]},
                          "same_picks": {"per_graph": bool(torch.equal(ours, theirs)),
                                         "first_difference_at": int((ours != theirs).nonzero()[0]) if not torch.equal(ours, theirs) else None}})


def bench_interpolate(args, dev, result):
    rest, _, rig = synth.make_batch(32)
    f, k = 256, 3
    pos_x, bx = rig.pos.to(dev).contiguous(), rig.batch.to(dev)
    pos_y, by = rest.pos.to(dev).contiguous(), rest.batch.to(dev)
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(-1, 1, (pos_x.size(0), f)).astype(np.float32)).to(dev).requires_grad_(True)
    gup = torch.from_numpy(rng.uniform(0.5, 1.5, (pos_y.size(0), f)).astype(np.float32)).to(dev)
    assign = dc.nn.knn(pos_x, pos_y, k, bx, by)

    def both(fwd_fn):
        def fwd():
            with torch.no_grad():
                fwd_fn()

        def fwd_bwd():
            torch.autograd.grad(fwd_fn(), [x], gup)
        return {"fwd": median_ms(fwd, args.iters, args.warmup), "fwd_bwd": median_ms(fwd_bwd, args.iters, args.warmup)}
    kernels = lambda: dc.nn.knn_interpolate(x, pos_x, pos_y, bx, by, k=k)
    with torch.no_grad():
        a, b = kernels(), torch_interpolate(x, pos_x, pos_y, assign)
        dist = float((a - b).abs().max() / b.abs().max())
    ms = {"kernels_total": both(kernels),
          "knn_padded": median_ms(lambda: neighbors.knn_padded(pos_x, pos_y, k, bx, by), args.iters, args.warmup),
          "torch_interp": both(lambda: torch_interpolate(x, pos_x, pos_y, assign)),
          "torch_total": both(lambda: torch_interpolate(x, pos_x, pos_y, dc.nn.knn(pos_x, pos_y, k, bx, by))),
          "knn_compacted": wall_ms(lambda: dc.nn.knn(pos_x, pos_y, k, bx, by), args.iters, args.warmup)}
    ms["kernels_interp"] = {p: ms["kernels_total"][p] - ms["knn_padded"] for p in ("fwd", "fwd_bwd")}
    result["knn_interpolate"].append({
        "case": "rigid_to_soft_b32", "Nx": int(pos_x.size(0)), "Ny": int(pos_y.size(0)), "F": f, "k": k,
        "slots": int(assign.size(1)), "ms": ms, "max_rel_distance_to_torch": dist,
        "torch_over_kernels": {"total": {p: ms["torch_total"][p] / ms["kernels_total"][p] for p in ("fwd", "fwd_bwd")},
                               "interp": {p: ms["torch_interp"][p] / ms["kernels_interp"][p] for p in ("fwd", "fwd_bwd")}},
        "model_bytes": {"fwd": 4 * f * (assign.size(1) + pos_y.size(0)),              # rows gathered, rows written
                        "bwd": 4 * f * (assign.size(1) + pos_x.size(0))}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=3, help="timed runs of the torch fps loops (each takes a while)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds after which the run is ended")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointops_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("pointops_bench needs a HIP device")
    signal.alarm(args.timeout)                                       # SIGALRM's default action ends the process
    dev = torch.device("cuda:0")
    result = {"tool": "pointops_bench", "iters": args.iters, "warmup": args.warmup, "torch_iters": args.torch_iters,
              "device": torch.cuda.get_device_name(0), "fps": [], "knn_interpolate": []}
    bench_fps(args, dev, result)
    bench_interpolate(args, dev, result)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
