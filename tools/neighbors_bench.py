"""Time the device kNN / radius graph builders against the host builder they replace, in one process on one box.

Cases (the issue's yardstick):
* ``radius_graph`` of the BASELINE configs[4] cloud (``synth.radius_graph_points(100_000)``: r = 0.02, cap 32);
* ``knn_graph`` with k = 5 and k = 7 over a B = 32 everyday batch (``synth.make_batch(32)``: the soft meshes and the
  rigid spheres, each with its batch vector);
* the host builder of the parent commit on the same inputs: ``synth.radius_graph_points``'s cKDTree build + query
  (``workers`` capped at 16, the CPUs a GPU job gets), and the same query with k + 1 per graph for the kNN cases.

Device times: the PyG-shaped call (host read of the edge total and compaction included) between a synchronise and
a synchronise, and the capturable padded fill alone with device events; median of ``--reps`` after ``--warmup``.

    python tools/neighbors_bench.py [--reps 50] [--warmup 5] [--out profiles/r07/neighbors_bench.json]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/neighbors_bench.py --device-only --reps 20
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import deformcontact_amd as dc  # noqa: E402
from deformcontact_amd import neighbors, synth  # noqa: E402

WORKERS = 16


def _host_radius(pts: np.ndarray, r: float, cap: int):
    """synth.radius_graph_points' builder (parent commit), workers capped at 16."""
    from scipy.spatial import cKDTree
    n = pts.shape[0]
    tree = cKDTree(pts)
    dist, nbr = tree.query(pts, k=cap + 1, distance_upper_bound=r, workers=WORKERS)
    centre = np.repeat(np.arange(n), cap + 1)
    nbr = nbr.reshape(-1)
    ok = (nbr < n) & (nbr != centre)
    return np.stack([nbr[ok], centre[ok]], 0).astype(np.int64)


def _host_knn(pts: np.ndarray, ptr, k: int):
    """The same cKDTree query per graph with k + 1 neighbours (the point itself dropped)."""
    from scipy.spatial import cKDTree
    out = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        tree = cKDTree(pts[a:b])
        _, nbr = tree.query(pts[a:b], k=k + 1, workers=WORKERS)
        centre = np.repeat(np.arange(b - a), k + 1)
        nbr = nbr.reshape(-1)
        ok = (nbr < b - a) & (nbr != centre)
        out.append(np.stack([nbr[ok] + a, centre[ok] + a], 0))
    return np.concatenate(out, 1).astype(np.int64)


def _host_time(fn, reps: int) -> float:
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


def _sync_time(fn, reps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="skip the host builder (profiler runs)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbors_bench needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "commit": _commit(), "reps": args.reps, "warmup": args.warmup,
           "host_workers": WORKERS, "cases": {}}

    pos, ei_host = synth.radius_graph_points(100_000, 0.02, 32)
    p = pos.to(dev)
    e = dc.nn.radius_graph(p, 0.02, max_num_neighbors=32)
    case = {"points": 100_000, "edges": int(e.shape[1]),
            "device_radius_graph_ms": _sync_time(lambda: dc.nn.radius_graph(p, 0.02, max_num_neighbors=32),
                                                 args.reps, args.warmup),
            "device_padded_fill_ms": _event_time(lambda: neighbors.radius_padded(p, p, 0.02, None, None, 32, True),
                                                 args.reps, args.warmup)}
    if not args.device_only:
        pts = pos.numpy()
        case["host_ckdtree_ms"] = _host_time(lambda: _host_radius(pts, 0.02, 32), args.host_reps)
        case["host_over_device"] = case["host_ckdtree_ms"] / case["device_radius_graph_ms"]
        case["host_edges"] = int(ei_host.shape[1])
    res["cases"]["radius_graph_configs4_r0.02_cap32"] = case

    rest, _, rig = synth.make_batch(32)
    for name, g in (("soft", rest), ("rigid", rig)):
        gp, gb = g.pos.to(dev), g.batch.to(dev)
        ptr = g.ptr.tolist()
        for k in (5, 7):
            e = dc.nn.knn_graph(gp, k, gb)
            case = {"points": int(gp.shape[0]), "graphs": 32, "edges": int(e.shape[1]),
                    "device_knn_graph_ms": _sync_time(lambda: dc.nn.knn_graph(gp, k, gb), args.reps, args.warmup),
                    "device_padded_fill_ms": _event_time(lambda: neighbors.knn_padded(gp, gp, k, gb, gb, True),
                                                         args.reps, args.warmup)}
            if not args.device_only:
                pts = g.pos.numpy()
                case["host_ckdtree_ms"] = _host_time(lambda: _host_knn(pts, ptr, k), args.host_reps)
                case["host_over_device"] = case["host_ckdtree_ms"] / case["device_knn_graph_ms"]
            res["cases"][f"knn_graph_{name}_B32_k{k}"] = case
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
