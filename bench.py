#!/usr/bin/env python3
"""bench.py -- M edges/s of the message-passing hot path (encoder fwd+bwd) on MI355X.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

    python bench.py --gpus N ...        (N > 1 without torchrun: this process only spawns the N ranks)

A *step* is one pass of the hot path over one NEW synthetic everyday-deform batch of 32
sample pairs per GPU (BASELINE.json configs[1]): the batch's features and edge_index are
copied into the step's input buffers (device to device: the stand-in for a loader's upload),
both sorted adjacencies + gcn_norm are built (`dc_graph_build`: the reference recomputes
gcn_norm inside every conv call, models/model.py:71,77), then forward through the 2+2 TAGConv
layers of the soft / rigid branches (12 hops + dense blocks), backward from a fixed synthetic
upstream gradient (6 transposed hops + dW/dX), gradient all-reduce over RCCL when N > 1, and
one Adam step on the encoder parameters.  The batches (4 distinct ones, rotated) are resident
in HBM before the timed region.  `value_cached_topology` is the same step replayed on ONE fixed
batch with the adjacency built once outside the loop (round 1's headline).  Prints ONE JSON
line (rank 0).

A plain run sets up, warms up (`--settle` + `--warmup` untimed steps), times `--steps` steps
and prints the headline line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step`, `config`).  `--full` adds everything else to that line: the extra windows,
`value_cached_topology`, the rooflines with their rocprofv3 child passes, strict fp32, the
drop-in wiring, merged branches, other backbones, radius100k, the full-model steps and the CPU
baseline.  `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy;
with the same arguments the inputs are the same in every run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
SOFT = dict(n=1024, e=6132)   # per sample
RIGID = dict(n=762, e=4560)


def hop_bytes(n: int, e: int, f: int, addend: bool) -> int:
    """Gather-model bytes of one hop launch: every neighbour row counted once
    per edge, E*(4 idx + 4 w + 4F gathered row) + N*(4F written row + 4 ptr) [+ N*4F addend].
    At this size most of those reads are L2 hits, so this is NOT what `roofline.achieved` uses."""
    return e * (8 + 4 * f) + n * (4 * f + 4) + (n * 4 * f if addend else 0)


def hop_bytes_compulsory(n: int, e: int, f: int, addend: bool) -> int:
    """Bytes that must cross the memory side per hop launch (SURVEY.md 8(d) "compulsory model",
    the strict lower bound): every index / weight once, every feature row in once and out once,
    E*8 + N*(2*4F + 4) [+ N*4F addend] - what `roofline.achieved` is computed from."""
    return e * 8 + n * (8 * f + 4) + (n * 4 * f if addend else 0)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="sample pairs per GPU")
    ap.add_argument("--settle", type=int, default=150,
                    help="untimed steps of the headline loop before the warm-up steps (clocks / caches settle)")
    ap.add_argument("--windows", type=int, default=4,
                    help="after the K timed steps, this many more K-step windows of the same loop (min / median reported)")
    ap.add_argument("--no-graph", action="store_true", help="do not capture the step in a hipGraph")
    ap.add_argument("--no-optim", action="store_true", help="leave the Adam step out of the step")
    ap.add_argument("--serial-branches", action="store_true",
                    help="soft and rigid branch on ONE stream (default: two overlapped HIP streams)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--cpu-all-cores", action="store_true",
                    help="also time the CPU baseline with os.cpu_count() threads (minutes on a 256-thread host)")
    ap.add_argument("--kernel-reps", type=int, default=100)
    ap.add_argument("--no-full-step", action="store_true",
                    help="skip the extra full-model (encoder + attention + decoder + losses + Adam) B=4 timing")
    ap.add_argument("--no-strict-fp32", action="store_true",
                    help="skip the extra line with the dense blocks on fp32 MFMA (DC_DENSE_SPLIT=0)")
    ap.add_argument("--no-pmc", action="store_true",
                    help="skip the two rocprofv3 --pmc child passes that measure roofline.traffic")
    ap.add_argument("--workload", default="everyday", choices=["everyday", "radius100k"],
                    help="radius100k: only the bf16 100k-point radius-graph stress (BASELINE.json configs[4])")
    ap.add_argument("--no-merged", action="store_true",
                    help="skip the extra line with both branches merged into one block-diagonal launch set")
    ap.add_argument("--headline-only", action="store_true",
                    help="time the headline loop, print its line and stop (the child pass of roofline.kernel_only_us)")
    ap.add_argument("--no-kernel-trace", action="store_true",
                    help="skip the rocprofv3 --kernel-trace child pass that measures roofline.kernel_only_us")
    ap.add_argument("--no-dropin", action="store_true",
                    help="skip the extra line with the reference's own encoder wiring (plain conv(x, edge_index) calls)")
    ap.add_argument("--global-build", dest="segmented_build", action="store_false",
                    help="build the adjacencies with the 5-launch global pipeline even though the batch layout is known")
    ap.add_argument("--no-backbones", action="store_true",
                    help="skip the extra lines with the GCNConv / GATConv encoders on the same batch")
    ap.add_argument("--no-radius100k", action="store_true",
                    help="leave the radius100k extra out of the default line")
    ap.add_argument("--graph-tail", action="store_true",
                    help="N > 1: capture the gradient all-reduce + Adam inside the step's hipGraph (default: eager after it)")
    ap.add_argument("--distinct-batches", type=int, default=4,
                    help="batches rotated through the timed steps (each step sees a new edge_index)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline: the PMC / kernel-trace child passes, the extra "
                         "windows, the cached-topology loop, rooflines, strict fp32, drop-in wiring, merged branches, "
                         "other backbones, radius100k, full-model steps and the CPU baseline (each still has its --no-* "
                         "switch); without it a run sets up, warms up, times --steps steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy (float32): "
                         "the encoder outputs (a fixed, seeded row sample of each above 16 MB), the parameters after "
                         "the Adam step and Adam's moments (or, with --no-optim, the parameter gradients)")
    return ap.parse_args()


def cpu_baseline(batch: int, budget_s: float, all_cores: bool = False):
    """Reference CPU op sequence (oracle/pyg_ref.py: index_select -> mul -> scatter_add_,
    gcn_norm per conv call, 4 F.linear per TAGConv) on the host cores: encoder fwd+bwd on a
    bounded number of iterations of the same B=32 workload.  Reported, not a target."""
    from deformcontact_amd import synth
    from deformcontact_amd.graphnet import ContactEncoder
    from oracle import pyg_ref
    # torch's CPU gather/scatter stop scaling (and then regress badly) past ~32 threads: measured
    # on the 2 x EPYC 9575F GPU box 1 thr 2.24 s, 16 thr 1.19 s, 32 thr 1.15 s, 64 thr 1.81 s,
    # 128 thr 3.41 s per step (tools/cpu_threads.py), so the baseline runs at its best setting.
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    rest, _, rig = synth.make_batch(batch)
    torch.manual_seed(0)
    enc = ContactEncoder([21, 25], 256, conv_module=pyg_ref)
    g_rest = torch.randn(rest.x.shape[0], 256)
    g_rig = torch.randn(rig.x.shape[0], 256)
    edges = rest.edge_index.shape[1] + rig.edge_index.shape[1]

    def one():
        enc.zero_grad(set_to_none=True)
        a, b = enc(rest, rig)
        torch.autograd.backward([a, b], [g_rest, g_rig])

    for _ in range(3):                       # 3 warm-up iterations
        one()
    times = []
    t_start = time.perf_counter()
    while len(times) < 10 and (time.perf_counter() - t_start) < budget_s:
        t0 = time.perf_counter()
        one()
        times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    out = {"value": round(edges / med / 1e6, 4), "unit": "M edges/s", "cores": cores,
           "kind": "port",
           "sample": f"{len(times)} timed iterations (3 warm-ups) of the same B={batch} encoder "
                     f"fwd+bwd, median {med * 1e3:.1f} ms, torch {torch.__version__} CPU ops, "
                     f"{cores} threads (of {os.cpu_count()} logical CPUs; best-scaling setting)"}
    # BASELINE.md section 2 says os.cpu_count() threads: that figure beside the best-scaling one on request (--cpu-all-cores;
    # VERDICT r04 weak 11).  Measured once in round 5 on a 256-thread host (profiles/r05/i_bench.json): 43.8 s per iteration =
    # 0.0078 M edges/s against 1.07 s = 0.32 M edges/s on 32 threads - torch's CPU gather / scatter ops regress past ~32
    # threads - which is why it is not part of the default run (it alone took 90 s of a 122 s bench).
    allc = os.cpu_count() or 1
    if all_cores and allc != cores:
        torch.set_num_threads(allc)
        one()
        ta = []
        t_start = time.perf_counter()
        while len(ta) < 3 and (time.perf_counter() - t_start) < max(budget_s / 3, 5.0):
            t0 = time.perf_counter()
            one()
            ta.append(time.perf_counter() - t0)
        ta.sort()
        out["all_cores"] = {"cores": allc, "value": round(edges / ta[len(ta) // 2] / 1e6, 4),
                            "median_ms": round(ta[len(ta) // 2] * 1e3, 1), "iterations": len(ta)}
        torch.set_num_threads(cores)
    return out


def dense_roofline(dev, n_s: int, n_r: int, reps: int, graphs=None):
    """Second roofline object: the wide dense blocks (about 40 % of the step), MFMA-bound.  The six
    layer-2 launches of a step (forward, dX - a second forward-shaped block -, dW for the soft and
    the rigid branch; F = 256, K = 4 x 256), timed with HIP events AS A STEP LAUNCHES THEM: inside the
    layer-2 op sequence of each branch (3 hops that write the slab -> forward block -> gradient mask ->
    3 transposed hops on the gradient slab -> dX block -> dW block + its slab reduce), so that the
    operands are in the cache state a step leaves them in (the same rule as for the hop's `roofline`).
    The same six launches interleaved on cold, rotating buffers are kept as `cold_us_per_6_launches`.
    `achieved` counts the MFMA FLOPs actually executed (products x algorithmic); `fp32_equivalent` is
    algorithmic FLOPs / time."""
    from deformcontact_amd import _lib, ops
    from deformcontact_amd.graph import current_stream_ptr
    from deformcontact_amd.ops import _i64_array, _ptr_array
    L = _lib.lib()
    st = current_stream_ptr(dev)
    fi = fo = 256
    nseg = 4
    launches, flops = [], 0.0
    keep = []
    branches = []
    for bi, n in enumerate((n_s, n_r)):
        slab = ops._alloc_slab(n, nseg * fi, dev).normal_()      # the product's (row-padded) slab layout
        lds = slab.stride(0)
        xs = [slab[:, s * fi:(s + 1) * fi] for s in range(nseg)]
        ws = [torch.randn(fo, fi, device=dev) / 16 for _ in range(nseg)]
        bias, out, g = torch.randn(fo, device=dev), torch.empty(n, fo, device=dev), torch.randn(n, fo, device=dev)
        gws = [torch.empty(fo, fi, device=dev) for _ in range(nseg)]
        gb = torch.empty(fo, device=dev)
        gslab = ops._alloc_slab(n, nseg * fi, dev)
        gxs = [gslab[:, s * fi:(s + 1) * fi] for s in range(nseg)]
        nb = L.dc_tag_linear_bwd_dw_workspace_bytes(n, fi, fo, nseg)
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        wsb = L.dc_tag_linear_bwd_dx_split_workspace_bytes(fi, fo, nseg)
        wsx = torch.empty(wsb, dtype=torch.uint8, device=dev)
        pa_x, pa_w, pa_gw, pa_gx, pa_ld = (_ptr_array(xs), _ptr_array(ws), _ptr_array(gws),
                                            _ptr_array(gxs), _i64_array([lds] * nseg))
        keep += [slab, ws, bias, out, g, gws, gb, gslab, scratch, wsx, pa_x, pa_w, pa_gw, pa_gx, pa_ld]
        split, npd = ops.DENSE_SPLIT_BF16, ops.DENSE_PRODUCTS

        def fwd(n=n, pa_x=pa_x, pa_ld=pa_ld, pa_w=pa_w, bias=bias, out=out):
            a = (pa_x, pa_ld, pa_w, nseg, bias.data_ptr(), 1, out.data_ptr(), fo, n, fi, fo)
            L.dc_tag_linear_fwd_split(*a, npd, st) if split else L.dc_tag_linear_fwd(*a, st)

        def dx(n=n, g=g, out=out, pa_w=pa_w, pa_gx=pa_gx, pa_ld=pa_ld, wsx=wsx, wsb=wsb):
            if split:
                L.dc_tag_linear_bwd_dx_split(g.data_ptr(), fo, out.data_ptr(), fo, pa_w, nseg, pa_gx, pa_ld,
                                             wsx.data_ptr(), wsb, n, fi, fo, npd, st)
            else:
                L.dc_tag_linear_bwd_dx(g.data_ptr(), fo, out.data_ptr(), fo, pa_w, nseg, pa_gx, pa_ld, n, fi, fo, st)

        def dw(n=n, g=g, out=out, pa_x=pa_x, pa_ld=pa_ld, pa_gw=pa_gw, gb=gb, scratch=scratch, nb=nb):
            a = (g.data_ptr(), fo, out.data_ptr(), fo, pa_x, pa_ld, nseg, pa_gw, nseg, fi, gb.data_ptr(), 0,
                 scratch.data_ptr(), nb, n, fi, fo)
            L.dc_tag_linear_bwd_dw_split(*a, npd, st) if split else L.dc_tag_linear_bwd_dw(*a, st)

        if split and ops.DENSE_F16X2:
            # default path: scaled fp16x2 (3 MFMA products); dX runs as a second forward-shaped
            # block over the hop slab of the masked gradient with the transposed weights
            rowmax = slab.abs().amax(1).contiguous()
            wmax = ops.weight_rowmax(ws)
            wt = torch.stack([w.t().contiguous() for w in ws])
            wts = [wt[s] for s in range(nseg)]
            wtmax = ops.weight_rowmax(wts)
            pa_wt = _ptr_array(wts)
            gx = torch.empty(n, fi, device=dev)
            growmax = gslab.normal_().abs().amax(1).contiguous()
            g0max = growmax.clone()                   # row maxima of the masked gradient (block 0): any upper bound
            keep += [rowmax, wmax, wt, wts, wtmax, pa_wt, gx, growmax, g0max]

            wimg, wtimg = torch.empty(fo, nseg * fi, device=dev), torch.empty(fi, nseg * fo, device=dev)
            L.dc_tag_weight_prep(pa_w, nseg, fo, fi, wmax.data_ptr(), wimg.data_ptr(), wtimg.data_ptr(),
                                 wtmax.data_ptr(), st)
            keep += [wimg, wtimg]

            def fwd(n=n, slab=slab, wimg=wimg, bias=bias, out=out, rowmax=rowmax, wmax=wmax, lds=lds):
                L.dc_tag_linear_fwd_h2p(slab.data_ptr(), lds, wimg.data_ptr(), bias.data_ptr(), 1,
                                        out.data_ptr(), fo, n, nseg * fi, fo, rowmax.data_ptr(),
                                        wmax.data_ptr(), None, 0, st)

            def dx(n=n, gslab=gslab, wtimg=wtimg, gx=gx, growmax=growmax, wtmax=wtmax):
                L.dc_tag_linear_fwd_h2p(gslab.data_ptr(), gslab.stride(0), wtimg.data_ptr(), None, 0, gx.data_ptr(),
                                        fi, n, nseg * fo, fi, growmax.data_ptr(), wtmax.data_ptr(), None, 0, st)

            def dw(n=n, gslab=gslab, pa_x=pa_x, pa_ld=pa_ld, pa_gw=pa_gw, gb=gb, scratch=scratch, nb=nb,
                   g0max=g0max, rowmax=rowmax):
                # as the backward launches it: the masked gradient is block 0 of the gradient slab
                L.dc_tag_linear_bwd_dw_h2(gslab.data_ptr(), gslab.stride(0), None, fo, pa_x, pa_ld, nseg, pa_gw,
                                          nseg, fi, gb.data_ptr(), 0, scratch.data_ptr(), nb, n, fi, fo,
                                          g0max.data_ptr(), rowmax.data_ptr(), st)

            branches.append({"n": n, "slab": slab, "gslab": gslab, "rowmax": rowmax, "growmax": growmax,
                             "g0max": g0max, "out": out, "gout": g, "fwd": fwd, "dx": dx, "dw": dw})

        launches += [fwd, dx, dw]
        flops += 3 * 2.0 * n * fi * nseg * fo
    for f in launches:
        f()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        for f in launches:
            f()
    ev1.record()
    torch.cuda.synchronize()
    cold_ms = ev0.elapsed_time(ev1) / reps
    ms, in_seq = cold_ms, None
    if graphs is not None and len(branches) == 2:
        # the layer-2 op sequence of a step, eager (the host runs ahead of the device: ~15 launches of
        # >= 15 us each per branch), HIP events on this stream around the three dense launches
        evs = []

        def sequence(record):
            for b, g in zip(branches, graphs):
                ops.chained_hops(g, b["slab"], fi, 3, backward=False, rowmax=b["rowmax"])
                e = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if record else None
                if record:
                    e[0].record()
                b["fwd"]()
                if record:
                    e[1].record()
                L.dc_tag_mask_grad(b["gout"].data_ptr(), fo, b["out"].data_ptr(), fo, b["gslab"].data_ptr(),
                                   b["gslab"].stride(0), b["n"], fo, b["g0max"].data_ptr(),
                                   b["growmax"].data_ptr(), st)
                ops.chained_hops(g, b["gslab"], fo, 3, backward=False, rowmax=b["growmax"], transposed=True,
                                 rowmax_has_block0=True)
                if record:
                    e[2].record()
                b["dx"]()
                if record:
                    e[3].record()
                b["dw"]()
                if record:
                    e[4].record()
                    evs.append(e)
        for _ in range(2):
            sequence(False)
        for _ in range(max(reps, 5)):
            sequence(True)
        torch.cuda.synchronize()
        t = {"fwd": [], "dX": [], "dW_incl_reduce": []}
        for e in evs:
            t["fwd"].append(e[0].elapsed_time(e[1]))
            t["dX"].append(e[2].elapsed_time(e[3]))
            t["dW_incl_reduce"].append(e[3].elapsed_time(e[4]))
        nrep = len(evs) // 2
        ms = sum(sum(v) for v in t.values()) / nrep
        in_seq = {k: {"soft_us": round(sum(v[0::2]) / nrep * 1e3, 1), "rigid_us": round(sum(v[1::2]) / nrep * 1e3, 1)}
                  for k, v in t.items()}
    h2 = ops.DENSE_SPLIT_BF16 and ops.DENSE_F16X2
    prod = (3 if h2 else ops.DENSE_PRODUCTS) if ops.DENSE_SPLIT_BF16 else 1
    peak = 2500.0 if ops.DENSE_SPLIT_BF16 else 157.3
    achieved = prod * flops / ms / 1e9
    res = {"bound": "mfma", "kernel": ("dc::k_fwd_h2d x2 (forward, dX in forward shape; both operands by LDS-DMA, MFMA waves + loading waves) / k_dw_h2w "
                                       "(layer-2 dense block, fp16x2, 128 x 256 tiles)" if h2 else
                                       "dc::k_fwd_split / k_dx_split / k_dw_split (layer-2 dense block)")
           if ops.DENSE_SPLIT_BF16 else "dc::k_fwd_fast / k_dx_fast / k_dw_fast",
           "achieved": round(achieved, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
           "executed": (f"{prod} {'fp16' if h2 else 'bf16'} MFMA products per fp32 product tile"
                        if ops.DENSE_SPLIT_BF16 else "fp32 MFMA"),
           "fp32_equivalent_TFLOPs": round(flops / ms / 1e9, 1), "fp32_mfma_peak": 157.3,
           "algorithmic_flop_per_step_l2": flops, "us_per_6_launches": round(ms * 1e3, 1),
           "cold_us_per_6_launches": round(cold_ms * 1e3, 1),
           "cold_frac": round(prod * flops / cold_ms / 1e9 / peak, 4),
           "sustained_bf16_peak_measured": "1.5-1.86 PF/s under DVFS (tools/mfma_peak_bf16.hip)"}
    if in_seq is not None:
        res["measured"] = ("the six launches inside the layer-2 op sequence of a step (hops -> forward -> mask -> "
                           "transposed hops -> dX -> dW + slab reduce, both branches), eager, HIP events on the "
                           "launch stream around each dense launch; `cold_*`: the same launches interleaved on "
                           "cold rotating buffers")
        res["in_sequence_us"] = in_seq
    else:
        res["measured"] = "six launches interleaved on cold rotating buffers, HIP events"
    return res


def dense_roofline_grouped(dev, parts, reps: int):
    """`roofline_mfma` for the merged encoder path: the THREE grouped layer-2 dense launches of a step
    (forward, dX - a second forward-shaped block -, dW + its slab reduce; both branches per launch,
    F = 256, K = 4 x 256), timed with HIP events inside the layer-2 op sequence a step runs (3 merged hops
    -> grouped forward -> grouped gradient mask -> 3 transposed merged hops -> grouped dX -> grouped dW),
    so the operands are in the cache state a step leaves them in.  `achieved` = MFMA FLOPs executed
    (3 fp16 products x algorithmic FLOPs of the REAL rows; padding rows are not counted) / time."""
    from deformcontact_amd import _lib, ops
    from deformcontact_amd.graph import GraphIndex, current_stream_ptr
    from deformcontact_amd.ops import _i64_array, _ptr_array, _vp_array
    L = _lib.lib()
    st = current_stream_ptr(dev)
    fi = fo = 256
    nseg, ng = 4, len(parts)
    mg = GraphIndex.from_parts(parts)
    n = mg.num_nodes
    n_real = sum(r for r in mg.rows)
    slab = ops._alloc_slab(n, nseg * fi, dev).normal_()
    gslab = ops._alloc_slab(n, nseg * fo, dev).normal_()
    for t in (slab, gslab):                      # padding rows are zero rows
        ends = list(mg.row_beg[1:]) + [n]
        for r0, r, r1 in zip(mg.row_beg, mg.rows, ends):
            t[r0 + r:r1].zero_()
    ws = [[torch.randn(fo, fi, device=dev) / 16 for _ in range(nseg)] for _ in range(ng)]
    bias = [torch.randn(fo, device=dev) for _ in range(ng)]
    out = torch.empty(n, fo, device=dev)
    gouts = [torch.randn(r, fo, device=dev) for r in mg.rows]
    gx = torch.empty(n, fi, device=dev)
    gws = [[torch.empty(fo, fi, device=dev) for _ in range(nseg)] for _ in range(ng)]
    gbs = [torch.empty(fo, device=dev) for _ in range(ng)]
    rowmax, g0max, growmax = (torch.zeros(n, device=dev) for _ in range(3))
    wmax, wtmax = torch.empty(ng, fo, device=dev), torch.empty(ng, fi, device=dev)
    wimg, wtimg = torch.empty(ng, fo, nseg * fi, device=dev), torch.empty(ng, fi, nseg * fo, device=dev)
    row_beg, rows = _i64_array(mg.row_beg), _i64_array(mg.rows)
    nb = L.dc_tag_grouped_bwd_dw_workspace_bytes(rows, ng, fi, fo, nseg)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    pv = lambda ts: _vp_array([t.data_ptr() for t in ts])
    xblocks = [slab[:, s * fi:(s + 1) * fi] for s in range(nseg)]
    pa_x, pa_ld = _ptr_array(xblocks), _i64_array([slab.stride(0)] * nseg)

    def prep():
        _lib.check(L.dc_tag_grouped_weight_prep(pv([w for g in ws for w in g]), ng, nseg, fo, fi, pv(list(wmax)),
                                                pv(list(wimg)), pv(list(wtimg)), pv(list(wtmax)), st), "prep")

    def fwd():
        _lib.check(L.dc_tag_grouped_fwd_h2p(slab.data_ptr(), slab.stride(0), ng, row_beg, rows, n, pv(list(wimg)),
                                            pv(bias), 1, out.data_ptr(), fo, nseg * fi, fo, rowmax.data_ptr(),
                                            pv(list(wmax)), st), "fwd")

    def mask():
        _lib.check(L.dc_tag_grouped_mask_grad(pv(gouts), _i64_array([fo] * ng), ng, row_beg, rows, n, out.data_ptr(),
                                              fo, gslab.data_ptr(), gslab.stride(0), fo, g0max.data_ptr(),
                                              growmax.data_ptr(), st), "mask")

    def dx():
        _lib.check(L.dc_tag_grouped_fwd_h2p(gslab.data_ptr(), gslab.stride(0), ng, row_beg, rows, n, pv(list(wtimg)),
                                            None, 0, gx.data_ptr(), fi, nseg * fo, fi, growmax.data_ptr(),
                                            pv(list(wtmax)), st), "dx")

    def dw():
        _lib.check(L.dc_tag_grouped_bwd_dw_h2(gslab.data_ptr(), gslab.stride(0), pa_x, pa_ld, nseg, ng, row_beg, rows,
                                              n, pv([w for g in gws for w in g]), pv(gbs), 0, scratch.data_ptr(), nb,
                                              fi, fo, g0max.data_ptr(), rowmax.data_ptr(), st), "dw")
    prep()
    evs = []

    def sequence(record):
        ops.chained_hops(mg, slab, fi, 3, backward=False, rowmax=rowmax)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if record else None
        if record:
            e[0].record()
        fwd()
        if record:
            e[1].record()
        mask()
        ops.chained_hops(mg, gslab, fo, 3, backward=False, rowmax=growmax, transposed=True, rowmax_has_block0=True)
        if record:
            e[2].record()
        dx()
        if record:
            e[3].record()
        dw()
        if record:
            e[4].record()
            evs.append(e)
    for _ in range(2):
        sequence(False)
    for _ in range(max(reps, 5)):
        sequence(True)
    torch.cuda.synchronize()
    t = {"fwd": [e[0].elapsed_time(e[1]) for e in evs], "dX": [e[2].elapsed_time(e[3]) for e in evs],
         "dW_incl_reduce": [e[3].elapsed_time(e[4]) for e in evs]}
    ms = sum(sum(v) for v in t.values()) / len(evs)
    flops = 3 * 2.0 * n_real * fi * nseg * fo
    achieved = 3 * flops / ms / 1e9
    return {"bound": "mfma", "kernel": "dc::k_fwd_h2d x2 (grouped forward, grouped dX in forward shape) / k_dw_h2w "
                                       "(grouped layer-2 dense blocks of BOTH branches, fp16x2, 128 x 256 tiles)",
            "achieved": round(achieved, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(achieved / 2500.0, 4),
            "executed": "3 fp16 MFMA products per fp32 product tile",
            "fp32_equivalent_TFLOPs": round(flops / ms / 1e9, 1), "fp32_mfma_peak": 157.3,
            "algorithmic_flop_per_step_l2": flops, "us_per_3_launches": round(ms * 1e3, 1),
            "sustained_bf16_peak_measured": "1.5-1.86 PF/s under DVFS (tools/mfma_peak_bf16.hip)",
            "measured": "the three grouped launches inside the layer-2 op sequence of a step (merged hops -> forward "
                        "-> mask -> transposed merged hops -> dX -> dW + slab reduce), eager, HIP events on the "
                        "launch stream around each dense launch; FLOPs of the real rows only",
            "in_sequence_us": {k: round(sum(v) / len(v) * 1e3, 1) for k, v in t.items()}}


def backbone_extra(dev, rest, rig, backbone: str, steps: int = 20):
    """Extra, not the headline: the same B = 32 encoder step (topology build for a new batch + fwd + bwd, one
    hipGraph) with the reference's other backbones (`models/model.py:39`: GCNConv / GATConv, selected by
    network.backbone) - M edges/s on the same batch."""
    from deformcontact_amd import graph as dc_graph
    from deformcontact_amd.graphnet import ContactEncoder
    torch.manual_seed(0)
    enc = ContactEncoder([rest.x.shape[1], rig.x.shape[1]], 256, backbone=backbone).to(dev)
    g_rest = torch.randn(rest.x.shape[0], 256, device=dev)
    g_rig = torch.randn(rig.x.shape[0], 256, device=dev)

    def body():
        for p_ in enc.parameters():
            p_.grad = None
        a, b = enc(rest, rig)
        torch.autograd.backward([a, b], [g_rest, g_rig])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            dc_graph.clear_cache()
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    dc_graph.clear_cache()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        body()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g.replay()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    edges = rest.edge_index.shape[1] + rig.edge_index.shape[1]
    return {"value": round(edges * steps / el / 1e6, 3), "unit": "M edges/s", "ms_per_step": round(el / steps * 1e3, 4),
            "steps": steps, "step": "adjacency build (self loops rewritten) + fwd + bwd of the 2-layer encoder, both "
                                    "branches, hidden 256, one hipGraph; no optimizer"}


def full_step_b4(dev, steps: int = 20, batch: int = 4):
    """Extra, not the headline: the reference's whole train step (train.py:46-58,71-73) at its
    shipped batch size 4 (configs/everyday.json:26) and at the benchmark batch 32 - encoder on the
    HIP path, unmasked cross-attention (flash-style on the library's kernels once the score
    matrix is large, stock PyTorch below that), decoder on the library's dense block, both losses fused
    (dc_contact_loss), FlatAdam."""
    from deformcontact_amd import synth
    from deformcontact_amd.graphnet import EVERYDAY_NETWORK, load_model
    from deformcontact_amd.train import train_step
    rest, deff, rig = (b.to(dev) for b in synth.make_batch(batch))
    torch.manual_seed(0)
    model = load_model(EVERYDAY_NETWORK).to(dev)
    from deformcontact_amd import dp
    from deformcontact_amd.train import losses
    bucket = dp.GradBucket(model.parameters(), direct=True)
    opt = dp.FlatAdam(bucket, lr=4e-4, zero_grad_in_step=True)   # train.py:20 Adam(lr=4e-4), one kernel
    bucket.zero()

    def one():
        o = losses(model, rest, deff, rig, 1.0)                  # train.py:46-58
        o["loss"].backward()
        opt.step()
        return o["loss"].detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            loss_t = one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    run, captured = one, False
    try:
        g = torch.cuda.CUDAGraph()
        with _capture(g):
            loss_t = one()
        run, captured = g.replay, True
    except Exception as e:  # pragma: no cover
        print(f"[bench] full-step hipGraph capture failed ({type(e).__name__}: {e}); eager", file=sys.stderr)
        torch.cuda.synchronize()
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = run()
    torch.cuda.synchronize()
    if not captured:
        loss_t = r
    ms = (time.perf_counter() - t0) / steps * 1e3
    edges = rest.edge_index.shape[1] + rig.edge_index.shape[1]
    big = rest.x.shape[0] * rig.x.shape[0] >= model.multihead_attention.fused_min_scores
    return {"ms_per_step": round(ms, 3), "M_edges_per_s": round(edges / ms / 1e3, 2), "batch": batch,
            "loss": round(float(loss_t), 6), "hipgraph": captured,
            "note": "whole model on the library's kernels; attention " +
                    ("flash-style forward (dc_attn_flash_fwd), backward = dc_attn_flash_ds + three fp16x2 GEMMs over all rows"
                     if big else "softmax materialised on stock PyTorch") +
                    "; L1 + gradient-consistency losses and their gradients in one launch (dc_contact_loss); "
                    "Adam = dc_adam_flat"}


def full_forward(dev, batch: int = 32, steps: int = 10):
    """Extra: the reference's inference path (eval.py: model(rest, rigid) under no_grad) at the benchmark batch - encoder,
    unmasked cross-attention (dc_attn_flash_fwd), decoder - one hipGraph, ms per forward."""
    from deformcontact_amd import synth
    from deformcontact_amd.graphnet import EVERYDAY_NETWORK, load_model
    rest, _, rig = (b.to(dev) for b in synth.make_batch(batch))
    torch.manual_seed(0)
    model = load_model(EVERYDAY_NETWORK).to(dev).eval()
    for e in model.topology(rest, rig) if hasattr(model, "topology") else []:
        e._static_ok = True
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                out = model(rest, rig)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _capture(g):
            out = model(rest, rig)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.replay()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    edges = rest.edge_index.shape[1] + rig.edge_index.shape[1]
    return {"ms_per_forward": round(el / steps * 1e3, 3), "M_edges_per_s": round(edges * steps / el / 1e6, 2),
            "batch": batch, "finite": bool(torch.isfinite(out.pos).all()),
            "note": "whole model forward under no_grad (eval.py), topology cached, one hipGraph"}


def train_loop(dev, batch: int = 4, steps: int = 40):
    """BASELINE.json configs[2]: the REAL loop - `train.train()`'s inner loop on the synthetic dataset: a
    new batch every step from `loaders.PrefetchLoader` (worker-thread assembly, pinned upload on a side
    stream), whole train step (encoder + attention + decoder + both losses + Adam) replayed from ONE
    hipGraph that contains the per-batch topology work (`train.GraphedTrainStep`).  Host wall time per
    step, everything included."""
    from deformcontact_amd import dp
    from deformcontact_amd.graphnet import EVERYDAY_NETWORK, load_model
    from deformcontact_amd.loaders import InMemoryDataset, PrefetchLoader, SyntheticEverydayDataset
    from deformcontact_amd.train import GraphedTrainStep
    torch.manual_seed(0)
    model = load_model(EVERYDAY_NETWORK).to(dev)
    bucket = dp.GradBucket(model.parameters(), direct=True)
    opt = dp.FlatAdam(bucket, lr=4e-4, zero_grad_in_step=True)
    bucket.zero()
    stepper = GraphedTrainStep(model, opt, bucket, 1.0, eager_steps=2)
    # samples generated BEFORE the loop (a dataset's graphs exist before training starts); the loop pays for
    # indexing, collate, pinned upload, per-batch topology and the step - not for synthesising meshes
    ds = InMemoryDataset(SyntheticEverydayDataset((steps + 8) * batch))
    times, losses_ = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, (_, (rest, deff, rig)) in enumerate(PrefetchLoader(ds, batch, dev, shuffle=False, depth=3)):
        out = stepper(rest, deff, rig)
        if i == 7:                                   # graph captured, loader warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if i >= steps + 7:
            break
    loss = float(out["loss"])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return {"ms_per_step": round(ms, 3), "batch": batch, "steps": steps, "graph_replays": stepper.replays,
            "final_loss": round(loss, 6),
            "note": "new batch every step from an in-memory dataset (PrefetchLoader: worker-thread collate, pinned "
                    "upload on a side stream), one hipGraph per step incl. adjacency build; host wall time"}


def radius100k(dev, reps: int = 30):
    """BASELINE.json configs[4]: one 100k-point radius graph with a dense blob (in-degree up to 32,
    mean ~11), 256 features STORED as bf16, two TAGConv(256, 256, K=3) layers forward (bf16 hops
    with fp32 accumulation + bf16 MFMA dense blocks, ReLU fused), nodes in Morton order.
    Reports the forward rate, the bf16 hop against the HBM roofline on compulsory bytes (with and
    without the reordering) and the bf16 dense block against the dense bf16 MFMA peak."""
    from deformcontact_amd import nn as dc_nn
    from deformcontact_amd import ops, synth
    from deformcontact_amd.graph import GraphIndex, NodeOrder

    def timeit(fn, r):
        for _ in range(3):
            fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(r):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / r

    pos, ei = synth.radius_graph_points(100_000, radius=0.02, max_num_neighbors=32)
    pos, ei = pos.to(dev), ei.to(dev)
    n, e, f = pos.shape[0], ei.shape[1], 256
    order = NodeOrder.morton(pos)
    ei_m = order.relabel(ei)
    g_raw, g_m = GraphIndex(ei, n), GraphIndex(ei_m, n)
    x = torch.randn(n, f, device=dev).bfloat16()
    y = torch.empty_like(x)
    comp = e * 8 + n * (2 * 2 * f + 4)                      # idx + w once, bf16 row in once and out once
    t_raw = timeit(lambda: ops.hop_bf16(g_raw.fwd, x, out=y), reps)
    t_m = timeit(lambda: ops.hop_bf16(g_m.fwd, x, out=y), reps)
    x32, y32 = x.float(), torch.empty(n, f, device=dev)
    comp32 = e * 8 + n * (2 * 4 * f + 4)
    t32_raw = timeit(lambda: ops.hop(g_raw.fwd, x32, out=y32), reps)
    t32_m = timeit(lambda: ops.hop(g_m.fwd, x32, out=y32), reps)
    torch.manual_seed(0)
    c1, c2 = dc_nn.TAGConv(f, f).to(dev), dc_nn.TAGConv(f, f).to(dev)
    xm = order.apply(x)
    gm = torch.randn(n, f, device=dev).bfloat16()
    from deformcontact_amd.graph import graph_index
    graph_index(ei_m, n)._static_ok = True                  # constant topology for the captured graphs below

    def fwd():
        with torch.no_grad():
            return c2(c1(xm, ei_m, relu=True, next_conv=c2), ei_m, relu=True)

    def fwd_bwd():
        for p_ in list(c1.parameters()) + list(c2.parameters()):
            p_.grad = None
        y = c2(c1(xm, ei_m, relu=True, next_conv=c2), ei_m, relu=True)
        y.backward(gm)

    def graphed(fn, r):
        """fn as ONE hipGraph, replayed: no host launch cost in the measurement (as the everyday step)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _capture(g):
            fn()
        return timeit(g.replay, r)
    t_fwd = graphed(fwd, max(reps // 3, 3))
    t_fb = graphed(fwd_bwd, max(reps // 3, 3))

    def with_prep():
        """The same forward + backward with everything a NEW point cloud needs in front of it: Morton codes + sort,
        relabelled edge_index, sorted adjacency (both sides) + gcn_norm, reordered features, and the result put back
        in the caller's node order (eager: the sort's bounds are read back on the host)."""
        o = NodeOrder.morton(pos)
        e = o.relabel(ei)
        xx, gg = o.apply(x), o.apply(gm)
        for p_ in list(c1.parameters()) + list(c2.parameters()):
            p_.grad = None
        y = c2(c1(xx, e, relu=True, next_conv=c2), e, relu=True)
        y.backward(gg)
        return o.undo(y.detach())
    t_prep = timeit(with_prep, max(reps // 6, 3))
    # ... and as ONE hipGraph: ordering a new cloud needs no host synchronisation any more (dc_morton_order)
    try:
        t_prep_graph = graphed(with_prep, max(reps // 6, 3))
    except Exception as ex:  # pragma: no cover
        t_prep_graph = None
        print(f"[bench] radius100k: capture of the step with preprocessing failed ({type(ex).__name__}: {ex})", file=sys.stderr)
        torch.cuda.synchronize()
    # the dense block alone: [N, 1024] bf16 slab x [256, 1024] bf16 weights
    from deformcontact_amd import _lib
    from deformcontact_amd.graph import current_stream_ptr
    L, st = _lib.lib(), current_stream_ptr(dev)
    slab = torch.randn(n, 4 * f, device=dev).bfloat16()
    w = (torch.randn(f, 4 * f, device=dev) / 32).bfloat16()
    out = torch.empty(n, f, dtype=torch.bfloat16, device=dev)
    t_d = timeit(lambda: L.dc_tag_linear_fwd_bf16(slab.data_ptr(), 4 * f, w.data_ptr(), None, 1, out.data_ptr(),
                                                  f, 1, n, 4 * f, f, st), reps)
    flop = 2.0 * n * 4 * f * f
    # ... and the weight-gradient block alone: dW_k = gm^T . slab_k (4 segments) + the bias sums, partials reduced
    import ctypes
    gmb = torch.randn(n, f, device=dev).bfloat16()
    gws = [torch.zeros(f, f, device=dev) for _ in range(4)]
    gbias = torch.zeros(f, device=dev)
    nb_dw = L.dc_tag_linear_bwd_dw_bf16_workspace_bytes(n, f, f, 4)
    ws_dw = torch.empty(max(int(nb_dw), 16), dtype=torch.uint8, device=dev)
    gw_ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in gws])
    t_dw = timeit(lambda: L.dc_tag_linear_bwd_dw_bf16(gmb.data_ptr(), f, slab.data_ptr(), 4 * f, 4, gw_ptrs, gbias.data_ptr(),
                                                      0, ws_dw.data_ptr(), nb_dw, n, f, f, st), reps)
    return {
        "workload": f"radius graph, N={n} points (30 % in a dense blob), E={e} (in-degree <= 32), F=256 stored as "
                    "bf16, nodes in Morton order; 2 x TAGConv(256,256,K=3) forward + backward, ReLU fused (configs[4])",
        "fwd_ms": round(t_fwd, 4), "M_edges_per_s_fwd": round(e / t_fwd / 1e3, 1),
        "fwd_bwd_ms": round(t_fb, 4), "M_edges_per_s_fwd_bwd": round(e / t_fb / 1e3, 1),
        # (key meanings as in rounds 1-3: `fwd_bwd_with_prep_ms` is the EAGER time; round 4 silently put the hipGraph
        # time under this key - that one is `fwd_bwd_with_prep_graph_ms`)
        "fwd_bwd_with_prep_ms": round(t_prep, 4),
        "fwd_bwd_with_prep_graph_ms": round(t_prep_graph, 4) if t_prep_graph is not None else None,
        "timing": "fwd / fwd_bwd: ONE hipGraph each (adjacency built once, nodes already in Morton order), replayed, "
                  "HIP events; fwd_bwd_with_prep: eager, per call also Morton codes + sort, edge relabelling, both "
                  "sorted adjacencies + gcn_norm, feature / gradient reordering and the output put back in the "
                  "caller's order; backward = bf16 mask, 3 transposed bf16 hops, forward-shaped bf16 dX block, bf16 "
                  "dW + slab reduce per layer, fp32 master-weight gradients",
        "hop_bf16": {"kernel": "dc::k_spmm_bf16x8 (bf16 rows gathered, fp32 running sum, bf16 stored)",
                     "us_morton": round(t_m * 1e3, 1), "us_unordered": round(t_raw * 1e3, 1),
                     "compulsory_bytes": comp, "frac_morton": round(comp / t_m / 1e6 / HBM_PEAK_GBS, 4),
                     "frac_unordered": round(comp / t_raw / 1e6 / HBM_PEAK_GBS, 4),
                     "G_edge_hops_per_s_morton": round(e / t_m / 1e6, 2)},
        "hop_f32": {"us_morton": round(t32_m * 1e3, 1), "us_unordered": round(t32_raw * 1e3, 1),
                    "frac_morton": round(comp32 / t32_m / 1e6 / HBM_PEAK_GBS, 4),
                    "frac_unordered": round(comp32 / t32_raw / 1e6 / HBM_PEAK_GBS, 4)},
        "dense_bf16": {"kernel": "dc::k_fwd_bf16x<true> (256 x 256 tiles, both operands by LDS-DMA in a four-stage ring)",
                       "us": round(t_d * 1e3, 1), "TFLOPs": round(flop / t_d / 1e9, 1),
                       "frac_of_2500_TF": round(flop / t_d / 1e9 / 2500.0, 4),
                       "GBps_operand_bytes": round((slab.numel() * 2 + out.numel() * 2) / t_d / 1e6, 1)},
        "dw_bf16": {"kernel": "dc::k_dw_bf16d (128 x 256 tiles per segment and node chunk, both operands by LDS-DMA in a "
                              "six-stage ring, transposing LDS reads) + dc::k_dw_reduce",
                    "us": round(t_dw * 1e3, 1), "TFLOPs": round(flop / t_dw / 1e9, 1),
                    "frac_of_2500_TF": round(flop / t_dw / 1e9 / 2500.0, 4),
                    "GBps_operand_bytes": round((slab.numel() * 2 + gmb.numel() * 2) / t_dw / 1e6, 1)},
    }


def measure_traffic(timeout_s: float = 300.0):
    """`roofline.traffic`, measured in THIS run: two rocprofv3 child passes (`--pmc FETCH_SIZE`,
    then `--pmc WRITE_SIZE`: the TCC block cannot hold both in one pass) over `tools/pmc_hop.py`,
    which issues exactly the hop launches `roofline` prices, corrected as MI355X_MICROARCH.md
    prescribes (FETCH_SIZE x2 on gfx950).  Runs BEFORE this process initialises the GPU (a child
    must never be exec'd from a GPU-initialised process).  Returns (bytes per launch | None, note)."""
    import shutil
    import subprocess
    import tempfile
    if "rocprof" in os.environ.get("LD_PRELOAD", "") or os.environ.get("ROCPROFILER_REGISTER_ROOT") \
            or any(k.startswith("ROCPROF") for k in os.environ):
        return None, "skipped: this process is itself being profiled"
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None, "rocprofv3 not found"
    script = os.path.join(ROOT, "tools", "pmc_hop.py")
    out = tempfile.mkdtemp(prefix="dc_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(out, ctr.lower())
            cmd = [rocprof, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "--",
                   sys.executable, script]
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=timeout_s)
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} failed (rc {r.returncode}): " + \
                    r.stderr.decode(errors="replace")[-300:]
        r = subprocess.run([sys.executable, script, "--parse", os.path.join(out, "fetch_size"),
                            os.path.join(out, "write_size")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=60)
        if r.returncode != 0:
            return None, "parse failed: " + r.stderr.decode(errors="replace")[-300:]
        j = json.loads(r.stdout.decode())
        return int(j["hbm_bytes_per_launch"]), (
            f"measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) over "
            f"tools/pmc_hop.py, {j['launches_averaged']} launches averaged, FETCH_SIZE x2 (gfx950), "
            f"raw KiB fetch {j['FETCH_SIZE_KiB_raw']} write {j['WRITE_SIZE_KiB']}")
    except Exception as e:  # pragma: no cover
        return None, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(out, ignore_errors=True)


def measure_kernel_only(batch: int, timeout_s: float = 300.0):
    """`roofline.kernel_only_us`: per-kernel average durations of the headline step from a `rocprofv3 --kernel-trace
    --stats` child pass over THIS file (`--headline-only --serial-branches`: both encoder branches on one stream, so that
    no kernel shares the chip with another one - the regime a per-kernel roofline fraction is defined in), started before
    this process initialises the GPU.  -> ({kernel name: {"calls", "avg_us"}} | None, note).  The stats table is kept as
    `gpurun_out/bench_kernel_stats.csv` when that directory exists (copy it to profiles/)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if "rocprof" in os.environ.get("LD_PRELOAD", "") or os.environ.get("ROCPROFILER_REGISTER_ROOT") \
            or any(k.startswith("ROCPROF") for k in os.environ):
        return None, "skipped: this process is itself being profiled"
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="dc_kt_", dir="/tmp")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--headline-only", "--serial-branches", "--batch", str(batch), "--settle", "20",
               "--steps", "30", "--warmup", "3", "--windows", "0", "--no-pmc", "--no-kernel-trace"]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=timeout_s)
        if r.returncode != 0:
            return None, f"rocprofv3 --kernel-trace failed (rc {r.returncode}): " + r.stderr.decode(errors="replace")[-300:]
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv in the child pass's output"
        res = {}
        for row in csv.DictReader(open(files[0])):
            name = row["Name"].replace("void ", "").split("(")[0]
            if name.startswith("dc::"):
                res[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
        keep = os.path.join(ROOT, "gpurun_out")
        if os.path.isdir(keep):
            shutil.copy(files[0], os.path.join(keep, "bench_kernel_stats.csv"))
        return res, ("rocprofv3 --kernel-trace --stats child pass of `bench.py --headline-only --serial-branches` (one "
                     "stream: no kernel shares the chip with another), graph-replayed headline steps, kernel-only averages")
    except Exception as e:  # pragma: no cover
        return None, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(out, ignore_errors=True)


def _row_sample(t: torch.Tensor, max_bytes: int = 16 << 20) -> torch.Tensor:
    """`t` itself when its float32 rows fit in `max_bytes`, else a fixed sample of its rows (seed 0, in row order)."""
    rows = max(1, max_bytes // (4 * max(t[0].numel(), 1)))
    if t.shape[0] <= rows:
        return t
    idx = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:rows].sort().values
    return t[idx.to(t.device)]


def dump_outputs(path: str, arrays: dict, limit_bytes: int = 64 << 20) -> None:
    """`--dump-outputs`: every array as `path/<name>.npy` in float32, at most `limit_bytes` in all."""
    import numpy as np
    host = {k: v.detach().to(torch.float32).cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > limit_bytes:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {limit_bytes})")
    os.makedirs(path, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(path, k + ".npy"), a)


def _capture(g):
    """Every hipGraph capture of this file: `dp.capture` - thread-local capture checks once a process group exists (RCCL's
    watchdog thread queries events while this thread captures; in the default mode that aborts the process)."""
    from deformcontact_amd import dp
    return dp.capture(g)


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without torchrun: start the N ranks as child processes (this parent never touches
    the GPU; `deformcontact_amd.launch`), relay rank 0's JSON line, return non-zero when a rank failed or the launch
    deadline (DC_LAUNCH_TIMEOUT seconds, default 1500) passed.  Every rank's stdout / stderr and phase markers go to
    DC_RANK_LOG_DIR (default: a fresh temporary directory, named on failure).  On failure a JSON line with `error`
    and the ranks' last phases (`dist.ranks_seen`) is printed instead of the result line."""
    from deformcontact_amd import launch
    res = launch.launch_ranks(n, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                              timeout=float(os.environ.get("DC_LAUNCH_TIMEOUT", "1500")),
                              log_dir=os.environ.get("DC_RANK_LOG_DIR") or None)
    if res.rc == 0:
        sys.stdout.write(res.stdout0)
        sys.stdout.flush()
        return 0
    if res.timed_out:
        sys.stderr.write("bench.py: ranks still running at the launch deadline (DC_LAUNCH_TIMEOUT): stopped\n")
    sys.stderr.write(res.describe() + "\n")
    summ = res.summary()
    print(json.dumps({"metric": "M edges/sec fwd+bwd, everyday-deform batch=32 per GPU (encoder hot path)",
                      "value": None, "n_gpus": n, "error": "launch deadline passed" if res.timed_out else
                      "a rank exited with a non-zero code", "launch": summ,
                      "dist": {"world_size": n, "ranks_seen": summ["ranks"]}}), flush=True)
    return 1


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args.gpus = world
    # DC_BENCH_FORCE_DIST=1 (tests/launch_scenarios.py: bench_rccl_single): ONE rank goes through the N > 1 form of this
    # file - RCCL process group, eager all-reduce + Adam behind the replayed graph, max-over-ranks timing, the `dist`
    # block - because two ranks cannot share the test box's one device under RCCL
    dist_on = world > 1 or os.environ.get("DC_BENCH_FORCE_DIST") == "1"
    from deformcontact_amd.launch import install_watchdog, phase
    if world > 1:
        install_watchdog()                 # DC_RANK_WATCHDOG_S: periodic stack dumps of a rank that is stuck
        # N ranks share the node's cores: N machine-wide OpenMP / MKL pools starve each other (launch.py; torchrun sets
        # OMP_NUM_THREADS = 1 for the same reason)
        from deformcontact_amd.launch import rank_cpu_threads
        torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", rank_cpu_threads(world))))
    stall = os.environ.get("DC_TEST_STALL_RANK")       # tests/test_z_launch.py: a rank that never gets anywhere
    if stall is not None and stall in ("all", str(rank)):
        phase("stalled (DC_TEST_STALL_RANK)")
        time.sleep(3600)
    phase("start")
    traffic, traffic_note = None, "not measured at N > 1"
    kernel_only, kernel_only_note = None, "not measured"
    if world == 1 and args.full:
        traffic, traffic_note = (None, "--no-pmc") if args.no_pmc else measure_traffic()
        if not (args.no_kernel_trace or args.headline_only or args.workload != "everyday"):
            kernel_only, kernel_only_note = measure_kernel_only(args.batch)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback in deformcontact_amd)")
    if args.workload == "radius100k":
        if args.dump_outputs:
            raise SystemExit("bench.py: --dump-outputs writes the everyday workload's step (not --workload radius100k)")
        torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
        r = radius100k(torch.device("cuda", torch.cuda.current_device()), args.kernel_reps // 3 or 3)
        if rank == 0:
            print(json.dumps({"metric": "M edges/sec fwd, 100k-node radius graph, bf16 features (configs[4])",
                              "value": r["M_edges_per_s_fwd"], "unit": "M edges/s", "n_gpus": 1, "steps": 1,
                              "warmup": 0, "ms_per_step": r["fwd_ms"], "higher_is_better": True,
                              "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                              "config": {"workload": r["workload"]}, "radius100k": r}), flush=True)
        return
    ndev = torch.cuda.device_count()
    dev_index = local_rank % max(ndev, 1)     # == local_rank on a real N-GPU node
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if os.environ["MASTER_ADDR"] in ("127.0.0.1", "localhost", "::1"):
            # one node: RCCL's socket bootstrap (not its data path: that is xGMI / shared memory) stays on the loopback interface
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        # RCCL ("nccl") over xGMI; DC_DIST_BACKEND=gloo only exists to smoke-test the N > 1 code
        # path on a single-GPU box (several ranks sharing one device)
        backend = os.environ.get("DC_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            # ranks of one node: keep gloo's pairwise connections on the loopback interface (a container hostname that
            # resolves to an address the ranks cannot reach each other on leaves them waiting in the rendezvous)
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            import datetime
            dist.init_process_group(backend, timeout=datetime.timedelta(
                seconds=float(os.environ.get("DC_GLOO_TIMEOUT_S", "120"))))
        phase(f"process group up ({backend})")

    from deformcontact_amd import dp, ops, synth
    from deformcontact_amd.graph import clear_cache, graph_index
    from deformcontact_amd.graphnet import ContactEncoder

    # ---- workload: B sample pairs per rank and step, distinct geometry per rank and per batch ----
    from deformcontact_amd import graph as dc_graph
    nb = max(1, args.distinct_batches)
    # A batch travels as ONE packed buffer, as `loaders.PrefetchLoader` uploads it (every tensor of the batch triple at
    # a 256-byte aligned offset of one pinned staging buffer, one copy): the step's static input tensors are views
    # into one device buffer and a new batch arrives with ONE device-to-device copy (round 2 issued four).
    pool, layout, static_buf = [], None, None
    for j in range(nb):
        r_h, _, g_h = synth.make_batch(args.batch, first_idx=(j * world + rank) * args.batch)
        tensors = (r_h.x, r_h.edge_index, g_h.x, g_h.edge_index)
        if layout is None:
            layout, off = [], 0
            for t in tensors:
                layout.append((off, t.numel() * t.element_size(), t.dtype, tuple(t.shape)))
                off += (t.numel() * t.element_size() + 255) // 256 * 256
            static_buf = torch.empty(off, dtype=torch.uint8, device=dev)
        assert all(tuple(t.shape) == l[3] for t, l in zip(tensors, layout)), "batches of one shape expected"
        packed = torch.empty_like(static_buf)
        for t, (off, nbytes, dt, shp) in zip(tensors, layout):
            packed[off:off + nbytes].view(dt).view(shp).copy_(t.to(dev))
        pool.append(packed)
        if j == 0:
            rest, rig = r_h.to(dev), g_h.to(dev)           # the step's (static) input batches ...
            views = [static_buf[off:off + nbytes].view(dt).view(shp) for off, nbytes, dt, shp in layout]
            lay_s, lay_r = rest.segments(), rig.segments()
            rest.x, rest.edge_index, rig.x, rig.edge_index = views   # ... whose tensors live in the packed buffer
            if args.segmented_build:
                # every batch of the pool has this layout (B meshes of one size): the adjacency build may use it
                rest.assume_segments(lay_s)
                rig.assume_segments(lay_r)
            static_buf.copy_(packed)
    n_s, e_s = rest.x.shape[0], rest.edge_index.shape[1]
    n_r, e_r = rig.x.shape[0], rig.edge_index.shape[1]
    edges_per_rank = e_s + e_r
    slots = ((rest, rig),)

    def load(j: int, slot=0) -> None:
        """A new batch arrives: features + edge_index of both graphs into the step's input buffers - one packed
        device-to-device copy (the stand-in for the loader's single upload per batch)."""
        static_buf.copy_(pool[j % nb])

    torch.manual_seed(0)                      # identical init on every rank
    enc = ContactEncoder([21, 25], 256).to(dev)
    enc.overlap_branches = not args.serial_branches
    dp.broadcast_parameters(enc)
    gen = torch.Generator(device=dev).manual_seed(1 + rank)
    g_rest = torch.randn(n_s, 256, device=dev, generator=gen)
    g_rig = torch.randn(n_r, 256, device=dev, generator=gen)
    bucket = dp.GradBucket(enc.parameters(), direct=True)
    # Adam defaults, one HIP kernel that also clears the gradients it consumed (zero_grad)
    opt = None if args.no_optim else dp.FlatAdam(bucket, lr=4e-4, zero_grad_in_step=True)
    bucket.zero()
    k_hops = enc.conv_layers_resting[0].K

    model_box = [enc]                                  # the module a step runs (the drop-in leg swaps the wiring, same parameters)
    # --dump-outputs: the encoder outputs of the latest step stay referenced (a captured step's outputs are then the
    # graph's static tensors, rewritten by every replay); without it nothing is held, as before
    last_out = [] if args.dump_outputs else None

    def fwd_bwd(slot=0):
        if opt is None:
            bucket.zero()
        a, b = model_box[0](*slots[slot])
        if last_out is not None:
            last_out[:] = (a, b)
        torch.autograd.backward([a, b], [g_rest, g_rig])

    ar_events = []                                     # HIP events around the gradient all-reduce (N > 1)

    ar_calls = [0, 0.0]                                # all-reduces this rank has issued (phase markers carry it), time of the last marker

    def tail():
        ar_calls[0] += 1
        if dist_on and (ar_calls[0] <= 4 or time.monotonic() - ar_calls[1] >= 1.0):
            # progress markers that let a slow launch be told from a stuck one (a file append when DC_RANK_LOG_DIR is set):
            # at most one per second - on a healthy box a step takes a millisecond and a marker per step put a file open /
            # append / close inside every timed step; on a crawling box every step still leaves one
            ar_calls[1] = time.monotonic()
            phase(f"collective {ar_calls[0]}")
        if dist_on and len(ar_events) < 4096:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            bucket.all_reduce_mean()
            if world == 1:                     # (forced one-rank form: GradBucket skips the collective at world size 1)
                dist.all_reduce(bucket.flat, op=dist.ReduceOp.AVG)
            e1.record()
            ar_events.append((e0, e1))
        else:
            bucket.all_reduce_mean()
        if opt is not None:
            opt.step()

    def barrier():
        if dist_on:
            dist.barrier()

    captured = []

    def capture(body):
        """`body()` as one hipGraph (None with --no-graph or if capture fails)."""
        if args.no_graph:
            return None
        try:
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                body()
            captured.append(g)
            return g
        except Exception as e:  # pragma: no cover
            if rank == 0:
                print(f"[bench] hipGraph capture failed ({type(e).__name__}: {e}); running eager",
                      file=sys.stderr)
            torch.cuda.synchronize()
            return None

    def warm(fn, reps=3):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(reps):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    # N > 1: the collective stays OUTSIDE the captured graph by default (the 2-rank tests cover exactly this form);
    # --graph-tail captures all-reduce + Adam with the step (RCCL collectives are capturable; falls back to eager if
    # the capture fails) - opt-in because it cannot be exercised on the one-GPU test box
    tail_in_graph = not dist_on or bool(args.graph_tail)

    def make_mode(mode: str):
        """-> step(i).  serial: every step loads a new batch into the input buffers and the captured
        step rebuilds the adjacency and the first-layer hops before training on it; cached: one fixed
        batch, adjacency + first-layer hops built once outside the loop.
        (Tried and dropped in round 2: preparing batch i+1 on another stream - inside the step's graph
        as a third branch, as its own graph, or eagerly - while batch i trains: 0.8955 / 0.951 / 0.946 ms
        against 0.8953 / 0.946 ms serial; the dependent chain of small topology kernels gains nothing
        from running beside the training kernels on this runtime.)"""
        dc_graph.clear_cache()
        if mode == "cached":
            load(0, 0)
            for g_ in enc.topology(*slots[0]):
                g_._static_ok = True                                        # constant for the graph's life

            def body():
                fwd_bwd(0)
                if tail_in_graph:
                    tail()
            warm(lambda: (fwd_bwd(0), tail()))
            g = capture(body)

            def step(i):
                if g is not None:
                    g.replay()
                    if not tail_in_graph:
                        tail()
                else:
                    fwd_bwd(0)
                    tail()
            return step
        if mode == "serial":
            def body():
                fwd_bwd(0)                        # adjacency is built inside (never reused under capture)
                if tail_in_graph:
                    tail()
            load(0, 0)
            phase(f"serial: warm (all-reduces so far {ar_calls[0]})")
            warm(lambda: (fwd_bwd(0), tail()))
            dc_graph.clear_cache()
            phase(f"serial: capture (all-reduces so far {ar_calls[0]})")
            g = capture(body)
            phase(f"serial: captured={g is not None}")

            def step(i):
                load(i, 0)
                if g is not None:
                    g.replay()
                    if not tail_in_graph:
                        tail()
                else:
                    fwd_bwd(0)
                    tail()
            return step
        raise ValueError(mode)

    def timed(step, steps, warmup):
        for i in range(warmup):
            step(i)
        phase(f"timed: warmup steps done (all-reduces so far {ar_calls[0]})")
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(warmup + i)
        torch.cuda.synchronize()
        barrier()
        elapsed = time.perf_counter() - t0
        phase(f"timed: {steps} steps done (all-reduces so far {ar_calls[0]})")
        if dist_on:
            # (gloo - the one-device stand-in - takes the host tensor: dp.staged_collective says why)
            t = torch.tensor([elapsed], device=dev if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed

    # ---- headline: every step is a NEW batch: load + adjacency / gcn_norm build + first-layer hops + train ----
    warmup = max(args.warmup, 1)
    serial_step = make_mode("serial")
    # the device's clocks and caches settle over the first ~0.1 s of graph replays (round 5: the first 50-step window after the
    # captures was up to 3.5 % slower than the four behind it): `--settle` untimed steps of the same loop come before the W
    # warm-up steps and the K timed ones (reported in config.settle_steps)
    for i in range(max(args.settle, 0)):
        serial_step(i)
    elapsed = timed(serial_step, args.steps, warmup)
    ms_per_step = elapsed / args.steps * 1e3
    value = edges_per_rank * world * args.steps / elapsed / 1e6
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller: the encoder outputs and the state the Adam step left (parameters,
        # moments) - or, with --no-optim, the gradients in the bucket
        torch.cuda.synchronize()
        arrays = {"out_rest": _row_sample(last_out[0]), "out_rigid": _row_sample(last_out[1])}
        names = {id(p): n for n, p in enc.named_parameters()}
        for p, off in zip(bucket.params, bucket.offsets):
            n, sl = names[id(p)], slice(off, off + p.numel())
            if opt is None:
                arrays["grad." + n] = bucket.flat[sl].view_as(p)
            else:
                arrays["param." + n] = opt.flat_param[sl].view_as(p)
                arrays["adam_exp_avg." + n] = opt.exp_avg[sl].view_as(p)
                arrays["adam_exp_avg_sq." + n] = opt.exp_avg_sq[sl].view_as(p)
        dump_outputs(args.dump_outputs, arrays)
    # the same loop again, `--windows` more windows of K steps each (the driver's 20-step window is
    # 13 ms of a 40 s run; min / median over windows say how far one window can sit from the typical one).  `value` above
    # stays the FIRST window - the K steps the contract times.
    window_ms = [round(ms_per_step, 4)]
    for _ in range(max(args.windows, 0) if args.full else 0):
        window_ms.append(round(timed(serial_step, args.steps, 0) / args.steps * 1e3, 4))
    if args.headline_only:
        if rank == 0:
            print(json.dumps({"metric": "M edges/sec fwd+bwd, everyday-deform batch=32 per GPU (encoder hot path)",
                              "value": round(value, 3), "unit": "M edges/s", "n_gpus": world, "steps": args.steps,
                              "warmup": warmup, "ms_per_step": round(ms_per_step, 4), "headline_only": True,
                              "two_stream_branches": not args.serial_branches}), flush=True)
        if dist_on:
            dist.barrier()
            dist.destroy_process_group()
        return
    # ---- secondary: the per-batch topology work left out of the loop (round-1 headline definition) ----
    elapsed_c = timed(make_mode("cached"), args.steps, warmup) if args.full else None
    graph_used = len(captured) >= (2 if args.full else 1)       # every mode timed really replays a captured graph

    out = {
        "metric": "M edges/sec fwd+bwd, everyday-deform batch=32 per GPU (encoder hot path)",
        "value": round(value, 3), "unit": "M edges/s", "n_gpus": world, "steps": args.steps,
        "warmup": warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        # storage, hops and every accumulation in fp32; the arithmetic of the dense blocks is in the label (VERDICT r04
        # weak 4): `strict_fp32` below is the same step with every product on fp32 arithmetic
        "dtype": ("f32 (hops, storage, accumulate); wide dense blocks fp16x2-split operands (3 fp16 MFMA products, fp32 "
                  "accumulate), narrow ones bf16x3-split (6 products)") if (ops.DENSE_SPLIT_BF16 and ops.DENSE_F16X2) else
                 ("f32 (dense blocks bf16x3-split operands, 6 bf16 MFMA products, fp32 accumulate)" if ops.DENSE_SPLIT_BF16
                  else "f32"),
        "data": "synthetic",
        "dense_arithmetic": (("fp32 storage and accumulate; wide dense blocks as power-of-two-scaled 2-way "
                              "fp16 splits (3 fp16 MFMAs per product tile, fp32-accurate), narrow ones as "
                              "exact 3-way bf16 splits (6 bf16 MFMAs)") if ops.DENSE_F16X2 else
                             ("fp32 storage and accumulate; dense products as exact 3-way bf16 splits "
                              "(6 bf16 MFMAs per product tile, fp32-accurate)")) if ops.DENSE_SPLIT_BF16
        else "fp32 MFMA (v_mfma_f32_32x32x2_f32)",
        "config": {
            "workload": f"everyday-deform synthetic, B={args.batch} sample pairs per GPU: soft "
                        f"{args.batch}x(1024 v, 6132 e) + rigid {args.batch}x(762 v, 4560 e); "
                        "TAGConv encoder 2 layers/branch, hidden 256, K=3 (configs[1])",
            "edges_per_gpu_step": edges_per_rank, "global_batch": args.batch * world, "settle_steps": max(args.settle, 0),
            "step": f"EVERY step: a new batch (1 of {nb} distinct, rotated) is copied into the input buffers "
                    "(ONE packed device-to-device copy, as the loader uploads a batch), both sorted adjacencies + gcn_norm are built for both graphs "
                    + ("(dc_graph_build_segmented: one launch per graph, the batch layout is host data)"
                       if args.segmented_build else "(dc_graph_build)")
                    + ", the first-layer hop slabs are computed, then fwd + bwd(synthetic "
                    "upstream grad)" + (" + RCCL grad all-reduce" if dist_on else "")
                    + ("" if args.no_optim else " + Adam") + "; all of it inside the timed region, one hipGraph",
            "hipgraph": graph_used, "two_stream_branches": not args.serial_branches,
            "merged_branches": bool(enc._mergeable(rest.x, rig.x)),
            "segmented_adjacency_build": all(getattr(g_, "_segments", None) is not None
                                             for g_ in enc.topology(rest, rig)),
            "parallelism": f"dp{world}",
        },
    }

    if args.full:
        out["ms_per_step_windows"] = {"windows": len(window_ms), "steps_each": args.steps, "min": min(window_ms),
                                      "median": sorted(window_ms)[len(window_ms) // 2], "max": max(window_ms),
                                      "note": "window 0 is `ms_per_step` (the K steps the contract times); the others "
                                              "repeat the same K-step loop in the same process"}
        out["value_cached_topology"] = round(edges_per_rank * world * args.steps / elapsed_c / 1e6, 3)
        out["ms_per_step_cached_topology"] = round(elapsed_c / args.steps * 1e3, 4)
        out["config"]["value_cached_topology"] = ("one fixed batch replayed, adjacency and first-layer hops built once "
                                                  "outside the loop (round-1 headline definition)")
    if dist_on:
        torch.cuda.synchronize()
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in ar_events[-max(args.steps, 1):])
        # which physical devices took part: every rank reports the device it ran on (UUID where the runtime exposes
        # one, else PCI location), all-gathered - the driver can check that N ranks mean N distinct GPUs
        props = torch.cuda.get_device_properties(dev)
        ident = str(getattr(props, "uuid", "") or "")
        if not ident or set(ident.replace("-", "")) <= {"0"}:
            ident = "pci:%s:%s:%s" % tuple(getattr(props, k, "?") for k in ("pci_domain_id", "pci_bus_id", "pci_device_id"))
        mine = {"rank": rank, "local_rank": local_rank, "device_index": dev_index, "device": ident, "name": props.name,
                "host": os.uname().nodename}
        seen = [None] * world
        dist.all_gather_object(seen, mine)
        # host-side cost of the eager tail (all-reduce + Adam launched from Python after every graph replay)
        th0 = time.perf_counter()
        for _ in range(20):
            tail()
        tail_host_us = (time.perf_counter() - th0) / 20 * 1e6
        torch.cuda.synchronize()
        out["dist"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                       "ranks_seen": seen,
                       "distinct_devices": len({(r["host"], r["device"]) for r in seen}),
                       "tail": "eager after the replayed fwd+bwd graph (all_reduce + dc_adam_flat: 2 launches)"
                               if not tail_in_graph else "inside the step's hipGraph",
                       "tail_host_us_per_step": round(tail_host_us, 1),
                       "allreduce_bytes": int(bucket.flat.numel() * bucket.flat.element_size()),
                       "allreduce_us": round(us[len(us) // 2], 1) if us else None,
                       "allreduce_us_max": round(us[-1], 1) if us else None,
                       "collective": "one all_reduce(AVG) per step over the flat fp32 gradient bucket "
                                     "(dp.GradBucket.all_reduce_mean), issued after the captured fwd+bwd; HIP events "
                                     "on rank 0's stream around the call, median / max over the timed steps"}
    if rank == 0 and args.full:
        # ---- roofline of the dominant kernel: the F=256 hop as a step launches it
        # (k_spmm_wave<4,8,true>: the hop + the row maxima the dense block scales by; forward over
        # the sorted adjacency, backward - on the masked gradient - over the transposed one) ----
        from tools import pmc_hop
        from deformcontact_amd.graph import GraphIndex
        f = 256
        merged = enc._mergeable(rest.x, rig.x)
        parts = [(rest.edge_index, n_s), (rig.edge_index, n_r)]

        def graph_time(fn, launches_per_call: int, calls: int = 20):
            """Device time per launch of `fn` (which enqueues `launches_per_call` kernels), replayed from
            a hipGraph `calls` x per replay so that the host (ctypes + Python, ~15 us per launch - as
            long as the kernel itself) is out of the measurement, exactly as in the graph-replayed step;
            HIP events on this stream, launch gaps inside the graph included."""
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                for _ in range(calls):
                    fn()
            g.replay()
            reps = max(args.kernel_reps // calls, 2)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(reps):
                g.replay()
            ev1.record()
            torch.cuda.synchronize()
            return ev0.elapsed_time(ev1) / (reps * calls * launches_per_call)

        # isolated launches (same launch back to back): the adjacency a step hops over, both directions
        per_case = {}
        iso = [("merged", GraphIndex.from_parts(parts), n_s + n_r, e_s + e_r)] if merged else \
            [("soft", GraphIndex(rest.edge_index, n_s), n_s, e_s), ("rigid", GraphIndex(rig.edge_index, n_r), n_r, e_r)]
        for name, g, n, e in iso:
            slab = ops._alloc_slab(g.num_nodes, 4 * f, dev).normal_()
            rm = torch.zeros(g.num_nodes, device=dev)
            for tag, adj, x, o in (("fwd", g.fwd, slab[:, :f], slab[:, f:2 * f]),
                                   ("bwd", g.bwd, slab[:, 2 * f:3 * f], slab[:, 3 * f:])):
                ms = graph_time(lambda: ops.hop(adj, x, out=o, rowmax=rm, rowmax_mode=2), 1)
                cb = hop_bytes_compulsory(n, e, f, False)
                per_case[f"{name}_{tag}"] = {"compulsory_bytes": cb, "us": round(ms * 1e3, 2),
                                             "GBps": round(cb / ms / 1e6, 1),
                                             "frac": round(cb / ms / 1e6 / HBM_PEAK_GBS, 4)}
        # the roofline figure: the F=256 hop launches of a step IN THE ORDER AND ON THE BUFFERS a step uses -
        # the forward chain block0 -> 1 -> 2 -> 3 of the layer-2 slab (each hop reads what the previous one
        # wrote) and the same chain over the transposed adjacency on the gradient slab, all with the row-maxima
        # side output; merged encoder path: 6 launches over the merged adjacency of both branches, else 12
        seg_list = None if merged else [rest.segments() if callable(getattr(rest, "segments", None)) else None,
                                        rig.segments() if callable(getattr(rig, "segments", None)) else None]
        if not args.segmented_build:
            seg_list = None
        in_step_sequence, nlaunch, comp_bytes, gath_bytes = pmc_hop.hop_sequence(dev, parts, merged, f, segments=seg_list)
        nhops = 6 if merged else 12                             # F=256 hops of a step, whatever the launch count
        chained = nlaunch < nhops
        tot_ms = graph_time(in_step_sequence, nlaunch, calls=5) * nlaunch
        achieved = comp_bytes / tot_ms / 1e6                     # GB/s of per-hop compulsory bytes
        # what a fused 3-hop launch itself has to move: the source block in once, three blocks out, the adjacency once
        fused_min = sum(2 * (e_ * 8 + n_ * (4 * 4 * f + 4)) for n_, e_ in ((n_s, e_s), (n_r, e_r)))
        # ---- what `frac` is: the bytes a launch MOVES - the PMC counters' traffic when this run
        # measured it, else the fused launch's minimum (source block in once, three blocks out, adjacency once) - over the
        # kernel-only average duration of a rocprofv3 --kernel-trace pass, over 8 TB/s.  The per-hop-compulsory figure of
        # rounds 2 - 5 (bytes the three hop units WOULD move hop by hop / graph-replay time) is kept under its own name.
        work_equiv = achieved
        hop_ko = {k: v for k, v in (kernel_only or {}).items() if "k_hop_chain" in k or "k_spmm_wave" in k}
        ko_calls = sum(v["calls"] for v in hop_ko.values())
        ko_avg_us = sum(v["calls"] * v["avg_us"] for v in hop_ko.values()) / ko_calls if ko_calls else None
        if chained:
            moved = float(traffic) if traffic is not None else fused_min / nlaunch
            moved_src = ("PMC counters of this run (FETCH_SIZE x 2 + WRITE_SIZE, per launch)" if traffic is not None else
                         "fused launch's minimum: source block in once, 3 blocks out, adjacency once")
        else:
            moved = float(traffic) if traffic is not None else comp_bytes / nlaunch
            moved_src = "PMC counters of this run" if traffic is not None else "per-hop compulsory bytes"
        t_us = ko_avg_us if ko_avg_us is not None else tot_ms / nlaunch * 1e3
        achieved = moved / t_us / 1e3                               # GB/s
        per_kernel = {}
        if chained and hop_ko:
            for tag, n_, e_ in (("soft", n_s, e_s), ("rigid", n_r, e_r)):
                steps_ = (n_ // args.batch + 127) // 128
                hit = [(k, v) for k, v in hop_ko.items() if k.endswith(f"k_hop_chain_gcn<{steps_}>")]
                if hit:
                    mb = e_ * 8 + n_ * (4 * 4 * f + 4)
                    per_kernel[hit[0][0]] = {"branch": tag, "kernel_only_us": hit[0][1]["avg_us"], "min_bytes_per_launch": mb,
                                             "frac_of_min_bytes": round(mb / hit[0][1]["avg_us"] / 1e3 / HBM_PEAK_GBS, 4)}
        out["roofline"] = {
            "bound": "hbm",
            "kernel": ("dc::k_hop_chain_gcn<8> / <6> (dc_hop_chain_f32: the 3 F=256 hops of a chain + row maxima as ONE "
                       "launch, every graph's 32-column slice and adjacency tables resident in LDS; forward and transposed "
                       "chain of both branches)")
            if chained else
            ("dc::k_spmm_wave<4,8,true> (F=256 hop + row maxima, as launched in a step" +
             (": ONE launch for both branches over the merged adjacency)" if merged else ")")),
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_note,
            "frac_definition": "frac = bytes a launch MOVES (moved_bytes_per_launch: " + moved_src + ") / kernel-only average "
                               "duration (" + ("kernel_only_avg_launch_us" if ko_avg_us is not None else
                                               "NOT measured in this run - avg_launch_us, HIP events with launch gaps, used instead") +
                               ") / 8 TB/s; frac_work_equivalent_per_hop_compulsory = per-hop compulsory bytes of the hop units "
                               "a launch performs (SURVEY.md 8(d) strict lower bound x 3 hops) / avg_launch_us / 8 TB/s - the "
                               "`frac` of rounds 2 - 5: it credits the fused launch with bytes it never moves",
            "moved_bytes_per_launch": int(moved), "moved_bytes_source": moved_src,
            "kernel_only_avg_launch_us": round(ko_avg_us, 2) if ko_avg_us is not None else None,
            "kernel_only_us": hop_ko or None, "kernel_only_source": kernel_only_note,
            "per_kernel": per_kernel or None,
            "launches_per_step": nlaunch, "hops_per_launch": nhops // nlaunch,
            "avg_launch_us": round(tot_ms / nlaunch * 1e3, 2),
            "avg_us_per_hop": round(tot_ms / nhops * 1e3, 2),
            "frac_live_hip_events": round(moved / (tot_ms / nlaunch * 1e3) / 1e3 / HBM_PEAK_GBS, 4),
            "frac_work_equivalent_per_hop_compulsory": round(work_equiv / HBM_PEAK_GBS, 4),
            "work_equivalent_GBps": round(work_equiv, 1),
            "compulsory_bytes_per_launch": int(comp_bytes / nlaunch),
            "bytes_model_work_equivalent": "compulsory bytes PER HOP, E*8 + N*(2*4F + 4) (each index / weight once, each feature "
                                           "row in once and out once; SURVEY.md 8(d) strict lower bound), times the hops a launch performs",
            "frac_of_measured_copy_peak_6290GBps": round(achieved / 6290.0, 4),
            "l2_lds_served": {"GBps": round(gath_bytes / tot_ms / 1e6, 1), "bytes_per_launch": int(gath_bytes / nlaunch),
                              "note": "SURVEY.md 8(d) gather model (every neighbour row counted per edge) / avg_launch_us; the "
                                      "chain kernel serves these reads from LDS, the per-hop kernel from L2 - NOT an HBM fraction"},
            "measured": f"avg_launch_us: the {nlaunch} launches that perform the {nhops} F=256 hops of a step, in step order on "
                        "step-shaped slabs (forward chain and transposed chain" + (" over the merged adjacency" if merged else "s of both branches") +
                        "), replayed from a hipGraph as the step is (no host launch cost), HIP events on the launch "
                        "stream, launch gaps included; kernel_only_*: see kernel_only_source",
            "cases_isolated": per_case,
            "cases_isolated_kernel": "dc::k_spmm_wave<4,8,true>, ONE hop per launch (ops.hop), the same launch back to back",
        }
        if chained:
            out["roofline"]["fused_chain_min_bytes_per_launch"] = int(fused_min / nlaunch)
            out["roofline"]["counter_over_min_traffic_ratio"] = round(traffic / (fused_min / nlaunch), 3) if traffic else None
            # and the same hops hop by hop (the r01-r03 kernel), same slabs, same method
            keep_chain = ops.HOP_CHAIN
            ops.HOP_CHAIN = False
            try:
                fn1, nl1, comp1, _ = pmc_hop.hop_sequence(dev, parts, merged, f, segments=seg_list)
                t1 = graph_time(fn1, nl1, calls=5) * nl1
                out["roofline"]["hop_by_hop"] = {"kernel": "dc::k_spmm_wave<4,8,true>", "launches_per_step": nl1,
                                                 "avg_launch_us": round(t1 / nl1 * 1e3, 2),
                                                 "frac": round(comp1 / t1 / 1e6 / HBM_PEAK_GBS, 4)}
            finally:
                ops.HOP_CHAIN = keep_chain
        gs, gr = GraphIndex(rest.edge_index, n_s), GraphIndex(rig.edge_index, n_r)
        if merged and ops.DENSE_SPLIT_BF16 and ops.DENSE_F16X2:
            out["roofline_mfma"] = dense_roofline_grouped(dev, parts, args.kernel_reps // 4 or 1)
        else:
            out["roofline_mfma"] = dense_roofline(dev, n_s, n_r, args.kernel_reps // 4 or 1, graphs=(gs, gr))
        if kernel_only:
            ko = {k: v for k, v in kernel_only.items() if "k_fwd_h2d" in k or "k_dw_h2w" in k or "k_fwd_h2w" in k}
            # the six layer-2 launches of a (one-stream) step: forward + dX of each branch on k_fwd_h2d, dW on k_dw_h2w
            calls = sum(v["calls"] for v in ko.values())
            if ko and calls:
                per_step = calls / 6.0                     # steps the child pass traced (6 such launches per step)
                t6 = sum(v["calls"] * v["avg_us"] for v in ko.values()) / per_step
                fl = out["roofline_mfma"].get("algorithmic_flop_per_step_l2")
                out["roofline_mfma"]["kernel_only_us"] = ko
                out["roofline_mfma"]["kernel_only_us_per_6_launches"] = round(t6, 1)
                if fl:
                    out["roofline_mfma"]["frac_kernel_only"] = round(3 * fl / t6 / 1e6 / 2500.0, 4)
                out["roofline_mfma"]["kernel_only_source"] = kernel_only_note
        if world == 1 and not args.no_strict_fp32:
            # auditable line: the headline step with every dense block on the fp32 matrix cores
            # (v_mfma_f32_32x32x2_f32, exact fp32 products) instead of the split fp16 / bf16 forms
            keep = ops.DENSE_SPLIT_BF16
            ops.DENSE_SPLIT_BF16 = False
            try:
                k = max(5, args.steps // 2)
                el = timed(make_mode("serial"), k, 3)
                out["strict_fp32"] = {"value": round(edges_per_rank * k / el / 1e6, 3), "unit": "M edges/s",
                                      "ms_per_step": round(el / k * 1e3, 4), "steps": k,
                                      "dense_arithmetic": "fp32 MFMA (v_mfma_f32_32x32x2_f32), DC_DENSE_SPLIT=0"}
            finally:
                ops.DENSE_SPLIT_BF16 = keep
        if world == 1 and not args.no_dropin:
            # the drop-in surface north_star names.  The SAME step (new batch copy + adjacency build +
            # fwd + bwd + Adam, one hipGraph) with the encoder wired the way the reference wires it - plain
            # `F.relu(conv(x, graph.edge_index))` + `F.dropout` calls, branch after branch on one stream
            # (graphnet.ReferenceWiring = models/model.py:69-78), batches from `Batch.from_data_list(...).to(dev)`
            # (train.py:36-46), same parameters - beside the headline's ContactEncoder (two streams) and the same
            # ContactEncoder held to one stream.
            from deformcontact_amd.graphnet import ReferenceWiring
            wiring = ReferenceWiring([21, 25], 256)
            wiring.conv_layers_resting, wiring.conv_layers_rigid = enc.conv_layers_resting, enc.conv_layers_rigid
            k = max(5, args.steps)
            from deformcontact_amd.nn import conv as conv_mod
            el_w2 = None
            try:
                model_box[0] = wiring
                el_w = timed(make_mode("serial"), k, 3)
                if not args.serial_branches:
                    # opt-in nn.conv.BRANCH_STREAMS: the wiring's two loops on two HIP streams (contract: conv.py)
                    conv_mod.BRANCH_STREAMS = True
                    try:
                        el_w2 = timed(make_mode("serial"), k, 3)
                    finally:
                        conv_mod.BRANCH_STREAMS = False
                model_box[0] = enc
                enc.overlap_branches = False
                el_1 = timed(make_mode("serial"), k, 3)
            finally:
                model_box[0] = enc
                enc.overlap_branches = not args.serial_branches
            out["dropin_reference_wiring"] = {
                "value": round(edges_per_rank * k / el_w / 1e6, 3), "unit": "M edges/s",
                "ms_per_step": round(el_w / k * 1e3, 4), "steps": k,
                "ratio_to_headline": round((el_w / k * 1e3) / ms_per_step, 4),
                "contact_encoder_one_stream": {"value": round(edges_per_rank * k / el_1 / 1e6, 3),
                                               "ms_per_step": round(el_1 / k * 1e3, 4)},
                "ratio_to_contact_encoder_one_stream": round(el_w / el_1, 4),
                "branch_streams_opt_in": None if el_w2 is None else {
                    "value": round(edges_per_rank * k / el_w2 / 1e6, 3), "ms_per_step": round(el_w2 / k * 1e3, 4),
                    "ratio_to_headline": round((el_w2 / k * 1e3) / ms_per_step, 4),
                    "note": "nn.conv.BRANCH_STREAMS = True (DC_BRANCH_STREAMS=1; off by default): the same wiring, the rigid "
                            "loop's launches on a side stream that waits for the start of the pass - needs every branch's "
                            "inputs complete when the pass's first conv is called (true of a model whose forward receives its "
                            "graphs as arguments)"},
                "wiring": "graphnet.ReferenceWiring: the encoder loops as /root/reference/models/model.py:69-78 writes "
                          "them (F.relu(conv(x, graph.edge_index)), F.dropout; resting branch, then rigid branch, caller's "
                          "stream) on Batch.from_data_list(...).to(dev) batches; the batch layout travels on the "
                          "edge_index tensor, the ReLU is fused by deferred, layer 1's output lands in layer 2's hop slab "
                          "(TAGConv._note_consumer): the launch set of ContactEncoder (tests/test_dropin.py asserts it, and "
                          "bit-identity); what the headline has on top is the second stream",
            }
        if world == 1 and not args.no_merged and not merged and ops.DENSE_SPLIT_BF16 and ops.DENSE_F16X2:
            # the OTHER encoder path, same step definition: both branches as one block-diagonal problem (one merged
            # adjacency, 6 instead of 12 F=256 hop launches, grouped dense launches; DC_MERGE_BRANCHES=1).  Same bits
            # out; measured slower than two overlapped per-branch streams, hence opt-in - numbers kept side by side.
            was_merged, enc.merge_branches = enc.merge_branches, True
            try:
                if enc._mergeable(rest.x, rig.x):
                    k = max(5, args.steps // 2)
                    el = timed(make_mode("serial"), k, 3)
                    fn_m, nl_m, comp_m, _ = pmc_hop.hop_sequence(dev, parts, True, f)
                    t_m = graph_time(fn_m, nl_m, calls=5) * nl_m
                    mf = dense_roofline_grouped(dev, parts, args.kernel_reps // 4 or 1)
                    out["merged_branches"] = {
                        "value": round(edges_per_rank * k / el / 1e6, 3), "unit": "M edges/s",
                        "ms_per_step": round(el / k * 1e3, 4), "steps": k,
                        "hop": {"launches_per_step": nl_m, "avg_launch_us": round(t_m / nl_m * 1e3, 2),
                                "compulsory_bytes_per_launch": int(comp_m / nl_m),
                                "frac_of_8TBps": round(comp_m / t_m / 1e6 / HBM_PEAK_GBS, 4)},
                        "dense_grouped": {"frac_of_2500_TF": mf["frac"], "in_sequence_us": mf["in_sequence_us"]},
                        "note": "ContactEncoder.merge_branches = True: one dc_graph_build_parts, first layers over "
                                "row windows, layer 2 of both branches as single launches; outputs and gradients "
                                "bit-identical to the default path (tests/test_merged.py)"}
            finally:
                enc.merge_branches = was_merged
        if world == 1 and not args.no_backbones:
            out["other_backbones"] = {}
            for bb in ("GCNConv", "GATConv"):
                try:
                    out["other_backbones"][bb] = backbone_extra(dev, rest, rig, bb)
                except Exception as e:  # pragma: no cover
                    out["other_backbones"][bb] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and not args.no_radius100k:
            try:
                out["radius100k"] = radius100k(dev, args.kernel_reps // 3 or 3)
            except Exception as e:  # pragma: no cover
                out["radius100k"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and not args.no_full_step:
            try:
                out["train_loop_b4"] = train_loop(dev)
            except Exception as e:  # pragma: no cover
                out["train_loop_b4"] = {"error": f"{type(e).__name__}: {e}"}
            out["full_train_step_b4"] = full_step_b4(dev)
            out["full_train_step_b32"] = full_step_b4(dev, steps=5, batch=32)
            try:
                out["full_forward_b32"] = full_forward(dev, 32)
            except Exception as e:  # pragma: no cover
                out["full_forward_b32"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.batch, args.cpu_seconds, all_cores=args.cpu_all_cores)
    if rank == 0:
        print(json.dumps(out), flush=True)

    phase("result line printed" if rank == 0 else "waiting for rank 0's kernel-level measurements")
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    phase("done")


if __name__ == "__main__":
    main()
