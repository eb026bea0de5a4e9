"""The first layers' forward block on PREPARED weights (dc_narrow_image.h, dc_dense_narrow.hip: `k_fwd_narrow_img`): the
bf16x3 fragment image of `[W_0 | ... | W_K | 0]` (lins[k].weight of PyG tag_conv.py; the first TAGConv of either branch,
models/model.py:44-50 of the reference) is written once per call - by the layer's pack + first-hop launch
(`dc_spmm_f32_pack_wprep`) or by `dc_tag_narrow_wimage` - and the block reads it instead of preparing the weights in every
workgroup.

* the image, record by record, against a torch restatement of `split1` (round-to-nearest-even bf16 of x, of x - hi, of
  x - hi - mid), from both launches, for contiguous weights and for views into a flat buffer at a 4-byte-odd offset;
* the forward block, bit for bit against the kernel that prepares its own weights (`dc_tag_linear_fwd_narrow`, what
  DC_NARROW_PREP=0 selects) and within the 2e-6 per row of float64 of tests/test_narrow_dense.py;
* the layer through `ops`: which launches prepare the image, and the same bits as with DC_NARROW_PREP=0 (a child process:
  the switch is read once)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, current_stream_ptr
from deformcontact_amd.ops import _ptr_array
from tests.helpers import random_multigraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FO = 256
STEP_BYTES = 3 * 8 * 64 * 16


def _planes(x: torch.Tensor):
    """split1 on the CPU: x = hi + mid + lo, each the nearest-even bf16 of what the ones before leave."""
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo])


def _expected_image(ws, wpad: int) -> np.ndarray:
    """[KS][3][8][64][8] int16: record (ks, plane, block, lane = c + 32 h) = plane of Wcat[32 block + c][16 ks + 8 h .. + 7]"""
    wcat = torch.zeros(FO, wpad)
    wcat[:, :sum(w.size(1) for w in ws)] = torch.cat([w.cpu() for w in ws], 1)
    p = _planes(wcat).view(3, 8, 32, wpad // 16, 2, 8)             # plane, block, c, ks, h, j
    img = p.permute(3, 0, 1, 4, 2, 5).contiguous()                 # ks, plane, block, h, c, j
    return img.view(torch.int16).numpy().reshape(wpad // 16, 3, 8, 64, 8)


def _weights(fi: int, nseg: int, form: str, gen):
    vals = [((torch.rand(FO, fi, generator=gen) * 2 - 1) / fi ** 0.5) for _ in range(nseg)]
    vals[0][0, 0], vals[-1][-1, -1] = 0.0, -1.0e-30                # a zero and a tiny number
    if form == "contiguous":
        return [v.to(DEV) for v in vals]
    flat = torch.zeros(1 + nseg * FO * fi, device=DEV)             # views at 4 bytes past a 16-byte boundary
    ws = []
    for s, v in enumerate(vals):
        w = flat[1 + s * FO * fi:1 + (s + 1) * FO * fi].view(FO, fi)
        w.copy_(v)
        assert w.data_ptr() % 16 == 4 and w.is_contiguous()
        ws.append(w)
    return ws


def _image_buffer(wpad: int) -> torch.Tensor:
    return torch.full((wpad // 16 * STEP_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)


def _check_image(buf: torch.Tensor, ws, fi: int, nseg: int, wpad: int):
    got = buf.cpu().numpy().view(np.int16).reshape(wpad // 16, 3, 8, 64, 8)
    want = _expected_image(ws, wpad)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # the K padding: columns k = 16 ks + 8 h + j >= nseg * fi are zero in every plane
    k = (16 * np.arange(wpad // 16)[:, None, None] + 8 * (np.arange(64) // 32)[None, :, None] + np.arange(8)[None, None, :])
    pad = np.broadcast_to((k >= nseg * fi)[:, None, None, :, :], got.shape)
    assert not got[pad].any()
    assert pad.sum() == 3 * FO * (wpad - nseg * fi)


SHAPES = [(21, 4, 96), (25, 4, 112), (32, 4, 128), (32, 3, 96), (24, 4, 96)]


@pytest.mark.parametrize("form", ["contiguous", "odd_offset_views"])
@pytest.mark.parametrize("fi,nseg,wpad", SHAPES)
def test_weight_image_from_its_own_kernel_bit_for_bit(fi, nseg, wpad, form):
    L = _lib.lib()
    ws = _weights(fi, nseg, form, torch.Generator().manual_seed(fi * nseg))
    buf = _image_buffer(wpad)
    _lib.check(L.dc_tag_narrow_wimage(_ptr_array(ws), nseg, fi, wpad, buf.data_ptr(), current_stream_ptr(torch.device(DEV))),
               "wimage")
    torch.cuda.synchronize()
    _check_image(buf, ws, fi, nseg, wpad)


@pytest.mark.parametrize("form", ["contiguous", "odd_offset_views"])
@pytest.mark.parametrize("fi,nseg,wpad", SHAPES)
def test_weight_image_from_the_pack_launch_bit_for_bit_and_the_slab_unchanged(fi, nseg, wpad, form):
    """`dc_spmm_f32_pack_wprep`: the image as above, and the slab (block 0, first hop, K padding) exactly what
    `dc_spmm_f32_pack` writes - 1,003 rows: 126 row blocks behind the image's workgroups, the last one ragged."""
    L = _lib.lib()
    n, e = 1003, 7001
    st = current_stream_ptr(torch.device(DEV))
    g = GraphIndex(torch.from_numpy(random_multigraph(n, e, fi)).to(DEV), n)
    adj = g.fwd
    ws = _weights(fi, nseg, form, torch.Generator().manual_seed(fi + nseg))
    torch.manual_seed(fi)
    x = torch.randn(n, fi, device=DEV)
    width = nseg * fi
    slabs = [torch.full((n, wpad + 8), float("nan"), device=DEV)[:, :wpad] for _ in range(2)]
    buf = _image_buffer(wpad)
    args = lambda slab: (adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), x.data_ptr(), x.stride(0),
                         slab.data_ptr(), slab.stride(0), n, fi, width, wpad)
    _lib.check(L.dc_spmm_f32_pack_wprep(*args(slabs[0]), _ptr_array(ws), nseg, buf.data_ptr(), st), "pack_wprep")
    _lib.check(L.dc_spmm_f32_pack(*args(slabs[1]), st), "pack")
    torch.cuda.synchronize()
    _check_image(buf, ws, fi, nseg, wpad)
    a, b = (s.cpu().numpy() for s in slabs)
    for cols in (slice(0, 2 * fi), slice(width, wpad)):            # (blocks 2.. are the later hops')
        assert np.array_equal(a[:, cols], b[:, cols])
    assert np.array_equal(a[:, :fi], x.cpu().numpy())


def _forward_case(n, fi, nseg, wpad, relu, bias_on, ldo_pad, gen):
    L = _lib.lib()
    dev = torch.device(DEV)
    st = current_stream_ptr(dev)
    slab = torch.zeros(n, wpad + 8, device=dev)[:, :wpad]                 # leading dimension != width
    slab[:, :nseg * fi] = ((torch.rand(n, nseg * fi, generator=gen) * 4 - 2) *
                           torch.logspace(-3, 0, n).unsqueeze(1)).to(dev)
    ws = [((torch.rand(FO, fi, generator=gen) * 2 - 1) / fi ** 0.5).to(dev) for _ in range(nseg)]
    bias = (torch.rand(FO, generator=gen) - 0.5).to(dev) if bias_on else None
    bp = bias.data_ptr() if bias_on else None
    buf = _image_buffer(wpad)
    _lib.check(L.dc_tag_narrow_wimage(_ptr_array(ws), nseg, fi, wpad, buf.data_ptr(), st), "wimage")
    base = torch.full((n, FO + ldo_pad), float("nan"), device=dev)       # the output as block 0 of a wider slab
    out = base[:, :FO]
    _lib.check(L.dc_tag_linear_fwd_narrow_img(slab.data_ptr(), slab.stride(0), buf.data_ptr(), bp, int(relu), out.data_ptr(),
                                              out.stride(0), n, wpad, FO, st), "narrow_img")
    ref = torch.empty(n, FO, device=dev)
    _lib.check(L.dc_tag_linear_fwd_narrow(slab.data_ptr(), slab.stride(0), _ptr_array(ws), nseg, fi, bp, int(relu),
                                          ref.data_ptr(), FO, n, wpad, FO, st), "narrow")
    torch.cuda.synchronize()
    assert torch.equal(out, ref), "not bit-identical to the kernel that prepares its own weights"
    if ldo_pad:
        assert torch.isnan(base[:, FO:]).all()                              # nothing written beside the output columns
    t = slab[:, :nseg * fi].double().cpu() @ torch.cat(ws, 1).double().cpu().t()
    if bias_on:
        t = t + bias.double().cpu()
    if relu:
        t = t.clamp_min(0)
    den = t.abs().amax(1, keepdim=True).clamp_min(1e-300)
    assert float(((out.double().cpu() - t).abs() / den).max()) < 2e-6


# 16,391 rows = 513 tiles of 32: the persistent loop wraps at two workgroups per CU (512); 1 / 31 / 32 / 33: a tile that is
# short, just short, whole, one row over
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 16391])
@pytest.mark.parametrize("fi,nseg,wpad", [(21, 4, 96), (25, 4, 112), (32, 4, 128)])
def test_forward_on_the_image_bit_identical_to_the_self_preparing_kernel_and_fp32_accurate(n, fi, nseg, wpad):
    gen = torch.Generator().manual_seed(n * 131 + fi)
    for relu, bias_on, ldo_pad in ((True, True, 0), (False, False, 0), (True, False, 832), (False, True, 64)):
        _forward_case(n, fi, nseg, wpad, relu, bias_on, ldo_pad, gen)


def test_forward_entries_reject_bad_arguments():
    L = _lib.lib()
    one = _ptr_array([torch.zeros(FO, 21, device=DEV)])
    assert L.dc_tag_narrow_wimage(one, 1, 21, 96, 24, None) == -1 and b"dc_tag_narrow_wimage" in L.dc_last_error()    # image % 16
    assert L.dc_tag_narrow_wimage(one, 5, 21, 112, 64, None) == -1                                                  # 5 * 21 > 112
    assert L.dc_tag_narrow_wimage(one, 1, 21, 80, 64, None) == -1                                                   # padded width
    assert L.dc_tag_linear_fwd_narrow_img(64, 96, 64, None, 0, 64, 256, 4, 96, 128, None) == -1                     # Fo
    assert L.dc_tag_linear_fwd_narrow_img(64, 96, None, None, 0, 64, 256, 4, 96, 256, None) == -1                   # no image
    assert L.dc_tag_linear_fwd_narrow_img(None, 96, None, None, 0, None, 256, 0, 96, 256, None) == 0                # no rows


def traced_on(conv, x, edge_index):
    _lib.kernel_trace(True)
    y = conv(x, edge_index, relu=True)
    torch.cuda.synchronize()
    _lib.kernel_trace(False)
    return y, _lib.kernel_trace_counts()


CHILD = r"""
import sys
import torch
sys.path.insert(0, %(root)r)
from deformcontact_amd import _lib, nn as dc_nn, ops, synth
assert ops.NARROW_PREP is False
rest, _, _ = synth.make_batch(2, soft_vertices=128, sphere_resolution=5)
rest = rest.to("cuda:0")
torch.manual_seed(0)
conv = dc_nn.TAGConv(21, 256).to("cuda:0")
_lib.kernel_trace(True)
y = conv(rest.x, rest.edge_index, relu=True)
torch.cuda.synchronize()
_lib.kernel_trace(False)
tr = _lib.kernel_trace_counts()
assert any(k.startswith("k_fwd_narrow<") for k in tr) and not any("wim" in k or "k_fwd_narrow_img" in k for k in tr), tr
torch.save(y.cpu(), sys.argv[1])
print("CHILD_OK")
"""


def test_layer_prepares_the_image_in_the_pack_launch_or_on_its_own_and_matches_narrow_prep_off(tmp_path):
    from deformcontact_amd import nn as dc_nn, synth
    rest, _, _ = synth.make_batch(2, soft_vertices=128, sphere_resolution=5)
    rest = rest.to(DEV)
    torch.manual_seed(0)
    conv = dc_nn.TAGConv(21, 256).to(DEV)

    def traced():
        return traced_on(conv, rest.x, rest.edge_index)

    # a new input: pack + first hop + image in one launch, no launch added
    y, tr = traced()
    assert sum(v for k, v in tr.items() if k.startswith("k_spmm_sub_wimg")) == 1, tr
    assert sum(v for k, v in tr.items() if k.startswith("k_spmm_sub")) == 3, tr
    assert sum(v for k, v in tr.items() if k.startswith("k_fwd_narrow_img")) == 1 and "k_narrow_wimage" not in tr, tr
    # the same input again: the hop slab is cached, the image gets a launch of its own
    y2, tr2 = traced()
    assert not any(k.startswith("k_spmm_sub") for k in tr2) and tr2.get("k_narrow_wimage") == 1, tr2
    assert sum(v for k, v in tr2.items() if k.startswith("k_fwd_narrow_img")) == 1, tr2
    assert torch.equal(y, y2)
    # no fused pack launch (DC_FUSED_PACK=0)
    keep, ops.FUSED_PACK = ops.FUSED_PACK, False
    try:
        y3, tr3 = traced_on(conv, rest.x.clone(), rest.edge_index)
    finally:
        ops.FUSED_PACK = keep
    assert tr3.get("k_narrow_wimage") == 1 and not any(k.startswith("k_spmm_sub_wimg") for k in tr3), tr3
    assert torch.equal(y, y3)
    # DC_NARROW_PREP=0: the self-preparing kernel, the same bits
    path = str(tmp_path / "y.pt")
    env = dict(os.environ, DC_NARROW_PREP="0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert torch.equal(y.cpu(), torch.load(path))

