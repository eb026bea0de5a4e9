"""The per-edge C entries of dc_gat.hip called directly - ``dc_gat_edge_softmax_fwd`` / ``_bwd``, ``dc_sddmm_f32``,
``dc_segment_sum_f32``, ``dc_gather_f32``, ``dc_compose_perm`` - against float64 restatements of the same formulas
(PyG gat_conv.py ``edge_update``, utils/_softmax.py), compared PER EDGE with a per-segment metric, at the segment
lengths, widths, alignments and logit magnitudes where the kernels change form; then ``GATConv`` / ``GCNConv`` at the
output widths that take those forms.

The restatements are numpy, a few lines each, parametrised by dtype: float32 is the ``ref32`` of
``helpers.assert_parity``, float64 its ``truth64``.  ``test_references_on_the_cpu`` checks them (against
``oracle.pyg_ref`` in double and torch autograd) and the conditioning of the chosen inputs where there is no GPU.

Input choices that come from conditioning, not from what the kernels give:

* logits up to scale 30 and a 5,000-edge hub: the float32 restatement stays within 3e-6 of float64 (per segment);
* softmax backward, ``ge_p = alpha_p (galpha_p - dot)``: ``galpha_p - dot`` is a difference of numbers of order 1,
  formed to ~2^-24, while every ge of a segment can be arbitrarily smaller - (a) when the upstream gradients of a short
  segment nearly coincide, (b) when the weight sits on one edge (alpha_1 -> 1: every ge of the segment carries the
  factor ``1 - alpha_1``).  No fp32 evaluation is then within 1e-5 per segment.  So (a) ``galpha`` alternates in sign
  along a segment with magnitudes in [1, 2) (``galpha_for``), and (b) value parity of ``ge`` is asked where the logits
  of a segment spread over a few units at most (scales 0.1 and 1, equal logits, all negative, slope 0) - at scales 8
  and 30 and with a dominant edge the backward is checked structurally only;
* ``g_a_dst[i] = sum_seg ge`` is mathematically zero when the logits of a segment share a sign, so its VALUE is compared
  where they do not (scales 0.1, 1, slope 0); everywhere it is held to the rounding bound of an fp32 sum of the ge;
* SDDMM operands are of one sign per row (|g_ij|, h_ij in [0.5, 1.5], rows of g times +-logspace(-3, 3)): a dot product
  of mixed-sign terms can cancel to nothing in a one-edge segment, and then no fp32 evaluation is within 1e-5 of it.
"""
import copy

import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache, current_stream_ptr
from oracle import pyg_ref
from oracle.weights import fill_state_dict_, hashed_uniform
from tests.helpers import assert_parity, record_parity, rel_err, row_rel_err

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SLOPE = 0.2
LENS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)
HUB = 5000
ZERO_SPECIAL = ("mathematically zero: rounding noise; bar 3 x the fp32 restatement's distance from float64")


# --------------------------------------------------------------------------- #
# graphs with prescribed segment lengths
# --------------------------------------------------------------------------- #
def seg_lens(n, hub=HUB):
    """``lens[i]`` = in-edges of destination i INCLUDING its self loop: LENS cyclically, one hub."""
    lens = np.array([LENS[i % len(LENS)] for i in range(n)], dtype=np.int64)
    if n > 1:
        lens[n // 2] = hub
    else:
        lens[:] = 1                                         # a single node has its self loop and nothing else
    return lens


def seg_graph(lens, seed):
    """``edge_index`` [2, E] (shuffled) in which destination i has ``lens[i] - 1`` in-edges from other nodes
    (duplicates allowed) - with ``GraphIndex(..., self_loops=True)`` its segment has exactly ``lens[i]`` entries."""
    n = len(lens)
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(n), lens - 1)
    src = (dst + rng.integers(1, max(n, 2), dst.size)) % max(n, 1) if n > 1 else dst
    assert not (src == dst).any()
    order = rng.permutation(dst.size)
    return np.stack([src[order], dst[order]]).astype(np.int64)


def seg_of(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def seg_rel_err_on(ptr):
    """max over segments of  max_p |a_p - b_p| / max_p |b_p|  (a segment whose reference is all zero is compared
    against the global scale) - ``helpers.row_rel_err`` for ragged rows."""
    seg, n = seg_of(ptr), len(ptr) - 1

    def seg_rel_err(a, b):
        a, b = np.asarray(a, np.float64)[:len(seg)], np.asarray(b, np.float64)[:len(seg)]
        if a.size == 0:
            return 0.0
        scale, diff = np.zeros(n), np.zeros(n)
        np.maximum.at(scale, seg, np.abs(b))
        np.maximum.at(diff, seg, np.abs(a - b))
        scale = np.where(scale > 0, scale, max(np.abs(b).max(), 1e-30))
        return float((diff / scale).max())
    return seg_rel_err


# --------------------------------------------------------------------------- #
# the restatements (dt = np.float32: ref32, np.float64: truth64)
# --------------------------------------------------------------------------- #
def _seg_sum(v, seg, n):
    """per-segment sums in v's dtype, each by numpy's pairwise ``sum`` (a running fp32 sum over a 5,000-edge hub of
    near-equal terms drifts by more than the bar all by itself)"""
    ptr = np.searchsorted(seg, np.arange(n + 1))
    return np.array([v[ptr[i]:ptr[i + 1]].sum(dtype=v.dtype) for i in range(n)], dtype=v.dtype)


def galpha_for(ptr, seed):
    """upstream gradient per edge: magnitude in [1, 2), sign alternating along the segment - neighbours in a segment
    differ by 2 at least, so ``galpha_p - dot`` does not cancel in the short segments (module docstring)"""
    pos = np.arange(ptr[-1]) - ptr[:-1][seg_of(ptr)]
    mag = 1.0 + np.random.default_rng(seed).random(int(ptr[-1]))
    return (mag * np.where(pos % 2 == 0, 1.0, -1.0)).astype(np.float32)


def ref_logits(ptr, other, a_src, a_dst, dt):
    return a_src.astype(dt)[other] + a_dst.astype(dt)[seg_of(ptr)]


def ref_softmax_fwd(ptr, other, a_src, a_dst, slope, dt):
    """alpha_p = softmax over the segment of leaky_relu(a_src[other[p]] + a_dst[i]), denominator + 1e-16."""
    seg, n = seg_of(ptr), len(ptr) - 1
    s = ref_logits(ptr, other, a_src, a_dst, dt)
    e = np.where(s > 0, s, dt(np.float32(slope)) * s)
    m = np.full(n, -np.inf, dt)
    np.maximum.at(m, seg, e)
    ex = np.exp(e - m[seg])
    return ex / (_seg_sum(ex, seg, n) + dt(1e-16))[seg]


def ref_softmax_bwd(ptr, other, a_src, a_dst, slope, alpha, galpha, dt):
    """ge_p = alpha_p (galpha_p - sum_seg alpha galpha) * (s > 0 ? 1 : slope);  g_a_dst[i] = sum_seg ge."""
    seg, n = seg_of(ptr), len(ptr) - 1
    s = ref_logits(ptr, other, a_src, a_dst, dt)
    al, ga = alpha.astype(dt), galpha.astype(dt)
    dot = _seg_sum(al * ga, seg, n)
    ge = al * (ga - dot[seg]) * np.where(s > 0, dt(1), dt(np.float32(slope)))
    return ge, _seg_sum(ge, seg, n)


def ref_sddmm(ptr, other, g, h, dt):
    """d_p = <g[i, :], h[other[p], :]>"""
    return np.einsum("pf,pf->p", g.astype(dt)[seg_of(ptr)], h.astype(dt)[other])


def logits_case(case, ptr, other, seed):
    """(a_src, a_dst, slope) of a named logit regime on the given adjacency."""
    n = len(ptr) - 1
    rng = np.random.default_rng(seed)
    slope = SLOPE
    if case.startswith("normal"):
        k = float(case[len("normal"):])
        a_src, a_dst = rng.standard_normal(n) * k, rng.standard_normal(n) * k
    elif case == "equal":                                   # uniform weights: 1 / len up to rounding
        a_src, a_dst = np.full(n, 0.75), rng.standard_normal(n)
    elif case == "dominant":                                # sources 12 apart: each segment's top source takes all but
        a_src, a_dst = 12.0 * (1 + rng.permutation(n)), rng.random(n)   # e^-12 of the weight (near one-hot)
    elif case == "negative":                                # the slope branch on every edge
        a_src, a_dst = -1.0 - rng.random(n) * 8, -1.0 - rng.random(n) * 8
    elif case == "slope0":
        a_src, a_dst, slope = rng.standard_normal(n) * 0.5, rng.standard_normal(n) * 0.5, 0.0
    else:
        raise KeyError(case)
    return a_src.astype(np.float32), a_dst.astype(np.float32), slope


def top_source_weight(ptr, other, a_src, alpha):
    """per segment: the weight on the edges from its highest-logit source (duplicate edges share it)"""
    seg, n = seg_of(ptr), len(ptr) - 1
    top = np.full(n, -np.inf)
    np.maximum.at(top, seg, a_src[other].astype(np.float64))
    return _seg_sum(np.where(a_src[other] == top[seg], alpha, 0).astype(np.float64), seg, n)


LOGIT_CASES = ["normal0.1", "normal1", "normal8", "normal30", "equal", "dominant", "negative", "slope0"]
#: value parity of ge (module docstring): where the backward is well conditioned
BWD_CASES = ["normal0.1", "normal1", "equal", "negative", "slope0"]
#: value parity of g_a_dst: where a segment's logits have both signs (with one sign sum_seg ge is mathematically zero)
GD_CASES = ["normal0.1", "normal1", "slope0"]


def host_adjacency(lens, seed):
    """(ptr, other) by destination as the device build orders it for the softmax: stable by destination, the self
    loop included - the ORDER inside a segment does not enter any per-edge quantity the CPU test looks at."""
    n = len(lens)
    ei = seg_graph(lens, seed)
    src = np.concatenate([ei[0], np.arange(n)])
    dst = np.concatenate([ei[1], np.arange(n)])
    order = np.argsort(dst, kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=ptr[1:])
    assert np.array_equal(np.diff(ptr), lens)
    return ptr, src[order], dst[order]


# --------------------------------------------------------------------------- #
# CPU: the references against oracle.pyg_ref (double) and torch autograd; the conditioning of the inputs
# --------------------------------------------------------------------------- #
def test_references_on_the_cpu():
    lens = seg_lens(257)
    ptr, other, dst = host_adjacency(lens, 5)
    seg_err = seg_rel_err_on(ptr)
    worst_fwd, worst_bwd = 0.0, 0.0
    for k, case in enumerate(LOGIT_CASES):
        a_src, a_dst, slope = logits_case(case, ptr, other, 100 + k)
        a64 = ref_softmax_fwd(ptr, other, a_src, a_dst, slope, np.float64)
        a32 = ref_softmax_fwd(ptr, other, a_src, a_dst, slope, np.float32)
        assert a32.dtype == np.float32
        # the float64 restatement IS oracle.pyg_ref's softmax in double, and differentiates as torch does
        ts = torch.from_numpy(a_src).double().requires_grad_(True)
        td = torch.from_numpy(a_dst).double().requires_grad_(True)
        s = ts[torch.from_numpy(other)] + td[torch.from_numpy(dst)]
        want = pyg_ref.segment_softmax(torch.nn.functional.leaky_relu(s, float(np.float32(slope))),
                                       torch.from_numpy(dst), len(lens))
        assert seg_err(a64, want.detach().numpy()) < 1e-12, case
        galpha = galpha_for(ptr, 7 + k)
        s.retain_grad()
        (want * torch.from_numpy(galpha).double()).sum().backward()
        ge64, gd64 = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, a64, galpha, np.float64)
        assert rel_err(ge64, s.grad.numpy()) < 1e-12, case
        if case in BWD_CASES:                               # (elsewhere float64 itself loses digits per segment)
            assert seg_err(ge64, s.grad.numpy()) < 1e-9, case
        if case in GD_CASES:
            assert rel_err(gd64, td.grad.numpy()) < 1e-9, case
        # conditioning: what fp32 alone costs on these inputs
        worst_fwd = max(worst_fwd, seg_err(a32, a64))
        if case in BWD_CASES:
            ge32, _ = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, a32, galpha, np.float32)
            ge64, _ = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, a32, galpha, np.float64)
            worst_bwd = max(worst_bwd, seg_err(ge32, ge64))
        if case == "equal":
            assert np.abs(a64 * lens[dst] - 1).max() < 1e-12
        if case == "dominant":
            assert (top_source_weight(ptr, other, a_src, a64) > 0.9999).all()
        if case == "negative":
            assert (ref_logits(ptr, other, a_src, a_dst, np.float64) < 0).all()
    assert worst_fwd < 0.5 * TOL, worst_fwd                 # the chosen logits leave fp32 half the bar and more
    assert worst_bwd < 0.5 * TOL, worst_bwd
    # SDDMM: the restatement against a loop; one-signed rows keep fp32 far inside the bar at the widest width
    g, h = sddmm_operands(len(lens), 1024, 3)
    d64 = ref_sddmm(ptr, other, g, h, np.float64)
    for p in (0, 17, len(other) - 1):
        assert abs(d64[p] - float(np.dot(g[dst[p]].astype(np.float64), h[other[p]].astype(np.float64)))) <= 1e-12 * abs(d64[p])
    assert seg_err(ref_sddmm(ptr, other, g, h, np.float32), d64) < 0.5 * TOL
    # the metric itself: one wrong tail element of one segment is seen at its own scale
    bad = a64.copy()
    p = ptr[3] + lens[3] - 1
    bad[p] *= 1.001
    assert seg_err(bad, a64) > 1e-4 * a64[p] / a64[ptr[3]:ptr[4]].max() > 0


def sddmm_operands(n, f, seed, pad=8):
    """(g, h) [n, f] float32: |entries| in [0.5, 1.5], one sign per row of g, rows of g times logspace(-3, 3)."""
    rng = np.random.default_rng(seed)
    rows = np.logspace(-3, 3, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = (0.5 + rng.random((n, f))) * rows[:, None]
    h = 0.5 + rng.random((n, f))
    return g.astype(np.float32), h.astype(np.float32)


# --------------------------------------------------------------------------- #
# GPU
# --------------------------------------------------------------------------- #
def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _st():
    return current_stream_ptr(torch.device(DEV))


def device_graph(n, seed, hub=HUB):
    lens = seg_lens(n, hub)
    ei = torch.from_numpy(seg_graph(lens, seed)).to(DEV)
    g = GraphIndex(ei, n, self_loops=True, normalize=False, validate=True)
    ptr = _np(g.fwd.ptr).astype(np.int64)
    assert np.array_equal(np.diff(ptr), lens), "the build did not give the prescribed segment lengths"
    other = _np(g.fwd.other).astype(np.int64)[:ptr[-1]]
    return g, ptr, other, lens


def run_softmax_fwd(ptr_t, other_t, a_src, a_dst, slope, n, cap, fill=0.0):
    alpha = torch.full((max(cap, 1),), fill, dtype=torch.float32, device=DEV)
    rc = _lib.lib().dc_gat_edge_softmax_fwd(ptr_t.data_ptr(), other_t.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(),
                                            slope, alpha.data_ptr(), n, _st())
    _lib.check(rc, "dc_gat_edge_softmax_fwd")
    return alpha


def run_softmax_bwd(ptr_t, other_t, a_src, a_dst, slope, alpha, galpha, n, fill=0.0):
    ge = torch.full_like(alpha, fill)
    g_a_dst = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    rc = _lib.lib().dc_gat_edge_softmax_bwd(ptr_t.data_ptr(), other_t.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(),
                                            slope, alpha.data_ptr(), galpha.data_ptr(), ge.data_ptr(),
                                            g_a_dst.data_ptr(), n, _st())
    _lib.check(rc, "dc_gat_edge_softmax_bwd")
    return ge, g_a_dst


def check_forward(tag, ptr, other, lens, a_src, a_dst, slope, alpha):
    e = int(ptr[-1])
    got = _np(alpha)[:e]
    seg_err = seg_rel_err_on(ptr)
    a32 = ref_softmax_fwd(ptr, other, a_src, a_dst, slope, np.float32)
    a64 = ref_softmax_fwd(ptr, other, a_src, a_dst, slope, np.float64)
    assert_parity(got, a32, a64, TOL, f"alpha {tag}", metric=seg_err)
    # invariants that need no reference
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), tag
    sums = _seg_sum(got.astype(np.float64), seg_of(ptr), len(lens))
    assert (np.abs(sums - 1)[lens > 0] <= lens[lens > 0] * 2.0 ** -23).all(), \
        (tag, float((np.abs(sums - 1) / np.maximum(lens, 1)).max() * 2 ** 23))
    return got


def check_g_a_dst(tag, ptr, ge, g_a_dst):
    """g_a_dst[i] is the fp32 sum of the segment's ge: within len * 2^-24 * sum |ge| of their exact sum (the
    textbook bound of any summation order).  Needs no reference - the sum itself cancels towards zero whenever the
    segment's logits share a sign, so it is not compared by value here."""
    seg, n = seg_of(ptr), len(ptr) - 1
    ge = ge[:len(seg)].astype(np.float64)
    exact, mass = _seg_sum(ge, seg, n), _seg_sum(np.abs(ge), seg, n)
    assert (np.abs(g_a_dst - exact) <= np.diff(ptr) * 2.0 ** -24 * mass).all(), tag


@gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4099])
def test_edge_softmax_segment_lengths(n):
    """Segment lengths 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65 and a 5,000-edge hub; N * 8 short of, equal to and past
    one 256-thread workgroup; forward + backward per edge, two runs bit-identical."""
    g, ptr, other, lens = device_graph(n, 40 + n)
    a_src, a_dst, slope = logits_case("normal1", ptr, other, n)
    ts, td = _dev(a_src), _dev(a_dst)
    alpha = run_softmax_fwd(g.fwd.ptr, g.fwd.other, ts, td, slope, n, g.capacity)
    check_forward(f"N={n}", ptr, other, lens, a_src, a_dst, slope, alpha)
    assert torch.equal(alpha, run_softmax_fwd(g.fwd.ptr, g.fwd.other, ts, td, slope, n, g.capacity))
    e = int(ptr[-1])
    galpha = galpha_for(ptr, n)
    tg = torch.zeros_like(alpha)
    tg[:e] = _dev(galpha)
    ge, gd = run_softmax_bwd(g.fwd.ptr, g.fwd.other, ts, td, slope, alpha, tg, n)
    a_gpu = _np(alpha)[:e]
    ge32, gd32 = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, a_gpu, galpha, np.float32)
    ge64, gd64 = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, a_gpu, galpha, np.float64)
    assert_parity(_np(ge)[:e], ge32, ge64, TOL, f"ge N={n}", metric=seg_rel_err_on(ptr))
    check_g_a_dst(f"N={n}", ptr, _np(ge), _np(gd))
    if n > 1:                                               # (N = 1: one edge, ge = g_a_dst = 0 exactly)
        assert_parity(_np(gd), gd32, gd64, TOL, f"g_a_dst N={n}")
    else:
        assert float(ge[0]) == 0.0 and float(gd[0]) == 0.0 and float(alpha[0]) == 1.0
    ge2, gd2 = run_softmax_bwd(g.fwd.ptr, g.fwd.other, ts, td, slope, alpha, tg, n)
    assert torch.equal(ge, ge2) and torch.equal(gd, gd2)


@gpu
def test_edge_softmax_empty_segments_write_nothing():
    """Hand-made ptr / other with empty segments at the front, in the middle, two in a row and at the end."""
    lens = np.array([0, 3, 0, 0, 9, 1, 0, 17, 8, 0], dtype=np.int64)
    n = len(lens)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(0)
    other = rng.integers(0, n, ptr[-1])
    a_src, a_dst = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    tp, to = _dev(ptr, torch.int32), _dev(other, torch.int32)
    ts, td = _dev(a_src), _dev(a_dst)
    e, pad = int(ptr[-1]), 5
    alpha = run_softmax_fwd(tp, to, ts, td, SLOPE, n, e + pad, fill=-3.0)
    assert (alpha[e:] == -3.0).all()                         # nothing past the last segment
    got = check_forward("empty segments", ptr, other, lens, a_src, a_dst, SLOPE, alpha)
    galpha = np.concatenate([galpha_for(ptr, 1), np.ones(pad, np.float32)])
    ge, gd = run_softmax_bwd(tp, to, ts, td, SLOPE, alpha, _dev(galpha), n, fill=-5.0)
    assert (ge[e:] == -5.0).all()
    assert (_np(gd)[lens == 0] == 0.0).all() and not np.signbit(_np(gd)[lens == 0]).any()
    ge32, gd32 = ref_softmax_bwd(ptr, other, a_src, a_dst, SLOPE, got, galpha[:e], np.float32)
    ge64, gd64 = ref_softmax_bwd(ptr, other, a_src, a_dst, SLOPE, got, galpha[:e], np.float64)
    assert_parity(_np(ge)[:e], ge32, ge64, TOL, "ge, empty segments", metric=seg_rel_err_on(ptr))
    assert_parity(_np(gd), gd32, gd64, TOL, "g_a_dst, empty segments")
    # an all-empty adjacency: no write at all
    zp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    alpha = run_softmax_fwd(zp, to, ts, td, SLOPE, n, 4, fill=-3.0)
    assert (alpha == -3.0).all()


@gpu
@pytest.mark.parametrize("case", LOGIT_CASES)
def test_edge_softmax_logit_regimes(case):
    n = 517                                                  # 517 * 8 = 16 workgroups + 40 threads
    g, ptr, other, lens = device_graph(n, 9)
    a_src, a_dst, slope = logits_case(case, ptr, other, 300 + LOGIT_CASES.index(case))
    ts, td = _dev(a_src), _dev(a_dst)
    alpha = run_softmax_fwd(g.fwd.ptr, g.fwd.other, ts, td, slope, n, g.capacity)
    got = check_forward(case, ptr, other, lens, a_src, a_dst, slope, alpha)
    seg, e = seg_of(ptr), int(ptr[-1])
    if case == "equal":
        assert (np.abs(got * lens[seg] - 1) <= 4 * 2.0 ** -24).all()
    if case == "dominant":
        assert (top_source_weight(ptr, other, a_src, got) > 0.9999).all()
    # backward: value parity where it is well conditioned (module docstring); the structural checks everywhere
    rng = np.random.default_rng(11)
    galpha = galpha_for(ptr, 11)
    tg = torch.zeros_like(alpha)
    tg[:e] = _dev(galpha)
    ge, gd = run_softmax_bwd(g.fwd.ptr, g.fwd.other, ts, td, slope, alpha, tg, n)
    assert torch.isfinite(ge).all() and torch.isfinite(gd).all()
    check_g_a_dst(case, ptr, _np(ge), _np(gd))
    seg_err = seg_rel_err_on(ptr)
    if case in BWD_CASES:
        ge32, gd32 = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, got, galpha, np.float32)
        ge64, gd64 = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, got, galpha, np.float64)
        assert_parity(_np(ge)[:e], ge32, ge64, TOL, f"ge {case}", metric=seg_err)
        if case in GD_CASES:
            assert_parity(_np(gd), gd32, gd64, TOL, f"g_a_dst {case}")
    if case == "slope0":
        s = ref_logits(ptr, other, a_src, a_dst, np.float32)
        assert (_np(ge)[:e][s <= 0] == 0.0).all() and (s <= 0).sum() > e // 4
    # galpha constant per segment: ge is mathematically zero
    const = rng.standard_normal(n).astype(np.float32)[seg]
    tg[:e] = _dev(const)
    ge, gd = run_softmax_bwd(g.fwd.ptr, g.fwd.other, ts, td, slope, alpha, tg, n)
    ge32, _ = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, got, const, np.float32)
    ge64, _ = ref_softmax_bwd(ptr, other, a_src, a_dst, slope, got, const, np.float64)
    # judged on the scale of what cancels: alpha_p |galpha_p| per edge (ge64 itself is only float64 noise)
    scale = got.astype(np.float64) * np.abs(const)
    e_h = float(np.abs(_np(ge)[:e] - ge64).max() / scale.max())
    e_o = float(np.abs(ge32 - ge64).max() / scale.max())
    # bar: 3 x what the fp32 restatement loses, and never below one fp32 ulp (2^-23) of the terms that cancel
    record_parity(f"ge, galpha constant per segment, {case}", e_h, True, e_h, e_o,
                  metric="max|ge - ge64| / max(alpha |galpha|)", special=ZERO_SPECIAL)
    assert e_h <= max(3 * e_o, 2.0 ** -23), (e_h, e_o)
    assert np.abs(_np(gd)).max() <= 2.0 ** -23 * HUB * np.abs(const).max()


SDDMM_WIDTHS = [1, 3, 4, 21, 32, 128, 129, 130, 131, 256, 512, 516, 520, 1024]


def run_sddmm(g, tg, th, f, cap):
    d = torch.full((max(cap, 1),), -9.0, dtype=torch.float32, device=DEV)
    _lib.kernel_trace(True)
    rc = _lib.lib().dc_sddmm_f32(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), tg.data_ptr(), tg.stride(0),
                                 th.data_ptr(), th.stride(0), d.data_ptr(), g.num_nodes, f, _st())
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    _lib.check(rc, "dc_sddmm_f32")
    forms = [k for k in counts if "k_sddmm" in k]
    assert len(forms) == 1 and counts[forms[0]] == 1, counts
    return d, ("vec4" if "<4>" in forms[0] else "scalar")


@gpu
@pytest.mark.parametrize("f", SDDMM_WIDTHS)
def test_sddmm_widths_forms_and_views(f):
    """k_sddmm<1> without / with its scalar tail (F > 128), k_sddmm<4> without / with its tail (F > 512); then the
    same operands as column windows of wider buffers and from a base one float off 16-byte alignment."""
    n = 131
    g, ptr, other, lens = device_graph(n, 77, hub=600)
    e = int(ptr[-1])
    seg_err = seg_rel_err_on(ptr)
    hg, hh = sddmm_operands(n, f, f)
    d32, d64 = ref_sddmm(ptr, other, hg, hh, np.float32), ref_sddmm(ptr, other, hg, hh, np.float64)
    results = {}

    def case(tag, tg, th, want_form):
        assert torch.equal(tg, _dev(hg)) and torch.equal(th, _dev(hh))
        d, form = run_sddmm(g, tg, th, f, g.capacity)
        assert form == want_form, (tag, form)
        assert (d[e:] == -9.0).all()
        assert_parity(_np(d)[:e], d32, d64, TOL, f"sddmm F={f} {tag}", metric=seg_err)
        results.setdefault(form, []).append(_np(d)[:e])

    aligned = "vec4" if f % 4 == 0 else "scalar"
    case("contiguous", _dev(hg), _dev(hh), aligned)
    # column windows of wider buffers: ldg, ldh > F, window starting at a multiple of four columns
    wide_g = torch.full((n, f + 12), 1e30, device=DEV)
    wide_h = torch.full((n, f + 8), -1e30, device=DEV)
    wide_g[:, 4:4 + f], wide_h[:, 8:8 + f] = _dev(hg), _dev(hh)
    case("ld > F", wide_g[:, 4:4 + f], wide_h[:, 8:8 + f], aligned)
    # odd leading dimension: scalar form whatever F is
    odd_g = torch.full((n, f + 5), 1e30, device=DEV)
    odd_g[:, :f] = _dev(hg)
    case("odd ldg", odd_g[:, :f], _dev(hh), "scalar" if (f + 5) % 4 else aligned)
    # base pointer one float past a 16-byte boundary, ld a multiple of 4: must select the scalar form
    off_h = torch.full((n, f + 4 - f % 4 + 4), -1e30, device=DEV)
    assert off_h.stride(0) % 4 == 0 and off_h.data_ptr() % 16 == 0
    off_h[:, 1:1 + f] = _dev(hh)
    case("h base + 1 float", _dev(hg), off_h[:, 1:1 + f], "scalar")
    off_g = torch.full((n, f + 4 - f % 4 + 4), 1e30, device=DEV)
    off_g[:, 1:1 + f] = _dev(hg)
    case("g base + 1 float", off_g[:, 1:1 + f], _dev(hh), "scalar")
    # every run of one form computes the same sums in the same order; the two forms agree within the bar
    for form, ds in results.items():
        for d in ds[1:]:
            assert np.array_equal(d, ds[0]), form
    if len(results) == 2:
        assert seg_err(results["vec4"][0], results["scalar"][0]) < TOL


@gpu
def test_gather_compose_with_device_count_and_segment_sum():
    L = _lib.lib()
    n = 517
    g, ptr, other, lens = device_graph(n, 21)
    e, cap = int(ptr[-1]), g.capacity
    assert g.capacity == e                                   # (no self loop in the input: nothing was dropped)
    rng = np.random.default_rng(2)
    v = rng.standard_normal(e).astype(np.float32)
    idx = rng.integers(0, e, e + 300)
    a = rng.integers(0, 1 << 30, e)
    tv, tidx, ta = _dev(v), _dev(idx, torch.int32), _dev(a, torch.int32)
    for count in (0, 1, 255, 256, 257, e - 1, e):
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        out = torch.full((e + 300,), -2.0, device=DEV)
        _lib.check(L.dc_gather_f32(tv.data_ptr(), tidx.data_ptr(), out.data_ptr(),
                                   cnt.data_ptr(), e + 300, _st()), "dc_gather_f32")
        assert np.array_equal(_np(out)[:count], v[idx[:count]]) and (out[count:] == -2.0).all(), count
        # cap < count: cap bounds the writes
        out = torch.full((e + 300,), -2.0, device=DEV)
        big = torch.tensor([e + 300], dtype=torch.int32, device=DEV)
        _lib.check(L.dc_gather_f32(tv.data_ptr(), tidx.data_ptr(), out.data_ptr(),
                                   big.data_ptr(), count, _st()), "dc_gather_f32")
        assert np.array_equal(_np(out)[:count], v[idx[:count]]) and (out[count:] == -2.0).all(), count
        oi = torch.full((e + 300,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L.dc_compose_perm(ta.data_ptr(), tidx.data_ptr(), oi.data_ptr(),
                                     cnt.data_ptr(), e + 300, _st()), "dc_compose_perm")
        assert np.array_equal(_np(oi)[:count], a[idx[:count]]) and (oi[count:] == -7).all(), count
    # bwd_to_fwd: the source-sorted edge q is the destination-sorted edge b2f[q]
    b2f = _np(g.bwd_to_fwd()).astype(np.int64)[:e]
    assert np.array_equal(np.sort(b2f), np.arange(e))
    assert np.array_equal(_np(g.fwd.perm)[:e][b2f], _np(g.bwd.perm)[:e])
    # segment sums: over the destination segments (no map), and per SOURCE through map = bwd_to_fwd
    out = torch.full((n,), 5.0, device=DEV)
    _lib.check(L.dc_segment_sum_f32(g.fwd.ptr.data_ptr(), None, tv.data_ptr(), out.data_ptr(), n, _st()),
               "dc_segment_sum_f32")
    seg = seg_of(ptr)
    assert_parity(_np(out), _seg_sum(v, seg, n), _seg_sum(v.astype(np.float64), seg, n), TOL, "segment sum, no map")
    mass = _seg_sum(np.abs(v).astype(np.float64), seg, n)
    assert (np.abs(_np(out) - _seg_sum(v.astype(np.float64), seg, n)) <= lens * 2.0 ** -24 * mass).all()
    out = torch.full((n,), 5.0, device=DEV)
    _lib.check(L.dc_segment_sum_f32(g.bwd.ptr.data_ptr(), g.bwd_to_fwd().data_ptr(), tv.data_ptr(), out.data_ptr(), n,
                                    _st()), "dc_segment_sum_f32")
    want64 = torch.zeros(n, dtype=torch.float64).index_add_(0, torch.from_numpy(other), torch.from_numpy(v).double())
    want32 = torch.zeros(n, dtype=torch.float32).index_add_(0, torch.from_numpy(other), torch.from_numpy(v))
    assert_parity(_np(out), want32.numpy(), want64.numpy(), TOL, "segment sum by source (map = bwd_to_fwd)")
    outdeg = np.bincount(other, minlength=n)
    mass = np.zeros(n)
    np.add.at(mass, other, np.abs(v).astype(np.float64))
    assert (np.abs(_np(out) - want64.numpy()) <= outdeg * 2.0 ** -24 * mass).all()


# --------------------------------------------------------------------------- #
# the layers at the widths that take each form
# --------------------------------------------------------------------------- #
ATT_SPECIAL = {"att_dst": "a gradient that is mathematically zero: rounding noise of the softmax backward; bar 3 x the "
                          "fp32 oracle's distance from float64",
               "att_src": "GAT attention vector: a sum of terms that cancel to ~1 % of their size; bar 3 x the fp32 "
                          "oracle's distance from float64"}


def _layer_graph():
    n = 300
    lens = seg_lens(n)
    return n, seg_graph(lens, 13)


@gpu
@pytest.mark.parametrize("fo,form", [(21, "<1>"), (30, "<1>"), (131, "<1>"), (516, "<4>"), (1024, "<4>")])
def test_gatconv_at_the_widths_of_each_sddmm_form(fo, form):
    """GATConv forward + backward: 21 / 30 unfused + scalar SDDMM, 131 its tail, 516 unfused + 16-byte form with
    tail, 1024 the fused layer - output, x.grad and lin.weight.grad PER ROW against oracle.pyg_ref (fp32, float64)."""
    torch.set_num_threads(1)
    fi = 25
    n, ei = _layer_graph()
    x = hashed_uniform((n, fi), 31, 2.0)
    gup = hashed_uniform((n, fo), 37, 2.0)
    cpu = pyg_ref.GATConv(fi, fo)
    fill_state_dict_(cpu, salt0=fo)
    gpu_conv = dc.nn.GATConv(fi, fo)
    gpu_conv.load_state_dict(cpu.state_dict())
    gpu_conv = gpu_conv.to(DEV)
    c64 = copy.deepcopy(cpu).double()
    xc = torch.from_numpy(x).requires_grad_(True)
    oc = cpu(xc, torch.from_numpy(ei))
    (oc * torch.from_numpy(gup)).sum().backward()
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    o64 = c64(x64, torch.from_numpy(ei))
    (o64 * torch.from_numpy(gup).double()).sum().backward()
    clear_cache()
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    _lib.kernel_trace(True)
    og = gpu_conv(xg, torch.from_numpy(ei).to(DEV))
    (og * torch.from_numpy(gup).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    ran = [k for k in counts if "k_sddmm" in k]
    assert len(ran) == 1 and form in ran[0], counts         # the route this case is here for
    for k in ("k_gat_softmax_fwd", "k_gat_softmax_bwd", "k_segment_sum", "k_gather"):
        assert any(k in name for name in counts), (k, counts)
    assert ops.fused_gnn_ok(torch.empty(1, fo, device=DEV)) == (fo == 1024)
    assert_parity(_np(og), _np(oc), _np(o64), TOL, f"GATConv {fo} forward per row", metric=row_rel_err)
    assert_parity(_np(xg.grad), _np(xc.grad), _np(x64.grad), TOL, f"GATConv {fo} x.grad per row", metric=row_rel_err)
    gc, g64 = dict(cpu.named_parameters()), dict(c64.named_parameters())
    for name, p in gpu_conv.named_parameters():
        got, r32, t64 = _np(p.grad), _np(gc[name].grad), _np(g64[name].grad)
        if name == "lin.weight":
            assert_parity(got, r32, t64, TOL, f"GATConv {fo} lin.weight.grad per output channel", metric=row_rel_err)
        elif name in ATT_SPECIAL:
            assert_parity(got, r32, t64, TOL, f"GATConv {fo} {name}", special=ATT_SPECIAL[name],
                          special_bound=lambda eo: 3 * eo)
        else:
            assert_parity(got, r32, t64, TOL, f"GATConv {fo} {name}")


@gpu
@pytest.mark.parametrize("fo", [21, 30, 131, 516, 1024])
def test_gcnconv_and_the_bias_act_aggregation_bitwise_at_the_same_widths(fo):
    """``dc_spmm_f32_bias_act`` in its scalar (21, 30, 131) and 16-byte (516, 1024) form, and the GCNConv layer,
    bitwise against ``relu(ops.hop(...) + bias)``."""
    fi = 25
    n, ei = _layer_graph()
    tei = torch.from_numpy(ei).to(DEV)
    g = GraphIndex(tei, n, self_loops=True)
    torch.manual_seed(fo)
    h, bias = torch.randn(n, fo, device=DEV), torch.randn(fo, device=DEV)
    ref = ops.hop(g.fwd, h)
    for b, relu in ((bias, True), (bias, False), (None, True), (None, False)):
        y = ops._agg_bias_act(g.fwd, g.fwd.w, h, b, relu)
        want = ref if b is None else ref + b
        want = torch.relu(want) if relu else want
        assert torch.equal(y, want), (b is not None, relu)
    # ... against float64 per row, so that "bitwise equal" is not two copies of one mistake
    ptr, other = _np(g.fwd.ptr).astype(np.int64), _np(g.fwd.other).astype(np.int64)
    w64 = _np(g.fwd.w).astype(np.float64)[:ptr[-1]]
    want64 = np.zeros((n, fo))
    np.add.at(want64, seg_of(ptr), w64[:, None] * _np(h).astype(np.float64)[other[:ptr[-1]]])
    assert row_rel_err(_np(ref), want64) < TOL
    clear_cache()
    conv = dc.nn.GCNConv(fi, fo).to(DEV)
    with torch.no_grad():
        conv.bias.uniform_(-0.3, 0.3)
    x = torch.randn(n, fi, device=DEV)
    for relu in (True, False):
        y = conv(x, tei, relu=relu)
        want = ops.hop(g.fwd, conv.lin(x)) + conv.bias
        assert torch.equal(ops.resolve(y), torch.relu(want) if relu else want), relu
