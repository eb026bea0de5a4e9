"""Launch-site census: every kernel instantiation the library ships is launched by some test.

The library lists its own launch sites (`_lib.launch_sites()`, one per `DC_LAUNCH` and per instantiation of a templated
host launcher; host data, no GPU needed).  `tests/golden/launch_reach.json` is the measured record `{site: [tests that
first reached it]}` of the whole GPU suite (tools/launch_coverage.py; INTEGRATION.md, "Launch sites").

* The CPU tests here are the gate: the record lists exactly the library's sites, and every site has a reacher or an
  entry in `OPEN` with the predicate that guards it.
* The GPU cases close what the suite did not reach before this file existed (profiles/r12/launch_coverage_before.txt):
  one case per site at the smallest shape that its launcher's predicates send there, the site asserted from the launch
  log by name, every output compared with a float64 restatement on the CPU.

Dense shapes are read off the predicates in csrc/dc_dense.hip (BN = 128 columns, BK = 16, 64 * MB rows per tile):
  vec      all operands 16-byte aligned, leading dimensions % 4 == 0, Fi % 4 == 0 (dX, dW: and Fo % 4 == 0)
  fast     forward: vec and Fi % 16 == 0 and equal leading dimensions; dX: vec and Fo % 16 == 0; dW: vec and N % 16 == 0
  MB       forward / dX: 2 iff ceil(N / 128) * column tiles >= 512 (pick_mb); dW: 2 iff Fo >= 128 (dw_mb)
  ragged   dW with vec and N % 16 != 0 and N > 16: the last N % 16 rows go through the generic kernel on their own
The generic kernel runs when `fast` fails; its VEC argument is `vec`, its MASK argument is "out_for_mask given".
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, rel_err

DEV = "cuda"
REACH_JSON = os.path.join(GOLDEN, "launch_reach.json")

#: sites no test reaches, with the predicate that guards each and why it stayed open.  None may come from the
#: training path, at most MAX_OPEN from the other files.
OPEN = {}
TRAINING_PATH = ("dc_dense", "dc_spmm", "dc_hopchain", "dc_csr", "dc_loss", "dc_optim", "dc_attn", "dc_gnn_epi")
MAX_OPEN = 15


# --------------------------------------------------------------------------- #
# the gate (CPU)
# --------------------------------------------------------------------------- #
def _reach():
    with open(REACH_JSON) as f:
        return json.load(f)


def test_record_lists_exactly_the_librarys_sites():
    """A new or changed launch site forces a new measurement (tools/launch_coverage.py)."""
    from deformcontact_amd import _lib
    sites, rec = set(_lib.launch_sites()), set(_reach())
    assert sites == rec, {"not in the record": sorted(sites - rec), "no longer in the library": sorted(rec - sites)}


def test_site_list_is_per_instantiation():
    from deformcontact_amd import _lib
    sites = _lib.launch_sites()
    assert len(sites) == len(set(sites)) > 400
    narrow = [s for s in sites if s.startswith("k_fwd_narrow_img<KS, WPC> @ ")]
    assert len(narrow) >= 3 and any("[KS = 6, WPC = 2]" in s for s in narrow)
    chains = [s for s in sites if s.startswith("k_hop_chain<")]
    assert "k_hop_chain_gcn<3> @" in " ".join(sites) and len(chains) >= 8


def test_every_site_is_reached_or_open():
    rec = _reach()
    missing = sorted(s for s, tests in rec.items() if not tests and s not in OPEN)
    assert not missing, missing
    stale = sorted(s for s in OPEN if s not in rec or rec[s])
    assert not stale, ("OPEN names a site that is reached or no longer exists", stale)


def test_open_sites_are_few_and_off_the_training_path():
    from deformcontact_amd import _lib
    files = _lib.launch_site_files()
    assert len(OPEN) <= MAX_OPEN
    for site, reason in OPEN.items():
        assert reason.strip(), site
        assert not files[site].startswith(TRAINING_PATH), (site, files[site])


@pytest.mark.gpu
def test_coverage_is_cumulative_and_independent_of_the_launch_log():
    from deformcontact_amd import _lib, ops
    site = next(s for s in _lib.launch_sites() if s.startswith("k_rowabsmax @ "))
    x = torch.randn(7, 5, device=DEV)
    _lib.launch_coverage(True)
    try:
        assert torch.equal(ops.rowabsmax(x), x.abs().amax(1))
        reached, n0 = _lib.launch_reached(), _lib.launch_site_counts()[site]
        assert site in reached and set(reached) <= set(_lib.launch_sites()) and n0 >= 1
        assert "::test_" in reached[site]                          # whichever test reached it first
        _lib.kernel_trace(True)                                    # clears the launch log, not the reached set
        assert _lib.launch_reached() == reached and _lib.launch_site_counts()[site] == n0
        ops.rowabsmax(x)
        _lib.kernel_trace(False)
        assert _lib.kernel_trace_counts().get("k_rowabsmax") == 1
        ops.rowabsmax(x)                                           # coverage alone is on: the log stays as it is
        assert _lib.kernel_trace_counts().get("k_rowabsmax") == 1
        assert _lib.launch_reached() == reached                    # the first test stays on record
        assert _lib.launch_site_counts()[site] == n0 + 2
        _lib.launch_coverage(False)                                # off: a launch is no longer counted
        ops.rowabsmax(x)
        assert _lib.launch_site_counts()[site] == n0 + 2 and _lib.launch_reached() == reached
    finally:
        _lib.launch_coverage(_coverage_default())


# --------------------------------------------------------------------------- #
# dense block through the C ABI: forward, dX, dW vs float64 - one harness, the rest is rows
# --------------------------------------------------------------------------- #
#: bound vs float64 by products per tile (tests/test_gpu_parity.py: test_dense_block_fwd_bwd_vs_float64; 2 = the scaled
#: fp16x2 kernels behind the *_h2 entries, test_dense_block_fp16x2_vs_float64)
TOL = {0: 2e-6, 6: 2e-6, 3: 3e-5, 1: 2e-2, 2: 2e-6}
TOL_BIAS = 2e-6


def _rand(shape, seed, scale=1.0):
    """Full-mantissa float32 values (a 2^-16 grid would make every bf16 split exact)."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


class _Dense:
    """Operands of one dense block `out = relu?(sum_s x_s W_s^T + b)`; x_s are column slices of one slab.

    `off` shifts every base pointer by that many elements (1: nothing is 16-byte aligned), `ldpad` widens the leading
    dimensions of the slab / the gradient / the mask."""

    def __init__(self, n, fi, fo, nseg, off=0, ldpad=0):
        from deformcontact_amd.graph import current_stream_ptr
        self.n, self.fi, self.fo, self.nseg = n, fi, fo, nseg
        self.st = current_stream_ptr(torch.device(DEV))

        def view(rows, cols, seed, scale):
            ld = cols + ldpad
            flat = torch.zeros(rows * ld + off + 4, device=DEV)
            v = flat[off:off + rows * ld].view(rows, ld)[:, :cols]
            v.copy_(_rand((rows, cols), seed, scale))
            return v
        self.slab = view(n, nseg * fi, 5, 1.0)
        self.xs = [self.slab[:, s * fi:(s + 1) * fi] for s in range(nseg)]
        self.ldx = [self.slab.stride(0)] * nseg
        self.ws = []                                       # weights are dense [Fo, Fi] blocks (leading dimension Fi)
        for s in range(nseg):
            flat = torch.zeros(fo * fi + off + 4, device=DEV)
            w = flat[off:off + fo * fi].view(fo, fi)
            w.copy_(_rand((fo, fi), 40 + s, 1.0 / np.sqrt(fi)))
            self.ws.append(w)
        self.bias = _rand((fo,), 77, 0.5).to(DEV)
        self.g = view(n, fo, 91, 1.0)
        self.maskt = view(n, fo, 92, 1.0)                  # stands for the forward output: the mask is (> 0)
        self.x64 = [x.double().cpu() for x in self.xs]
        self.w64 = [w.double().cpu() for w in self.ws]

    def gm64(self, mask):
        g = self.g.double().cpu()
        return g * (self.maskt.double().cpu() > 0).double() if mask else g


class _Launched(dict):
    """`{kernel name: launches}` from the launch log of one call, and `.sites`: the launch sites that call reached."""
    sites = frozenset()


def _coverage_default():
    from deformcontact_amd import _lib
    return bool(os.environ.get(_lib.COVERAGE_ENV))                 # a measurement run keeps coverage on throughout


def _trace(fn):
    """Run `fn` with the launch log and launch-site coverage on.  The sites are the ones whose launch count moved during
    the call, so a site an earlier test reached does not pass for one this call missed."""
    from deformcontact_amd import _lib
    _lib.launch_coverage(True)
    before = _lib.launch_site_counts()
    _lib.kernel_trace(True)
    try:
        fn()
        torch.cuda.synchronize()
        out = _Launched(_lib.kernel_trace_counts())
        out.sites = frozenset(s for s, n in _lib.launch_site_counts().items() if n > before.get(s, 0))
        return out
    finally:
        _lib.kernel_trace(False)
        _lib.launch_coverage(_coverage_default())


def _assert_launched(launched, spec, times=None):
    """`spec`: a kernel name as the launch log has it, or "name | end of the site's identity" where the name alone does
    not tell the site (a templated launcher: "[L = 16]"; the second launch of a name in one function: "#2")."""
    name, _, end = spec.partition(" | ")
    assert launched.get(name, 0) >= 1 if times is None else launched.get(name, 0) == times, (spec, dict(launched))
    assert any(s.startswith(name + " @ ") and s.endswith(end) for s in launched.sites), (spec, sorted(launched.sites))


def _dense_fwd(d, relu, products, bias=True):
    from deformcontact_amd import _lib
    from deformcontact_amd.ops import _i64_array, _ptr_array
    L = _lib.lib()
    out = torch.full((d.n, d.fo), float("nan"), device=DEV)
    args = (_ptr_array(d.xs), _i64_array(d.ldx), _ptr_array(d.ws), d.nseg, d.bias.data_ptr() if bias else None,
            int(relu), out.data_ptr(), d.fo, d.n, d.fi, d.fo)
    if products == 2:
        from deformcontact_amd import ops
        rowmax, wmax = d.slab.abs().amax(1).contiguous(), ops.weight_rowmax(d.ws)
        call = lambda: _lib.check(L.dc_tag_linear_fwd_h2(*args, rowmax.data_ptr(), wmax.data_ptr(), d.st), "fwd_h2")
    elif products:
        call = lambda: _lib.check(L.dc_tag_linear_fwd_split(*args, products, d.st), "fwd_split")
    else:
        call = lambda: _lib.check(L.dc_tag_linear_fwd(*args, d.st), "fwd")
    counts = _trace(call)
    d.outputs = [out]                                      # the device tensors (tests/test_guard_bands.py)
    ref = sum(d.x64[s] @ d.w64[s].t() for s in range(d.nseg))
    if bias:
        ref = ref + d.bias.double().cpu()
    if relu:
        ref = ref.clamp_min(0)
    return counts, [("out", out.cpu().numpy(), ref.numpy(), TOL[products])]


def _dense_dx(d, mask, products):
    from deformcontact_amd import _lib
    from deformcontact_amd.ops import _i64_array, _ptr_array
    L = _lib.lib()
    gslab = torch.full((d.n, d.nseg * d.fi), float("nan"), device=DEV)
    gxs = [gslab[:, s * d.fi:(s + 1) * d.fi] for s in range(d.nseg)]
    ldgx = [gslab.stride(0)] * d.nseg
    m = d.maskt.data_ptr() if mask else None
    head = (d.g.data_ptr(), d.g.stride(0), m, d.maskt.stride(0), _ptr_array(d.ws), d.nseg, _ptr_array(gxs),
            _i64_array(ldgx))
    if products:
        nb = L.dc_tag_linear_bwd_dx_split_workspace_bytes(d.fi, d.fo, d.nseg)
        wsx = torch.empty(nb, dtype=torch.uint8, device=DEV)
        if products == 2:
            from deformcontact_amd import ops
            growmax, wmax = d.g.abs().amax(1).contiguous(), ops.weight_rowmax(d.ws)   # unmasked: an upper bound
            call = lambda: _lib.check(L.dc_tag_linear_bwd_dx_h2(*head, wsx.data_ptr(), nb, d.n, d.fi, d.fo,
                                                                growmax.data_ptr(), wmax.data_ptr(), d.st), "dx_h2")
        else:
            call = lambda: _lib.check(L.dc_tag_linear_bwd_dx_split(*head, wsx.data_ptr(), nb, d.n, d.fi, d.fo,
                                                                   products, d.st), "dx_split")
    else:
        call = lambda: _lib.check(L.dc_tag_linear_bwd_dx(*head, d.n, d.fi, d.fo, d.st), "dx")
    counts = _trace(call)
    d.outputs = [gslab]
    gm = d.gm64(mask)
    return counts, [(f"gx[{s}]", gxs[s].cpu().numpy(), (gm @ d.w64[s]).numpy(), TOL[products])
                    for s in range(d.nseg)]


def _dense_dw(d, mask, products, accumulate=0, bps=1, gbias=True):
    """`bps` output blocks per segment (ngw = bps * nseg), each of Fi // bps columns."""
    from deformcontact_amd import _lib
    from deformcontact_amd.ops import _i64_array, _ptr_array
    L = _lib.lib()
    cols = d.fi // bps
    init = 0.25 if accumulate else float("nan")
    gws = [torch.full((d.fo, cols), init, device=DEV) for _ in range(bps * d.nseg)]
    gb = torch.full((d.fo,), init, device=DEV)
    nb = L.dc_tag_linear_bwd_dw_workspace_bytes(d.n, d.fi, d.fo, d.nseg)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    m = d.maskt.data_ptr() if mask else None
    args = (d.g.data_ptr(), d.g.stride(0), m, d.maskt.stride(0), _ptr_array(d.xs), _i64_array(d.ldx), d.nseg,
            _ptr_array(gws), bps * d.nseg, cols, gb.data_ptr() if gbias else None, accumulate, scratch.data_ptr(), nb,
            d.n, d.fi, d.fo)
    counts = _trace(lambda: _lib.check(L.dc_tag_linear_bwd_dw_split(*args, products, d.st) if products
                                       else L.dc_tag_linear_bwd_dw(*args, d.st), "dw"))
    d.outputs = gws + ([gb] if gbias else [])
    gm = d.gm64(mask)
    base = 0.25 if accumulate else 0.0
    cmp = []
    for j in range(bps * d.nseg):
        s, b = divmod(j, bps)
        ref = (gm.t() @ d.x64[s])[:, b * cols:(b + 1) * cols] + base
        cmp.append((f"gw[{j}]", gws[j].cpu().numpy(), ref.numpy(), TOL[products]))
    if gbias:
        cmp.append(("gbias", gb.cpu().numpy(), (gm.sum(0) + base).numpy(), TOL_BIAS))
    return counts, cmp


def _check(counts, cmp, kernels):
    for k in kernels:
        _assert_launched(counts, k)
    for name, got, ref, tol in cmp:
        e = rel_err(got, ref)
        print(f"{name}: rel_err {e:.3e} (bound {tol:.0e})")
        assert e < tol, (name, e, tol)


# rows: (kernel names the launch log must hold, pass, n, fi, fo, nseg, keyword arguments)
#   pass "fwd": relu=, products=; "dx": mask=, products=; "dw": mask=, products=, accumulate=, bps=
#   shape: off= (elements every base pointer is shifted by), ldpad=
DENSE_ROWS = []


def _row(kernels, what, n, fi, fo, nseg, **kw):
    if isinstance(kernels, str):
        kernels = (kernels,)
    DENSE_ROWS.append(pytest.param(kernels, what, n, fi, fo, nseg, kw,
                                   id=f"{what}-{kernels[0].partition(' | ')[0]}-n{n}-fi{fi}-fo{fo}-s{nseg}"
                                      + "".join(f"-{k}{v}" for k, v in sorted(kw.items()))))


# ---- generic kernels with 128-row tiles: pick_mb needs ceil(N / 128) * column tiles >= 512 -> 64 x 8 at N = 8,065 ----
_row("k_tag_linear_fwd<2, false>", "fwd", 8065, 5, 1024, 1, relu=True)           # Fi % 4 != 0: not vec
_row("k_tag_linear_fwd<2, true>", "fwd", 8065, 20, 1024, 1, relu=False)          # vec, Fi % 16 != 0: fast ineligible
_row("k_fwd_fast<2>", "fwd", 8065, 16, 1024, 1, relu=True)
# dX: column tiles = ceil(Fi / 128) * nseg = 2 * 4
_row("k_tag_linear_bwd_dx<2, true, true>", "dx", 8065, 132, 20, 4, mask=True)    # vec, Fo % 16 != 0: fast ineligible
_row("k_tag_linear_bwd_dx<2, true, false>", "dx", 8065, 132, 20, 4, mask=False)
_row("k_tag_linear_bwd_dx<2, false, true>", "dx", 8065, 130, 5, 4, mask=True)    # Fi % 4 != 0
_row("k_tag_linear_bwd_dx<2, false, false>", "dx", 8065, 130, 5, 4, mask=False)
_row("k_dx_fast<2, true>", "dx", 8065, 132, 16, 4, mask=True)
_row("k_dx_fast<2, false>", "dx", 8065, 132, 16, 4, mask=False)
# ---- dW: 128-row tiles from Fo >= 128 (dw_mb); vec, but fewer than 16 rows: no 16-row stage for the fast kernel, and
# nothing before the tail to call it ragged - the generic kernel's vector form on the whole block ----
_row("k_tag_linear_bwd_dw<2, true, true> | #2", "dw", 7, 32, 128, 2, mask=True)
# ---- split kernels with 128-row tiles: split_mb is 2 when the 64-row tiles need a second round of 256 workgroups and
# the 128-row tiles do not: 33 x 8 = 264 > 256 >= 17 x 8 at N = 2,049 with 8 column tiles ----
_row("k_fwd_split<2, 3>", "fwd", 2049, 16, 1024, 1, relu=True, products=3)
_row("k_fwd_split<2, 1>", "fwd", 2049, 16, 1024, 1, relu=False, products=1)
_row("k_fwd_h2<2, false>", "fwd", 2049, 16, 1024, 1, relu=True, products=2)      # fp32 weights, one segment
_row("k_fwd_split<2, 2>", "fwd", 2049, 16, 1024, 2, relu=True, products=2)       # two segments: not k_fwd_h2
for _products in (3, 2, 1):
    _row(f"k_dx_split<2, true, {_products}>", "dx", 2049, 132, 16, 4, mask=True, products=_products)
    _row(f"k_dx_split<2, false, {_products}>", "dx", 2049, 132, 16, 4, mask=False, products=_products)
# ---- 64-row tiles (Fo < 128) without a mask ----
_row("k_dw_split<1, false, 3>", "dw", 64, 32, 64, 1, mask=False, products=3)
_row("k_dw_split<1, false, 1>", "dw", 64, 32, 64, 1, mask=False, products=1)
# ---- forms the suite reaches elsewhere, kept here with the arguments no other test gives them ----
_row("k_tag_linear_bwd_dw<1, false, false>", "dw", 33, 5, 7, 2, mask=False)      # Fo < 128, no mask, nothing % 4
# the ragged tail: vec, N % 16 != 0, N > 16 - the last 8 rows on the generic kernel, the first 32 on k_dw_fast
_row(("k_tag_linear_bwd_dw<2, true, true> | )", "k_dw_fast<2, true>"), "dw", 40, 32, 128, 2, mask=True)
_row("k_tag_linear_bwd_dw<1, false, true>", "dw", 33, 8, 8, 2, mask=True, off=1)  # every base pointer off by 4 bytes
_row("k_tag_linear_fwd<1, false>", "fwd", 33, 8, 8, 2, relu=True, off=1)
_row("k_tag_linear_bwd_dx<1, false, true>", "dx", 33, 8, 16, 2, mask=True, off=1)
_row(("k_dw_fast<1, false>", "k_dw_reduce"), "dw", 64, 32, 8, 2, mask=False, accumulate=1, bps=2)   # ngw = 2 * nseg
_row(("k_dw_fast<1, true>", "k_dw_reduce4"), "dw", 16144, 8, 8, 1, mask=True, accumulate=1)         # 64 chunks of 256


@pytest.mark.gpu
@pytest.mark.parametrize("kernels,what,n,fi,fo,nseg,kw", DENSE_ROWS)
def test_dense_site_vs_float64(kernels, what, n, fi, fo, nseg, kw):
    kw = dict(kw)
    d = _Dense(n, fi, fo, nseg, off=kw.pop("off", 0), ldpad=kw.pop("ldpad", 0))
    products = kw.pop("products", 0)
    if what == "fwd":
        counts, cmp = _dense_fwd(d, kw.pop("relu"), products)
    elif what == "dx":
        counts, cmp = _dense_dx(d, kw.pop("mask"), products)
    else:
        counts, cmp = _dense_dw(d, kw.pop("mask"), products, **kw)
        kw = {}
    assert not kw, kw
    _check(counts, cmp, kernels)


@pytest.mark.gpu
def test_wide_tile_forward_with_correction_operand_on_ragged_tiles():
    """`k_fwd_h2w<false, true>`: dc_tag_linear_fwd_h2p_corr (left operand x - coef[row] * x2, formed at load time) when
    the rows / columns do not fill the 128 x 256 tiles; the suite's only caller (the attention backward) pads to whole
    tiles.  2e-6 per row, the bound of the fp16x2 kernels."""
    from deformcontact_amd import _lib, ops
    from deformcontact_amd.graph import current_stream_ptr
    from deformcontact_amd.ops import _ptr_array
    from tests.helpers import row_rel_err
    L = _lib.lib()
    st = current_stream_ptr(torch.device(DEV))
    n, k, fo = 130, 64, 260
    x = (_rand((n, k), 1) * torch.logspace(-3, 0, n, dtype=torch.float64).float().unsqueeze(1)).to(DEV)
    x2, coef = _rand((n, k), 2).to(DEV), _rand((n,), 3, 0.5).to(DEV)
    w = _rand((fo, k), 4, 1.0 / np.sqrt(k)).to(DEV)
    wmax = ops.weight_rowmax([w])
    wimg = torch.empty(fo, k, device=DEV)
    _lib.check(L.dc_tag_weight_prep(_ptr_array([w]), 1, fo, k, wmax.data_ptr(), wimg.data_ptr(), None, None, st), "prep")
    rowmax = (x - coef.unsqueeze(1) * x2).abs().amax(1).contiguous()
    out = torch.full((n, fo), float("nan"), device=DEV)
    counts = _trace(lambda: _lib.check(L.dc_tag_linear_fwd_h2p_corr(
        x.data_ptr(), k, x2.data_ptr(), coef.data_ptr(), wimg.data_ptr(), out.data_ptr(), fo, n, k, fo,
        rowmax.data_ptr(), wmax.data_ptr(), st), "fwd_h2p_corr"))
    _assert_launched(counts, "k_fwd_h2w<false, true>", 1)
    ref = (x.double().cpu() - coef.double().cpu().unsqueeze(1) * x2.double().cpu()) @ w.double().cpu().t()
    e = row_rel_err(out.cpu().numpy(), ref.numpy())
    print(f"rel_err per row {e:.3e}")
    assert e < 2e-6, e


# --------------------------------------------------------------------------- #
# segment kernels: 1e-5 per row of float64
# --------------------------------------------------------------------------- #
def _csr_apply64(adj, x64, weighted=True):
    """float64 restatement of one hop over a destination-sorted adjacency: y[i] = sum over row i's slots of w * x[other]"""
    ptr, other = adj.ptr.cpu().numpy().astype(np.int64), adj.other.cpu().numpy().astype(np.int64)
    n = len(ptr) - 1
    e = int(ptr[-1])
    w = adj.w.cpu().numpy().astype(np.float64)[:e] if weighted else np.ones(e)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    y = np.zeros((n, x64.shape[1]))
    np.add.at(y, rows, w[:, None] * x64[other[:e]])
    return y


#: (the kernel, nodes of the largest graph, weighted, gcn): STEPS = ceil(nodes / rows per step), 128 rows per step with
#: 32-column slices (up to 1,024 nodes), 256 with 16-column slices (up to 2,048), 512 with 8-column slices (up to 4,096)
CHAIN_ROWS = [("k_hop_chain_gcn<4>", 512, True, True), ("k_hop_chain_gcn<5>", 513, True, True),
              ("k_hop_chain_gcn<7>", 800, True, True),
              ("k_hop_chain<true, 4, 8>", 500, True, False), ("k_hop_chain<true, 5, 8>", 640, True, False),
              ("k_hop_chain<true, 7, 8>", 769, True, False),
              ("k_hop_chain<false, 2, 8>", 250, False, False), ("k_hop_chain<false, 4, 8>", 385, False, False),
              ("k_hop_chain<false, 5, 8>", 600, False, False), ("k_hop_chain<false, 7, 8>", 896, False, False),
              ("k_hop_chain<true, 5, 4>", 1025, True, False), ("k_hop_chain<true, 7, 4>", 1700, True, False),
              ("k_hop_chain<false, 5, 4>", 1280, False, False), ("k_hop_chain<false, 7, 4>", 1537, False, False),
              ("k_hop_chain<true, 5, 2>", 2049, True, False), ("k_hop_chain<true, 7, 2>", 3100, True, False),
              ("k_hop_chain<false, 5, 2>", 2560, False, False), ("k_hop_chain<false, 7, 2>", 3584, False, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,big,weighted,gcn", CHAIN_ROWS, ids=[r[0] for r in CHAIN_ROWS])
def test_hop_chain_site_vs_float64(kernel, big, weighted, gcn):
    """One launch of dc_hop_chain_f32 over a ragged batch whose largest graph picks the instantiation: equal bit for bit
    to the hops one by one (blocks and row maxima), and every hop within 1e-5 per row of float64 applied to the block
    it read."""
    from deformcontact_amd.graph import GraphIndex
    from tests.helpers import row_rel_err
    from tests.test_hop_chain import batch_of_graphs, run_both
    f, k = 32, 2
    ei, segs = batch_of_graphs((37, big, 130), (3, 5, 2), seed=big, hub=(1, 41))
    n = segs[0][-1]
    g = GraphIndex(ei.to(DEV), n, segments=segs)
    out = {}
    counts = _trace(lambda: out.update(slab=run_both(g, g.fwd, n, f, k, 1, weighted=weighted, gcn=gcn, seed=big)))
    _assert_launched(counts, kernel, 1)
    slab = out["slab"]
    blocks = slab.cpu().numpy().astype(np.float64)
    for j in range(k):
        ref = _csr_apply64(g.fwd, blocks[:, j * f:(j + 1) * f], weighted)
        e = row_rel_err(blocks[:, (j + 1) * f:(j + 2) * f], ref)
        print(f"hop {j}: rel_err per row {e:.3e}")
        assert e < 1e-5, (j, e)


BF16_HOP_ROWS = [(37, "k_spmm_bf16x1<L, 8, OUT_F32>", "L = 64, X8 = false"),
                 (96, "k_spmm_bf16x8<L, 8, OUT_F32>", "L = 16, X8 = true")]


def _bf16_hop_run(f, kernel, form):
    """-> (graph, x, addend, {out_f32: y}): both output types of one bf16 hop, the site of each asserted"""
    from deformcontact_amd import ops
    from deformcontact_amd.graph import GraphIndex
    from tests.helpers import random_multigraph
    n, e = 333, 2500
    g = GraphIndex(torch.from_numpy(random_multigraph(n, e, f)).to(DEV), n)
    xb = _rand((n, f), 7, 2.0).to(DEV).bfloat16()
    add = _rand((n, f), 8).to(DEV).bfloat16()
    ys = {}
    for out_f32 in (True, False):
        dt = torch.float32 if out_f32 else torch.bfloat16
        counts = _trace(lambda: ys.update({out_f32: ops.hop_bf16(g.fwd, xb, addend=add.to(dt), out_dtype=dt)}))
        assert len(counts) == 1, dict(counts)
        _assert_launched(counts, f"{kernel} | [{form}, OUT_F32 = {'true' if out_f32 else 'false'}]", 1)
    return g, xb, add, ys


@pytest.mark.gpu
@pytest.mark.parametrize("f,kernel,form", BF16_HOP_ROWS)
def test_bf16_hop_site_vs_float64(f, kernel, form):
    """dc_spmm_bf16 at the widths that pick 64 lanes per row of the any-alignment kernel (32 < F, F % 8 != 0) and 16
    lanes per row of the 16-byte kernel (64 < F <= 128), with an addend.  The fp32 output within 1e-5 per row of
    float64; the bf16 output equal bit for bit to that fp32 output rounded once to bf16 (the addend holds bf16 values in
    both calls, so both accumulate the same fp32 sum: all the bf16 form adds is the one rounding on store)."""
    from tests.helpers import row_rel_err
    g, xb, add, ys = _bf16_hop_run(f, kernel, form)
    ref = add.double().cpu().numpy() + _csr_apply64(g.fwd, xb.double().cpu().numpy())
    err = row_rel_err(ys[True].double().cpu().numpy(), ref)
    print(f"rel_err per row {err:.3e}")
    assert err < 1e-5, err
    assert ys[False].dtype == torch.bfloat16 and torch.equal(ys[False], ys[True].bfloat16())


PACK_WPREP_ROWS = [(16, 16), (9, 16), (8, 8), (3, 8)]


def _pack_wprep_run(fi, kernel_l):
    """-> (adjacency, weights, x, slab, weight image) of one dc_spmm_f32_pack_wprep launch, its site asserted"""
    from deformcontact_amd import _lib
    from deformcontact_amd.graph import GraphIndex, current_stream_ptr
    from deformcontact_amd.ops import _ptr_array
    from tests.helpers import random_multigraph
    from tests.test_narrow_prepared import _image_buffer, _weights
    L = _lib.lib()
    n, e, nseg, wpad = 1003, 7001, 4, 96
    st = current_stream_ptr(torch.device(DEV))
    g = GraphIndex(torch.from_numpy(random_multigraph(n, e, fi)).to(DEV), n)
    adj = g.fwd
    ws = _weights(fi, nseg, "odd_offset_views", torch.Generator().manual_seed(fi))
    x = _rand((n, fi), fi).to(DEV)
    width = nseg * fi
    slab = torch.full((n, wpad + 8), float("nan"), device=DEV)[:, :wpad]
    buf = _image_buffer(wpad)
    counts = _trace(lambda: _lib.check(L.dc_spmm_f32_pack_wprep(
        adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), x.data_ptr(), x.stride(0), slab.data_ptr(),
        slab.stride(0), n, fi, width, wpad, _ptr_array(ws), nseg, buf.data_ptr(), st), "pack_wprep"))
    _assert_launched(counts, f"k_spmm_sub_wimg<L, 8> | [L = {kernel_l}]", 1)
    return adj, ws, x, slab, buf


@pytest.mark.gpu
@pytest.mark.parametrize("fi,kernel_l", PACK_WPREP_ROWS)
def test_pack_with_weight_image_at_narrow_inputs(fi, kernel_l):
    """dc_spmm_f32_pack_wprep with 16 / 8 lanes per row (F <= 16 / F <= 8; the shipped first layers have F = 21 / 25):
    the weight image equal bit for bit to the CPU restatement of the three bf16 planes, block 0 the input, block 1 the
    first hop within 1e-5 per row of float64, the K padding zero."""
    from tests.helpers import row_rel_err
    from tests.test_narrow_prepared import _check_image
    nseg, wpad, width = 4, 96, 4 * fi
    adj, ws, x, slab, buf = _pack_wprep_run(fi, kernel_l)
    _check_image(buf, ws, fi, nseg, wpad)
    got = slab.cpu().numpy()
    assert np.array_equal(got[:, :fi], x.cpu().numpy())
    assert not got[:, width:wpad].any()
    err = row_rel_err(got[:, fi:2 * fi], _csr_apply64(adj, x.double().cpu().numpy()))
    print(f"rel_err per row {err:.3e}")
    assert err < 1e-5, err


def _morton_codes_run():
    """-> (positions on the host, lo, 1 / extent, codes on the device) of one dc_morton_codes launch, its site asserted"""
    import ctypes
    from deformcontact_amd import _lib
    from deformcontact_amd.graph import current_stream_ptr
    n, ld = 1000, 5                                               # 4 blocks, the last one ragged; rows wider than 3
    base = _rand((n, ld), 11, 1.5)                                # beyond [lo, lo + extent) on both sides: the clamps
    pos = base.to(DEV)
    lo, inv = np.array([-1.0, -0.5, 0.25], np.float32), np.array([0.5, 1.0, 2.0], np.float32)
    codes = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    F3 = ctypes.c_float * 3
    counts = _trace(lambda: _lib.check(_lib.lib().dc_morton_codes(
        pos.data_ptr(), ld, n, F3(*lo), F3(*inv), codes.data_ptr(), current_stream_ptr(torch.device(DEV))), "morton"))
    assert len(counts) == 1, dict(counts)
    _assert_launched(counts, "k_morton", 1)
    return base, lo, inv, codes


@pytest.mark.gpu
def test_morton_codes_entry():
    """dc_morton_codes (`k_morton`): 10 bits per axis of (pos - lo) * inv_extent * 1024, clamped to [0, 1023] and
    interleaved x, y, z from bit 0.  Equal to the float32 restatement of the same three operations; a float64 evaluation
    may put a point that sits on a cell boundary into the neighbouring cell, never further."""
    base, lo, inv, codes = _morton_codes_run()
    n = base.shape[0]
    p = base.numpy()[:, :3]

    def cells(dtype):
        t = (p.astype(dtype) - lo.astype(dtype)) * inv.astype(dtype) * dtype(1024)
        return np.clip(t, 0, 1023).astype(np.int64)

    def interleave(c):
        out = np.zeros(len(c), np.int64)
        for bit in range(10):
            for ax in range(3):
                out |= ((c[:, ax] >> bit) & 1) << (3 * bit + ax)
        return out
    got = codes.cpu().numpy()
    assert np.array_equal(got, interleave(cells(np.float32)))
    back = np.stack([sum(((got >> (3 * bit + ax)) & 1) << bit for bit in range(10)) for ax in range(3)], 1)
    assert np.abs(back - cells(np.float64)).max() <= 1
    assert (back == 0).any() and (back == 1023).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "multigraph"])
def test_spline_backward_in_h_on_a_narrow_vector_row(kind):
    """`k_spline_bwd_h<4, false>`: float4 columns (M % 4 == 0) with K * M / 4 <= 32 lanes per row (the suite's vector
    shapes all fill a wave): M = 8, K = 4.  1e-5 per row of the float64 formula, both reductions."""
    from deformcontact_amd import ops
    from tests import test_spline_conv as sc
    m, ks, dim, degree = 8, (4,), 1, 1
    case = sc.bwd_case(kind, m, ks, dim, degree)
    g, k = sc._device_graph(kind)[0], case["K"]
    a, gy = sc._dev(case["a"]), sc._dev(case["gy"])
    b, wi = ops._spline_basis(a, case["ks"], case["op"], degree)
    win = sc._np(wi).astype(np.int64)
    for mean in (True, False):
        want = sc.bwd_truth(case, sc._np(b), win, mean, case["gb"])
        out = {}
        counts = _trace(lambda: out.update(gh=ops._spline_bwd_h(g, b, wi, gy, k, mean)))
        _assert_launched(counts, "k_spline_bwd_h<4, false>", 1)
        sc._within_bar_of_float64(sc._np(out["gh"]), want["gh"], f"spline g_h M={m} K={k} {kind} mean={mean}")
