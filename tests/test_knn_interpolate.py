"""``knn_interpolate`` (``deformcontact_amd.pointops``, csrc/dc_pointops.hip): PointNet++ feature propagation.

CPU: argument errors of the Python function and of the two C entries, the exported names.
GPU: the forward bit for bit against a numpy fp32 loop over the ``nbr`` / ``counts`` that ``knn_padded`` returned (the
neighbour search has its own tests: this file pins the interpolation); the backward against the same maths in float64,
started from the kernel's fp32 ``d2`` values so that only the summation is compared, under ``helpers.assert_parity``."""
import sys

import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, neighbors, pointops
from deformcontact_amd.deferred import resolve
from tests.helpers import assert_parity

DEV = torch.device("cuda:0")
EINVAL = -1


# ---------------------------------------------------------------------------------------------------------------- #
# CPU
# ---------------------------------------------------------------------------------------------------------------- #
def test_argument_errors(monkeypatch):
    x, pos = torch.zeros(5, 4), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        dc.nn.knn_interpolate(x, pos, pos)
    with pytest.raises(TypeError, match="tensor"):
        dc.nn.knn_interpolate(None, pos, pos)
    monkeypatch.setattr(pointops, "_require_cuda", lambda t, what: None)
    for bad in (torch.zeros(5, 4, dtype=torch.float64), torch.zeros(5), torch.zeros(5, 0), torch.zeros(5, 4, 1)):
        with pytest.raises(ValueError, match=r"float32 \[Nx, F >= 1\]"):
            dc.nn.knn_interpolate(bad, pos, pos)
    for k in (65, -1):
        with pytest.raises(ValueError, match=r"^k"):
            dc.nn.knn_interpolate(x, pos, pos, k=k)
    with pytest.raises(RuntimeError, match="HIP device"):                # the positions: the neighbour search's checks
        dc.nn.knn_interpolate(x, pos, pos)
    monkeypatch.setattr(neighbors, "_require_cuda", lambda t, what: None)
    with pytest.raises(TypeError, match="float32"):
        dc.nn.knn_interpolate(x, pos.double(), pos)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        dc.nn.knn_interpolate(x, torch.zeros(5, 2), pos)
    with pytest.raises(ValueError, match="x has 5 rows but pos_x has 4"):
        dc.nn.knn_interpolate(x, pos[:4], pos)


def _entry_calls():
    """name -> call(rows, width, pointers given?, leading dimension, k) of the two entries, otherwise valid; ``rows`` is
    the entry's row count (Ny forward, Nx backward)"""
    L = _lib.lib()
    p = lambda ok, a=64: a if ok else None                           # any non-null address: rejected calls never touch it
    return {
        "dc_knn_interpolate_fwd": lambda r, f, ok, ld, k=3: L.dc_knn_interpolate_fwd(
            p(ok), ld, p(ok, 128), 3, p(ok, 192), 3, p(ok, 256), p(ok, 320), k, p(ok, 384), ld, None, None, 7, r, f, None),
        "dc_knn_interpolate_bwd": lambda r, f, ok, ld, k=3: L.dc_knn_interpolate_bwd(
            p(ok), p(ok, 128), p(ok, 192), p(ok, 256), p(ok, 320), ld, p(ok, 384), ld, k, r, 7, f, None),
    }


def test_abi_argument_errors_without_gpu():
    L = _lib.lib()
    calls = _entry_calls()
    assert sorted(n for n in _lib.exported_names() if n.startswith("dc_knn_")) == sorted(calls)
    for name, call in calls.items():
        err = lambda: L.dc_last_error()
        assert call(3, 16, False, 64) == EINVAL and name.encode() in err() and b"null" in err(), name
        assert call(3, 16, True, 15) == EINVAL and name.encode() in err() and b"leading" in err(), name
        assert call(3, 16, False, 15) == EINVAL and b"leading" in err(), name        # sizes, strides, then nulls
        assert call(0, 16, False, 64) == 0, name                     # no row: nothing is read, written or launched
        assert call(0, 16, False, 15) == EINVAL, name
        assert call(-1, 16, True, 64) == EINVAL and name.encode() in err(), name
        assert call(3, 0, True, 64) == EINVAL and name.encode() in err(), name
        assert call(3, -2, True, 64) == EINVAL and name.encode() in err(), name
        assert call(3, 1 << 24, True, 1 << 24) == EINVAL and b"range" in err(), name
        assert call(1 << 30, 16, True, 64) == EINVAL and b"range" in err(), name
        for k in (0, -1, 65):
            assert call(3, 16, True, 64, k) == EINVAL and b"k=" in err() and name.encode() in err(), (name, k)
    # the positions need three columns; w and den come together; an output must not be an input
    assert L.dc_knn_interpolate_fwd(64, 16, 128, 2, 192, 3, 256, 320, 3, 384, 16, None, None, 7, 3, 16, None) == EINVAL
    assert b"leading" in L.dc_last_error()
    assert L.dc_knn_interpolate_fwd(64, 16, 128, 3, 192, 3, 256, 320, 3, 384, 16, 448, None, 7, 3, 16, None) == EINVAL
    assert b"come together" in L.dc_last_error()
    assert L.dc_knn_interpolate_fwd(64, 16, 128, 3, 192, 3, 256, 320, 3, 64, 16, None, None, 7, 3, 16, None) == EINVAL
    assert b"alias" in L.dc_last_error()
    assert L.dc_knn_interpolate_fwd(64, 16, 128, 3, 192, 3, 256, 320, 3, 384, 16, 448, 448, 7, 3, 16, None) == EINVAL
    assert b"alias" in L.dc_last_error()
    assert L.dc_knn_interpolate_bwd(64, 128, 192, 256, 320, 16, 320, 16, 3, 3, 7, 16, None) == EINVAL
    assert b"alias" in L.dc_last_error()
    assert L.dc_knn_interpolate_fwd(64, 16, 128, 3, 192, 3, 256, 320, 3, 384, 16, None, None, -1, 3, 16, None) == EINVAL
    assert L.dc_knn_interpolate_bwd(64, 128, 192, 256, 320, 16, 384, 16, 3, 3, -1, 16, None) == EINVAL


def test_exports_and_alias():
    assert dc.nn.knn_interpolate is pointops.knn_interpolate
    assert "knn_interpolate" in dc.nn.__all__
    dc.install_as_torch_geometric()
    try:
        from torch_geometric.nn import knn_interpolate
        assert knn_interpolate is pointops.knn_interpolate
    finally:
        for k in ("torch_geometric", "torch_geometric.nn", "torch_geometric.data"):
            sys.modules.pop(k, None)


# ---------------------------------------------------------------------------------------------------------------- #
# the reference
# ---------------------------------------------------------------------------------------------------------------- #
EPS = np.float32(1e-16)


def _d2(px, py, nbr):
    """fp32 [Ny, k]: the kernel's d2 of every slot (the padding reads point 0: masked by the callers)"""
    d = px[np.maximum(nbr, 0)] - py[:, None, :]                      # float32, x_j - y_i
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def ref_forward(x, px, py, nbr, counts):
    """the forward in fp32, rank by rank: every product, sum and division rounds as the kernel's does"""
    ny, k = nbr.shape
    w = np.float32(1.0) / np.maximum(_d2(px, py, nbr), EPS)
    num, den = np.zeros((ny, x.shape[1]), np.float32), np.zeros(ny, np.float32)
    for r in range(k):
        on = counts > r
        j = nbr[on, r]
        num[on] = num[on] + w[on, r][:, None] * x[j]
        den[on] = den[on] + w[on, r]
    y = np.zeros_like(num)
    has = counts > 0
    y[has] = num[has] / den[has, None]
    return y


def ref_backward(gy, px, py, nbr, counts, nx, dtype):
    """g_x in ``dtype`` from the kernel's fp32 d2 values, slots in ascending (i, r) order"""
    ny, k = nbr.shape
    on = np.arange(k)[None, :] < counts[:, None]
    w = np.where(on, dtype(1.0) / np.maximum(_d2(px, py, nbr), EPS).astype(dtype), dtype(0.0))
    den = np.zeros(ny, dtype)
    for r in range(k):
        den = den + w[:, r]
    gx = np.zeros((nx, gy.shape[1]), dtype)
    t = gy.astype(dtype) / np.where(den > 0, den, dtype(1.0))[:, None]
    for i in range(ny):
        for r in range(int(counts[i])):
            gx[nbr[i, r]] += w[i, r] * t[i]
    return gx


def _points(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def _feat(n, f, seed):
    return np.random.default_rng(seed).standard_normal((n, f), dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(px, py, k, bx=None, by=None):
    nbr, counts = neighbors.knn_padded(px, py, k, bx, by)
    return nbr.cpu().numpy(), counts.cpu().numpy()


SHAPES = [(1, 1), (2, 5), (70, 33), (300, 257)]
WIDTHS = [1, 3, 4, 64, 67, 256]
KS = [1, 3, 8]


# ---------------------------------------------------------------------------------------------------------------- #
# GPU: forward
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_forward_bit_for_bit(nx, ny):
    px, py = _points(nx, 10 + nx), _points(ny, 20 + ny)
    dpx, dpy = _dev(px), _dev(py)
    for k in KS:
        nbr, counts = _padded(dpx, dpy, k)
        assert counts.max() == min(k, nx)                            # k > Nx: fewer neighbours than slots
        for f in WIDTHS:
            x = _feat(nx, f, 30 + f)
            got = dc.nn.knn_interpolate(_dev(x), dpx, dpy, k=k)
            assert got.shape == (ny, f) and got.dtype == torch.float32 and got.is_contiguous()
            assert np.array_equal(got.cpu().numpy(), ref_forward(x, px, py, nbr, counts)), (k, f)


@pytest.mark.gpu
def test_a_query_without_a_neighbour_gets_zeros():
    """graph 1 of batch_y has no counterpart in batch_x: its queries get rows of zeros, not PyG's NaN"""
    px, py = _points(40, 1), _points(90, 2)
    bx = torch.tensor([0] * 25 + [2] * 15).to(DEV)
    by = torch.tensor([0] * 30 + [1] * 20 + [2] * 40).to(DEV)
    x = _feat(40, 64, 3)
    nbr, counts = _padded(_dev(px), _dev(py), 3, bx, by)
    assert (counts[30:50] == 0).all() and (counts[:30] == 3).all() and (counts[50:] == 3).all()
    xg = _dev(x).requires_grad_(True)
    got = dc.nn.knn_interpolate(xg, _dev(px), _dev(py), bx, by, k=3)
    out = got.detach().cpu().numpy()
    assert np.isfinite(out).all() and (out[30:50] == 0).all() and np.abs(out[:30]).min() > 0
    assert np.array_equal(out, ref_forward(x, px, py, nbr, counts))
    got.sum().backward()
    assert torch.isfinite(xg.grad).all()
    empty = dc.nn.knn_interpolate(_dev(x)[:0], _dev(px)[:0], _dev(py), k=3)        # no source at all
    assert empty.shape == (90, 64) and not empty.any()
    assert dc.nn.knn_interpolate(_dev(x), _dev(px), _dev(py)[:0], k=3).shape == (0, 64)
    assert not dc.nn.knn_interpolate(_dev(x), _dev(px), _dev(py), k=0).any()


@pytest.mark.gpu
def test_queries_on_top_of_sources_take_the_clamp():
    px = _points(70, 4)
    py = _points(33, 5)
    py[:12] = px[5:17]                                               # exact copies: d2 = 0, w = 1 / 1e-16
    x = _feat(70, 67, 6)
    nbr, counts = _padded(_dev(px), _dev(py), 3)
    got = dc.nn.knn_interpolate(_dev(x), _dev(px), _dev(py), k=3).cpu().numpy()
    assert np.array_equal(got, ref_forward(x, px, py, nbr, counts))
    assert (nbr[:12, 0] == np.arange(5, 17)).all() and np.isfinite(got).all()
    assert np.abs(got[:12] - x[5:17]).max() <= 1e-6 * np.abs(x).max()


@pytest.mark.gpu
def test_x_as_a_column_slice_and_as_a_deferred_conv_result():
    px, py = _points(70, 7), _points(33, 8)
    dpx, dpy = _dev(px), _dev(py)
    nbr, counts = _padded(dpx, dpy, 3)
    wide = _dev(_feat(70, 80, 9))
    for lo, f in ((4, 64), (3, 64), (5, 67), (8, 4)):                # 16-byte aligned rows and not
        xs = wide[:, lo:lo + f]
        assert not xs.is_contiguous()
        got = dc.nn.knn_interpolate(xs, dpx, dpy, k=3)
        assert np.array_equal(got.cpu().numpy(), ref_forward(xs.cpu().numpy(), px, py, nbr, counts)), (lo, f)
    torch.manual_seed(5)
    conv = dc.nn.GCNConv(80, 16).to(DEV)
    with torch.no_grad():
        h = conv(wide, dc.nn.knn_graph(dpx, 4))
        assert type(h).__name__ == "DeferredActivation"
        a, b = dc.nn.knn_interpolate(h, dpx, dpy, k=3), dc.nn.knn_interpolate(resolve(h), dpx, dpy, k=3)
    assert type(a) is torch.Tensor and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), ref_forward(resolve(h).cpu().numpy(), px, py, nbr, counts))


# ---------------------------------------------------------------------------------------------------------------- #
# GPU: backward
# ---------------------------------------------------------------------------------------------------------------- #
def _backward(x, dpx, dpy, gy, k, bx=None, by=None):
    xg = x.detach().requires_grad_(True)
    y = dc.nn.knn_interpolate(xg, dpx, dpy, bx, by, k=k)
    y.backward(gy)
    return y.detach(), xg.grad


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", SHAPES + [(2, 257)])              # (2, 257): every source selected by 257 queries
def test_backward_against_float64(nx, ny):
    px, py = _points(nx, 40 + nx), _points(ny, 50 + ny)
    dpx, dpy = _dev(px), _dev(py)
    for k in KS:
        nbr, counts = _padded(dpx, dpy, k)
        picked = np.bincount(nbr[nbr >= 0], minlength=nx)
        if (nx, ny) == (2, 257) and k >= 2:
            assert (picked == 257).all()
        if (nx, ny) == (300, 257) and k == 1:
            assert (picked == 0).any()                               # sources that no query selected
        for f in WIDTHS:
            gy = _feat(ny, f, 60 + f)
            _, gx = _backward(_dev(_feat(nx, f, 70 + f)), dpx, dpy, _dev(gy), k)
            assert gx.shape == (nx, f) and gx.dtype == torch.float32
            got = gx.cpu().numpy()
            assert not got[picked == 0].any()                        # ... get a zero row
            assert_parity(got, ref_backward(gy, px, py, nbr, counts, nx, np.float32),
                          ref_backward(gy, px, py, nbr, counts, nx, np.float64), name=f"gx {nx}x{ny} k={k} F={f}")


@pytest.mark.gpu
def test_backward_gradient_layouts_and_positions_get_none():
    px, py = _points(70, 80), _points(33, 81)
    nbr, counts = _padded(_dev(px), _dev(py), 3)
    x = _dev(_feat(70, 64, 82)).requires_grad_(True)
    dpx, dpy = _dev(px).requires_grad_(True), _dev(py).requires_grad_(True)
    y = dc.nn.knn_interpolate(x, dpx, dpy, k=3)
    gx, gpx, gpy = torch.autograd.grad(y.sum(), (x, dpx, dpy), allow_unused=True, retain_graph=True)   # an expanded g_y
    assert gpx is None and gpy is None
    ones = np.ones((33, 64), np.float32)
    assert_parity(gx.cpu().numpy(), ref_backward(ones, px, py, nbr, counts, 70, np.float32),
                  ref_backward(ones, px, py, nbr, counts, 70, np.float64), name="gx expanded")
    wide = _dev(_feat(33, 72, 83))
    for g in (wide[:, 4:68], wide[:, 3:67], wide.t()[4:68].t()):     # column slices of a wider gradient
        gx, = torch.autograd.grad(y, x, g, retain_graph=True)
        assert_parity(gx.cpu().numpy(), ref_backward(g.cpu().numpy(), px, py, nbr, counts, 70, np.float32),
                      ref_backward(g.cpu().numpy(), px, py, nbr, counts, 70, np.float64), name="gx sliced")
    gt = _dev(_feat(64, 33, 84)).t()                                 # a transposed gradient: inner stride != 1
    gx, = torch.autograd.grad(y, x, gt)
    assert_parity(gx.cpu().numpy(), ref_backward(gt.cpu().numpy(), px, py, nbr, counts, 70, np.float32),
                  ref_backward(gt.cpu().numpy(), px, py, nbr, counts, 70, np.float64), name="gx transposed")
    with torch.no_grad():                                            # no gradient wanted: nothing is saved
        assert torch.equal(dc.nn.knn_interpolate(x, dpx, dpy, k=3), y)


@pytest.mark.gpu
def test_capture_forward_and_backward_and_replay():
    nx, ny, f = 300, 257, 64
    sx, spx, spy, sgy = (_dev(a) for a in (_feat(nx, f, 90), _points(nx, 91), _points(ny, 92), _feat(ny, f, 93)))
    bx = torch.tensor([0] * 120 + [1] * 180).to(DEV)
    by = torch.tensor([0] * 100 + [1] * 157).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _backward(sx, spx, spy, sgy, 3, bx, by)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y, gx = _backward(sx, spx, spy, sgy, 3, bx, by)
    for seed in (94, 98):
        new = (_dev(a) for a in (_feat(nx, f, seed), _points(nx, seed + 1), _points(ny, seed + 2), _feat(ny, f, seed + 3)))
        new = list(new)
        for dst, src in zip((sx, spx, spy, sgy), new):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        wy, wgx = _backward(*new[:3], new[3], 3, bx, by)
        assert torch.equal(y, wy) and torch.equal(gx, wgx)


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    x, dpx, dpy, gy = (_dev(a) for a in (_feat(2, 67, 1), _points(2, 2), _points(257, 3), _feat(257, 67, 4)))
    a, b = _backward(x, dpx, dpy, gy, 3), _backward(x, dpx, dpy, gy, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    x, dpx, dpy, gy = (_dev(a) for a in (_feat(300, 256, 5), _points(300, 6), _points(257, 7), _feat(257, 256, 8)))
    a, b = _backward(x, dpx, dpy, gy, 8), _backward(x, dpx, dpy, gy, 8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- #
# GPU: fps down, knn_interpolate up
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_fps_then_knn_interpolate_reproduces_the_sampled_rows():
    """The PointNet++ down-and-up path on a three-graph batch.  At a sampled node the query lies on its source: the
    clamp weight 1e16 swamps the other two (distinct random points: d2 > 1e-8, w < 1e8), so the row comes back within
    1e-6 relative."""
    sizes = [90, 257, 40]
    pos, x = _dev(_points(sum(sizes), 1)), _dev(_feat(sum(sizes), 64, 2))
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(DEV)
    idx = dc.nn.fps(pos, batch, 0.25, random_start=False)
    assert idx.numel() == 23 + 65 + 10 and idx.unique().numel() == idx.numel()
    up = dc.nn.knn_interpolate(x[idx], pos[idx], pos, batch[idx], batch, k=3)
    assert up.shape == x.shape and torch.isfinite(up).all()
    err = (up[idx] - x[idx]).abs().max().item() / x[idx].abs().max().item()
    print(f"  sampled rows: {err:.2e} relative")
    assert err <= 1e-6
