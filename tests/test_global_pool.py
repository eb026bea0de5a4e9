"""``global_add_pool`` / ``global_mean_pool`` / ``global_max_pool`` (``deformcontact_amd.pointops``) and the C entries
``dc_pool_fwd`` / ``dc_pool_bwd`` of dc_pointnet.hip.

The reference is this file's own restatement of the contract (pointops' docstring): a torch CPU
composition in float32 and float64 (``index_add_``; the max in the mask / count form of tests/test_edge_conv.py, so
autograd yields the even split among all rows that attain the maximum), and numpy formulas for the entries.

The order of the sums is part of the contract: one workgroup per (graph, column block), the rows of a graph dealt to 16
slots - slot ``s`` adds the rows ``a + s, a + s + 16, ...`` in ascending order from 0 - and the 16 partial sums added in
slot order.  ``pool_sum_f32`` is that loop in numpy, and the device's sums are compared with it bit for bit; the mean is
that sum divided by ``np.float32(rows)``; the max and its counts are exact; the backward is one copy or one division
per element.

Shapes: B = 5 graphs of 1, 0, 7, 300 and 1025 rows - a single row, an empty graph, fewer rows than slots, and segments
that take many rounds of the 16 slots x 4 rows in flight - at every width the kernels treat differently (scalar 1, 3,
70; 16-byte 20, 64, 256; 1100: many column blocks).  The max inputs come from a coarse grid, so ties are certain.
"""
import functools

import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, pointops
from deformcontact_amd.nn import global_add_pool, global_max_pool, global_mean_pool  # noqa: F401  (no test without them)
from tests.helpers import assert_parity, rel_err
from tests.test_edge_conv import _odd, _wide, coarse_grid, segment_max, signed
from tests.test_gat_edge_kernels import _dev, _np

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

COUNTS = [1, 0, 7, 300, 1025]
WIDTHS = [1, 3, 20, 64, 70, 256, 1100]
MODES = {"add": 0, "mean": 1, "max": 2}
FNS = {"add": pointops.global_add_pool, "mean": pointops.global_mean_pool, "max": pointops.global_max_pool}


def pool_sum_f32(ptr, x, slots=pointops.POOL_SLOTS):
    """the documented order, add by add: per graph 16 slot sums over the rows a + s, a + s + 16, ..., then the slot
    sums in slot order"""
    y = np.zeros((len(ptr) - 1, x.shape[1]), np.float32)
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        part = np.zeros((slots, x.shape[1]), np.float32)
        for s in range(slots):
            for r in range(a + s, b, slots):
                part[s] = part[s] + x[r]
        acc = part[0].copy()
        for s in range(1, slots):
            acc = acc + part[s]
        y[g] = acc
    return y


@functools.lru_cache(maxsize=None)
def pool_case(c, counts=tuple(COUNTS)):
    counts = np.asarray(counts)
    nb, n = len(counts), int(counts.sum())
    batch = np.repeat(np.arange(nb), counts)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    rng = np.random.default_rng(500 + c + nb)
    x, xg, gy = rng.standard_normal((n, c)).astype(np.float32), coarse_grid(rng, (n, c)), signed(rng, (nb, c))
    s32 = pool_sum_f32(ptr, x)
    cntf = np.maximum(counts, 1).astype(np.float32)[:, None]
    y, cnt = segment_max(nb, batch, xg)
    fwd = {"add": s32, "mean": np.where(counts[:, None] > 0, s32 / cntf, np.float32(0)), "max": y}
    bwd = {"add": gy[batch], "mean": gy[batch] / cntf[batch],
           "max": np.where(xg == y[batch], gy[batch] / np.maximum(cnt, 1).astype(np.float32)[batch], np.float32(0))}
    assert all(v.dtype == np.float32 for v in list(fwd.values()) + list(bwd.values()))
    return dict(nb=nb, n=n, batch=batch, ptr=ptr, counts=counts, x=x, xg=xg, gy=gy, cnt=cnt, fwd=fwd, bwd=bwd)


def ref_pool(x, batch, nb, mode):
    """torch restatement in ``x``'s dtype; the max in the mask / count form (mask and cnt constant: the even split)"""
    zeros = x.new_zeros((nb, x.size(1)))
    if mode == "max":
        with torch.no_grad():
            y, _ = segment_max(nb, batch.numpy(), x.numpy())
            mask = (x == torch.from_numpy(y)[batch]).to(x.dtype)
            cnt = zeros.clone().index_add_(0, batch, mask)
        return zeros.index_add_(0, batch, mask * x / cnt[batch].clamp(min=1))
    out = zeros.index_add_(0, batch, x)
    if mode == "mean":
        out = out / torch.bincount(batch, minlength=nb).clamp(min=1).to(x.dtype)[:, None]
    return out


def _ref_run(case, mode, dtype):
    x = torch.from_numpy(case["xg"] if mode == "max" else case["x"]).to(dtype).requires_grad_(True)
    out = ref_pool(x, torch.from_numpy(case["batch"]), case["nb"], mode)
    (out * torch.from_numpy(case["gy"]).to(dtype)).sum().backward()
    return out.detach().numpy(), x.grad.numpy()


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_errors_raised_on_the_host():
    x, batch = torch.zeros(6, 4), torch.zeros(6, dtype=torch.long)
    for name, fn in FNS.items():
        who = f"global_{name}_pool"
        with pytest.raises(TypeError, match=who):
            fn("x", batch)
        for bad in (x.double(), x[0], torch.zeros(6, 0), torch.zeros(6, 4, 1)):
            with pytest.raises(ValueError, match=who):
                fn(bad, batch)
        for bad in (batch.int(), batch[:5], batch[None]):
            with pytest.raises(ValueError, match="batch"):
                fn(x, bad)
        with pytest.raises(ValueError, match="size"):
            fn(x, batch, -1)
        with pytest.raises(TypeError):
            fn(x, batch, 2.5)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(x, batch)                                         # every host check passed: no CPU path
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(x, None)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(x, batch, 3)


def test_exports():
    assert dc.nn.global_add_pool is pointops.global_add_pool and dc.nn.global_mean_pool is pointops.global_mean_pool
    assert dc.nn.global_max_pool is pointops.global_max_pool
    names = dc.nn.__all__
    at = names.index("global_add_pool")
    assert names[at - 1:at + 3] == ["PointNetConv", "global_add_pool", "global_mean_pool", "global_max_pool"]
    assert sorted(n for n in _lib.exported_names() if n.startswith("dc_pool_")) == ["dc_pool_bwd", "dc_pool_fwd"]
    assert pointops.POOL_SLOTS == 16


def _fwd(L, rows, c, ok, ld, mode=0, nb=2):
    p = lambda a, on=True: a if ok and on else None
    return L.dc_pool_fwd(p(64), p(128), ld, p(256), ld, p(320, mode == 2), ld, mode, rows, nb, c, None)


def _bwd(L, rows, c, ok, ld, mode=0, nb=2):
    p = lambda a, on=True: a if ok and on else None
    return L.dc_pool_bwd(p(64), p(64), p(128, mode == 2), ld, p(256, mode == 2), ld, p(320, mode == 2), ld, p(384), ld,
                         p(448), ld, mode, rows, nb, c, None)


def test_abi_argument_errors_of_the_pool_entries_without_gpu():
    """short leading dimensions, null pointers, aliased outputs, a bad mode, cnt given for a sum or missing for the
    max, ptr missing for several graphs, sizes out of range: -1 and the entry's own message, before any HIP call; no
    graph (forward) or no row (backward) returns 0 with no pointer at all."""
    L = _lib.lib()
    err = L.dc_last_error
    for name, call in (("dc_pool_fwd", _fwd), ("dc_pool_bwd", _bwd)):
        tag = name.encode()
        for mode in (0, 1, 2):
            assert call(L, 3, 16, False, 64, mode) == -1 and tag in err() and b"null" in err(), (name, mode)
            assert call(L, 3, 16, True, 15, mode) == -1 and tag in err() and b"leading" in err(), (name, mode)
            assert call(L, 3, 16, False, 15, mode) == -1 and b"leading" in err(), (name, mode)
        assert call(L, -1, 16, True, 64) == -1 and tag in err(), name
        assert call(L, 3, 16, True, 64, nb=-1) == -1 and tag in err(), name
        assert call(L, 3, 0, True, 64) == -1 and tag in err(), name
        assert call(L, 3, 1 << 24, True, 1 << 24) == -1 and b"range" in err(), name
        assert call(L, 1 << 30, 16, True, 64) == -1 and b"range" in err(), name
        for mode in (-1, 3, 7):
            assert call(L, 3, 16, True, 64, mode) == -1 and b"mode" in err() and tag in err(), (name, mode)
            assert call(L, 0, 16, False, 64, mode, nb=0) == -1 and b"mode" in err(), (name, mode)
    # zero sizes: no graph - nothing to write; no row - the forward still writes its zeros, the backward has no output
    for mode in (0, 1, 2):
        assert _fwd(L, 5, 16, False, 64, mode, nb=0) == 0 and _bwd(L, 0, 16, False, 64, mode) == 0
        assert _fwd(L, 0, 16, False, 64, mode) == -1 and b"null" in err()
        assert _fwd(L, 0, 16, False, 15, mode, nb=0) == -1 and _bwd(L, 0, 16, False, 15, mode) == -1
    # ptr (and batch) may be NULL for one graph only; the mean's backward reads ptr
    assert L.dc_pool_fwd(None, 128, 16, 256, 16, None, 16, 0, 3, 2, 16, None) == -1 and b"one graph" in err()
    assert L.dc_pool_bwd(None, None, None, 16, None, 16, None, 16, 384, 16, 448, 16, 0, 3, 2, 16, None) == -1 \
        and b"one graph" in err()
    assert L.dc_pool_bwd(64, None, None, 16, None, 16, None, 16, 384, 16, 448, 16, 1, 3, 2, 16, None) == -1 and b"ptr" in err()
    # cnt: written by the max only
    for mode in (0, 1):
        assert L.dc_pool_fwd(64, 128, 16, 256, 16, 320, 16, mode, 3, 2, 16, None) == -1 and b"cnt" in err()
    assert L.dc_pool_fwd(64, 128, 16, 256, 16, None, 16, 2, 3, 2, 16, None) == -1 and b"cnt" in err() and b"null" in err()
    # outputs that alias an operand
    assert L.dc_pool_fwd(64, 128, 16, 128, 16, None, 16, 0, 3, 2, 16, None) == -1 and b"alias" in err()
    assert L.dc_pool_fwd(64, 128, 16, 256, 16, 128, 16, 2, 3, 2, 16, None) == -1 and b"alias" in err()
    assert L.dc_pool_fwd(64, 128, 16, 256, 16, 256, 16, 2, 3, 2, 16, None) == -1 and b"alias" in err()
    assert L.dc_pool_bwd(64, 64, None, 16, None, 16, None, 16, 384, 16, 384, 16, 0, 3, 2, 16, None) == -1 and b"alias" in err()
    for other in (128, 256, 320):
        assert L.dc_pool_bwd(64, 64, 128, 16, 256, 16, 320, 16, 384, 16, other, 16, 2, 3, 2, 16, None) == -1 \
            and b"alias" in err()


def test_float32_restatement_within_the_bar_of_float64_and_formulas_agree_with_autograd():
    """every case of the GPU tests: the float32 restatement within 1e-5 of the float64 one (output and gradient); the
    slot-ordered float32 sums within 1e-5 of float64; the hand-written backward formulas equal float64 autograd; the max
    cases hold ties"""
    for c in WIDTHS:
        case = pool_case(c)
        assert (case["cnt"] >= 2).mean() > 0.1 and (case["cnt"][1] == 0).all()
        for mode in MODES:
            o32, g32 = _ref_run(case, mode, torch.float32)
            o64, g64 = _ref_run(case, mode, torch.float64)
            assert rel_err(o32, o64) < TOL and rel_err(g32, g64) < TOL, (c, mode)
            assert rel_err(case["fwd"][mode], o64) < TOL and rel_err(case["bwd"][mode], g64) < 1e-6, (c, mode)
            assert (case["fwd"][mode][1] == 0).all()             # the graph without rows


# --------------------------------------------------------------------------- #
# GPU
# --------------------------------------------------------------------------- #
def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(case):
    return _dev(case["ptr"].astype(np.int64))


@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_pool_forward_entry_and_functions(c):
    """sum bit-identical to the slot-ordered float32 loop, mean that sum divided by ``np.float32(rows)``, max and its
    counts exact; x as a column slice (aligned and not), strided outputs: the same bits; the three functions with and
    without ``size``: the same bits; twice: the same bits"""
    case = pool_case(c)
    nb, n = case["nb"], case["n"]
    L, ptr, batch = _lib.lib(), _ptr(case), _dev(case["batch"])
    x, xg = _dev(case["x"]), _dev(case["xg"])
    for name, mode in MODES.items():
        src = xg if mode == 2 else x
        for view, ld in ((src, c), (_wide(src), c + 12), (_odd(src), c + 3)):
            for ldy in (c, c + 8):
                o_y = torch.full((nb, ldy), 7.0, device=DEV)
                o_c = torch.full((nb, ldy), 7, dtype=torch.int32, device=DEV) if mode == 2 else None
                _lib.check(L.dc_pool_fwd(ptr.data_ptr(), view.data_ptr(), ld, o_y.data_ptr(), ldy,
                                         None if o_c is None else o_c.data_ptr(), ldy, mode, n, nb, c, _st()), "dc_pool_fwd")
                assert np.array_equal(_np(o_y[:, :c]), case["fwd"][name]), (name, c, ld, ldy)
                assert (o_y[:, c:] == 7.0).all()
                if mode == 2:
                    assert np.array_equal(_np(o_c[:, :c]), case["cnt"]) and (o_c[:, c:] == 7).all()
        want = _dev(case["fwd"][name])
        for view in (src, _wide(src), _odd(src)):
            assert torch.equal(FNS[name](view, batch), want) and torch.equal(FNS[name](view, batch, nb), want)
        assert torch.equal(FNS[name](src, batch, nb), want)
        # more graphs than ids: empty ones at the end; fewer: the rows of the others take no part
        more = FNS[name](src, batch, nb + 2)
        assert more.shape == (nb + 2, c) and torch.equal(more[:nb], want) and (more[nb:] == 0).all()
        assert torch.equal(FNS[name](src, batch, 4), want[:4])


@gpu
@pytest.mark.parametrize("c", WIDTHS)
def test_pool_backward_entry_and_node(c):
    """bit-identical to the numpy float32 formula; operands as column slices, a strided output: the same bits; through
    autograd with a contiguous, a non-contiguous and an expanded gradient: the same bits; a repeat: the same bits"""
    case = pool_case(c)
    nb, n = case["nb"], case["n"]
    L, ptr, batch = _lib.lib(), _ptr(case), _dev(case["batch"])
    x, xg, gy = _dev(case["x"]), _dev(case["xg"]), _dev(case["gy"])
    y, cnt = _dev(case["fwd"]["max"]), _dev(case["cnt"])
    for name, mode in MODES.items():
        want = _dev(case["bwd"][name])
        for views in ((xg, y, cnt, gy), (_wide(xg), _wide(y), _wide(cnt), _wide(gy)), (_odd(xg), y, _odd(cnt), _odd(gy))):
            for ldg in (c, c + 8):
                xv, yv, cv, gv = views
                o_g = torch.full((n, ldg), 7.0, device=DEV)
                sv = [xv.data_ptr(), xv.stride(0), yv.data_ptr(), yv.stride(0), cv.data_ptr(), cv.stride(0)] \
                    if mode == 2 else [None, c, None, c, None, c]
                _lib.check(L.dc_pool_bwd(batch.data_ptr(), ptr.data_ptr(), *sv, gv.data_ptr(), gv.stride(0), o_g.data_ptr(),
                                         ldg, mode, n, nb, c, _st()), "dc_pool_bwd")
                assert torch.equal(o_g[:, :c], want) and (o_g[:, c:] == 7.0).all(), (name, c, ldg)
        src = xg if mode == 2 else x
        xs = _wide(src).detach().requires_grad_(True)
        wide_g = torch.full((nb, 2 * c), 1e30, device=DEV)
        wide_g[:, ::2] = gy
        for size in (None, nb):
            for grad in (gy, gy, wide_g[:, ::2], _wide(gy), _odd(gy)):
                xs.grad = None
                torch.autograd.backward([FNS[name](xs, batch, size)], [grad])
                assert torch.equal(xs.grad, want), (name, c)
        xs.grad = None
        FNS[name](xs, batch, nb).sum().backward()                # an expanded gradient of ones
        ones = xs.grad.clone()
        xs.grad = None
        torch.autograd.backward([FNS[name](xs, batch, nb)], [torch.ones_like(gy)])
        assert torch.equal(xs.grad, ones) and ones.abs().max() > 0
        # fewer graphs than ids: the rows beyond get a zero gradient
        xs.grad = None
        torch.autograd.backward([FNS[name](xs, batch, 4)], [gy[:4]])
        cut = int(case["ptr"][4])
        assert torch.equal(xs.grad[:cut], want[:cut]) and (xs.grad[cut:] == 0).all()


@gpu
@pytest.mark.parametrize("c", [3, 64, 1100])
def test_one_graph_without_batch_and_no_rows(c):
    """``batch=None``: one graph of all rows, ``[1, C]``, in the same slot order; N = 0: zeros (or no row) and an empty
    gradient"""
    case = pool_case(c, (1333,))
    assert case["nb"] == 1
    x, xg, gy = _dev(case["x"]), _dev(case["xg"]), _dev(case["gy"])
    for name, mode in MODES.items():
        src = (xg if mode == 2 else x).requires_grad_(True)
        src.grad = None
        out = FNS[name](src, None)
        assert out.shape == (1, c) and np.array_equal(_np(out), case["fwd"][name]), (name, c)
        assert torch.equal(out, FNS[name](src, None, 9))         # size is ignored without a batch, as in PyG
        assert torch.equal(out, FNS[name](src, _dev(case["batch"]))) and torch.equal(out, FNS[name](_odd(src.detach()), None))
        torch.autograd.backward([out], [gy])
        assert np.array_equal(_np(src.grad), case["bwd"][name]), (name, c)
        e = torch.zeros((0, c), device=DEV, requires_grad=True)
        none = FNS[name](e, None)
        assert none.shape == (1, c) and (none == 0).all()
        none.sum().backward()
        assert e.grad.shape == (0, c)
        b0 = torch.zeros(0, dtype=torch.int64, device=DEV)
        assert FNS[name](e, b0).shape == (0, c)
        three = FNS[name](e, b0, 3)
        assert three.shape == (3, c) and (three == 0).all()
        three.sum().backward()


@gpu
@pytest.mark.parametrize("name", list(MODES))
def test_functions_against_the_restatement_and_their_launches(name):
    """the function against the float32 / float64 restatement at 1e-5, output and gradient; one launch forward, one
    backward, nothing else of the library"""
    case = pool_case(70)
    o32, g32 = _ref_run(case, name, torch.float32)
    o64, g64 = _ref_run(case, name, torch.float64)
    x = _dev(case["xg"] if name == "max" else case["x"]).requires_grad_(True)
    batch = _dev(case["batch"])
    _lib.kernel_trace(True)
    out = FNS[name](x, batch, case["nb"])
    torch.autograd.backward([out], [_dev(case["gy"])])
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    assert sum(counts.values()) == 2 and any("k_pool_fwd<" in k for k in counts) and any("k_pool_bwd<" in k for k in counts), counts
    assert_parity(_np(out), o32, o64, TOL, f"global_{name}_pool forward")
    assert_parity(_np(x.grad), g32, g64, TOL, f"global_{name}_pool x.grad")
