"""CPU: the width-F kNN entry (``dc_neighbors_nd_fill``), ``neighbors.knn_padded_nd`` and ``DynamicEdgeConv`` - argument
checks, names, and the numpy reference of the GPU tests run over every one of their inputs.

Every rejection here happens before anything touches a device: the C entry returns DC_EINVAL before any HIP call, the
Python functions raise before they allocate."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, neighbors
from tests import nd_reference as ref

EINVAL, OK = -1, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_the_library_exports_it():
    with open(os.path.join(ROOT, "include", "deformcontact.h")) as f:
        header = f.read()
    assert re.search(r"\bint dc_neighbors_nd_fill\(const float \*x, int64_t ldx, int64_t nx, const int64_t \*batch_x,",
                     header)
    chunk = re.search(r"#define DC_NEIGHBORS_ND_CHUNK (\d+)", header)
    assert chunk and int(chunk.group(1)) == neighbors.ND_CHUNK      # the widths of the GPU tests follow the kernel
    assert neighbors.ND_CHUNK >= 4 and neighbors.ND_CHUNK % 2 == 0
    assert hasattr(_lib.lib(), "dc_neighbors_nd_fill")


def test_fill_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    fake = ctypes.c_void_p(16)                     # never dereferenced: every call below fails its checks first

    def fill(x=fake, ldx=8, nx=10, y=fake, ldy=8, ny=10, f=8, cap=8, nbr=fake, counts=fake):
        return L.dc_neighbors_nd_fill(x, ldx, nx, None, y, ldy, ny, None, f, cap, 1, nbr, counts, None)
    for kw, msg in ((dict(x=None), b"null"), (dict(y=None), b"null"), (dict(nbr=None), b"null"),
                    (dict(counts=None), b"null"), (dict(f=0), b"width f=0"), (dict(f=-3), b"width f=-3"),
                    (dict(ldx=7), b"leading"), (dict(ldy=3), b"leading"), (dict(cap=65), b"cap=65"),
                    (dict(cap=-1), b"cap=-1"), (dict(nx=-1), b"bad sizes"), (dict(ny=-5), b"bad sizes"),
                    (dict(nx=2 ** 31), b"bad sizes")):
        assert fill(**kw) == EINVAL, kw
        err = L.dc_last_error()
        assert err.startswith(b"dc_neighbors_nd_fill: ") and msg in err, (kw, err)
    # nothing to do: DC_OK before the null check
    assert fill(ny=0, x=None, y=None, nbr=None, counts=None) == OK
    assert fill(cap=0, x=None, y=None, nbr=None, counts=None) == OK
    assert fill(ny=0, cap=0, nx=0, x=None, y=None, nbr=None, counts=None) == OK


def test_knn_padded_nd_rejects_unsupported_operands(monkeypatch):
    x = torch.zeros(6, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        neighbors.knn_padded_nd(x, x, 3)
    with pytest.raises(TypeError, match="tensor"):
        neighbors.knn_padded_nd(x.numpy(), x, 3)
    with pytest.raises(ValueError, match="k=65"):
        neighbors.knn_padded_nd(x, x, 65)
    # the checks below come after the device check: stub it out, as tests/test_neighbors_host.py does
    monkeypatch.setattr(neighbors, "_require_cuda", lambda t, what: None)
    with pytest.raises(TypeError, match="float32"):
        neighbors.knn_padded_nd(x.double(), x.double(), 3)
    for bad in (torch.zeros(6), torch.zeros(6, 8, 1), torch.zeros(6, 0)):
        with pytest.raises(ValueError, match=r"\[N, F\] rows of width F >= 1"):
            neighbors.knn_padded_nd(bad, bad, 3)
    with pytest.raises(ValueError, match=r"^y must be \[N, F\]"):
        neighbors.knn_padded_nd(x, torch.zeros(6), 3)
    with pytest.raises(ValueError, match="inner stride"):
        neighbors.knn_padded_nd(torch.zeros(8, 6).t(), x, 3)
    with pytest.raises(ValueError, match="non-overlapping"):
        neighbors.knn_padded_nd(torch.zeros(16).as_strided((6, 8), (1, 1)), x, 3)
    with pytest.raises(ValueError, match="same width"):
        neighbors.knn_padded_nd(x, torch.zeros(6, 9), 3)
    neighbors._check_rows(torch.zeros(4, 11)[:, 2:9], "x")                   # a row stride is fine
    neighbors._check_rows(torch.zeros(4, 3), "x")                            # and so is width 3


def test_the_knn_functions_dispatch_on_the_width():
    """Only a float32 device matrix of a width other than 3 leaves the grid path; what the grid path refused it still
    refuses with its own words (CPU tensors never reach either kernel)."""
    assert not neighbors._is_nd(torch.zeros(5, 3)) and not neighbors._is_nd(torch.zeros(5, 8))    # CPU
    assert not neighbors._is_nd(torch.zeros(5, 8, device="meta"))
    assert not neighbors._is_nd(None)
    for fn in (lambda p: dc.nn.knn_graph(p, 3), lambda p: dc.nn.knn(p, p, 3), lambda p: neighbors.knn_padded(p, p, 3)):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(torch.zeros(5, 8))
    with pytest.raises(ValueError, match="cosine"):
        dc.nn.knn_graph(torch.zeros(5, 8), 3, cosine=True)
    with pytest.raises(ValueError, match="cosine"):
        dc.nn.knn(torch.zeros(5, 8), torch.zeros(5, 8), 3, cosine=True)


def test_dynamic_edge_conv_surface():
    from deformcontact_amd.nn import DynamicEdgeConv, EdgeConv
    mlp = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ReLU(), torch.nn.Linear(8, 4))
    for k in (0, 65, 2.5, -1, True, "3", None):
        with pytest.raises(ValueError, match="k must be an integer"):
            DynamicEdgeConv(mlp, k)
    with pytest.raises(ValueError, match="aggr"):
        DynamicEdgeConv(mlp, 3, aggr="min")
    assert dc.nn.__all__[9] == "DynamicEdgeConv" and dc.nn.DynamicEdgeConv is DynamicEdgeConv
    conv = DynamicEdgeConv(mlp, k=5, aggr="add", num_workers=4)
    assert isinstance(conv, EdgeConv) and conv.k == 5 and conv.aggr == "sum"
    assert repr(conv) == f"DynamicEdgeConv(nn={mlp}, k=5)"
    assert list(conv.state_dict()) == ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]
    assert DynamicEdgeConv(mlp, 64).k == 64 and DynamicEdgeConv(mlp, 1).aggr == "max"
    before = mlp[0].weight.clone()
    torch.manual_seed(1)
    conv.reset_parameters()                                                  # inherited: resets the user's module
    assert not torch.equal(before, mlp[0].weight)
    # the static-graph error is PyG's text and comes before the device check
    with pytest.raises(ValueError, match="^Static graphs not supported in DynamicEdgeConv$"):
        conv(torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="Static graphs"):
        conv(torch.zeros(7))
    with pytest.raises(RuntimeError, match="HIP device"):
        conv(torch.zeros(5, 3))
    for args in (((torch.zeros(5, 3), torch.zeros(5, 3)),), (torch.zeros(5, 3), (None, None))):
        with pytest.raises(TypeError, match="bipartite"):
            conv(*args)


def test_pyg_alias_exports_dynamic_edge_conv():
    dc.install_as_torch_geometric()
    try:
        import torch_geometric.nn as tgnn
        from torch_geometric.nn import DynamicEdgeConv
        assert DynamicEdgeConv is dc.nn.DynamicEdgeConv and tgnn.DynamicEdgeConv is DynamicEdgeConv
    finally:
        for k in ("torch_geometric", "torch_geometric.nn", "torch_geometric.data"):
            sys.modules.pop(k, None)


def test_the_numpy_reference_over_every_gpu_input():
    """The reference of tests/test_neighbors_nd.py, run here over all of that file's inputs: it is quick, and every
    query gets exactly min(k, n_g) neighbours - min(k, n_g - 1) where ``exclude_self`` drops the query itself -, each
    one a row of the query's own graph, no row twice, ranks ascending in (d2, j)."""
    t0 = time.perf_counter()
    cases = ref.cases()
    assert {f"width{f}-ex0" for f in ref.WIDTHS} <= set(cases) and len(set(ref.WIDTHS)) == len(ref.WIDTHS)
    for name, c in cases.items():
        nbr, counts = ref.knn_ref(c["x"], c["y"], c["k"], c["bx"], c["by"], c["exclude_self"])
        nx, ny = c["x"].shape[0], c["y"].shape[0]
        want = ref.expected_counts(c["k"], c["bx"], c["by"], nx, ny, c["exclude_self"])
        assert np.array_equal(counts, want), name
        assert nbr.shape == (ny, c["k"]) and np.array_equal(nbr >= 0, np.arange(c["k"])[None, :] < counts[:, None]), name
        bx = np.zeros(nx, np.int64) if c["bx"] is None else c["bx"]
        by = np.zeros(ny, np.int64) if c["by"] is None else c["by"]
        for i in range(ny):
            row = nbr[i, :counts[i]]
            assert np.unique(row).size == row.size and np.all(bx[row] == by[i]), (name, i)
            if c["exclude_self"]:
                assert i not in row, (name, i)
            d2 = ref.d2_columns(c["x"][row], c["y"][i:i + 1])[0] if row.size else np.zeros(0, np.float32)
            key = list(zip(d2.tolist(), row.tolist()))
            assert key == sorted(key), (name, i)
    assert (ref.knn_ref(cases["xy"]["x"], cases["xy"]["y"], 20, cases["xy"]["bx"], cases["xy"]["by"])[1][50:71] == 0).all()
    assert time.perf_counter() - t0 < 20.0
