"""CPU: argument checks of the kNN / radius graph builders (C entries and Python functions) and their PyG names.

Every rejection here happens before anything touches a device: the C entries return DC_EINVAL before any HIP call,
the Python functions raise before they allocate."""
import ctypes
import sys

import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, neighbors

EINVAL = -1


def test_fill_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.dc_neighbors_workspace_bytes(-1, 4) < 0 and L.dc_neighbors_workspace_bytes(4, -1) < 0
    assert L.dc_neighbors_workspace_bytes(100, 100) > 0 and L.dc_neighbors_workspace_bytes(0, 5) == 0
    fake = ctypes.c_void_p(16)                     # never dereferenced: every call below fails its checks first

    def fill(x=fake, ldx=3, nx=10, y=fake, ldy=3, ny=10, mode=0, r=0.5, cap=8, nbr=fake, counts=fake, ws=fake,
             nbytes=1 << 30):
        return L.dc_neighbors_fill(x, ldx, nx, None, y, ldy, ny, None, mode, r, cap, 1, nbr, counts, ws, nbytes, None)
    for kw, msg in ((dict(nx=-1), b"bad sizes"), (dict(ny=-5), b"bad sizes"), (dict(cap=65), b"cap=65"),
                    (dict(cap=-1), b"cap=-1"), (dict(mode=2), b"mode"), (dict(mode=1, r=-1.0), b"radius"),
                    (dict(mode=1, r=float("nan")), b"radius"), (dict(ldx=2), b"leading"),
                    (dict(y=None), b"null"), (dict(counts=None), b"null"), (dict(nbr=None), b"null"),
                    (dict(x=None), b"null"), (dict(ws=None), b"null"), (dict(nbytes=16), b"workspace too small")):
        assert fill(**kw) == EINVAL, kw
        assert msg in L.dc_last_error(), (kw, L.dc_last_error())


def test_compact_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.dc_neighbors_compact_workspace_bytes(-1) < 0 and L.dc_neighbors_compact_workspace_bytes(0) == 0
    assert L.dc_neighbors_compact_workspace_bytes(1000) >= 8000
    fake = ctypes.c_void_p(16)

    def compact(nbr=fake, cap=8, counts=fake, ny=10, row=1, out=fake, m=20, ws=fake, nbytes=1 << 30):
        return L.dc_neighbors_compact(nbr, cap, counts, ny, row, out, m, ws, nbytes, None)
    for kw, msg in ((dict(ny=-1), b"bad sizes"), (dict(m=-1), b"bad sizes"), (dict(cap=65), b"cap=65"),
                    (dict(row=2), b"query_row"), (dict(nbr=None), b"null"), (dict(counts=None), b"null"),
                    (dict(out=None), b"null"), (dict(ws=None), b"null"), (dict(nbytes=8), b"workspace too small")):
        assert compact(**kw) == EINVAL, kw
        assert msg in L.dc_last_error(), (kw, L.dc_last_error())


def test_python_functions_reject_unsupported_inputs():
    pos = torch.zeros(5, 3)
    for fn in (lambda p: dc.nn.knn_graph(p, 3), lambda p: dc.nn.radius_graph(p, 0.1),
               lambda p: dc.nn.knn(p, p, 3), lambda p: dc.nn.radius(p, p, 0.1),
               lambda p: neighbors.knn_padded(p, p, 3), lambda p: neighbors.radius_padded(p, p, 0.1)):
        with pytest.raises(RuntimeError, match="HIP device"):          # the convs' error: no CPU path
            fn(pos)
    # the checks below fail before the device check would: fake a device tensor's answers
    meta = torch.empty(5, 3, device="meta")
    with pytest.raises(RuntimeError, match="HIP device"):
        dc.nn.knn_graph(meta, 3)
    with pytest.raises(ValueError, match="cosine"):
        dc.nn.knn_graph(pos, 3, cosine=True)
    with pytest.raises(ValueError, match="cosine"):
        dc.nn.knn(pos, pos, 3, cosine=True)
    for k in (65, 100, -1):
        with pytest.raises(ValueError, match=r"^k"):
            neighbors._check_cap(k, "k")
    assert neighbors._check_cap(64, "k") == 64 and neighbors._check_cap(0, "k") == 0
    with pytest.raises(ValueError, match="max_num_neighbors=65"):
        dc.nn.radius_graph(pos, 0.1, max_num_neighbors=65)
    with pytest.raises(ValueError, match="k=65"):
        dc.nn.knn_graph(pos, 65)
    with pytest.raises(ValueError, match="flow"):
        dc.nn.knn_graph(pos, 3, flow="both")
    with pytest.raises(ValueError, match="r must be"):
        dc.nn.radius_graph(pos, -0.5)


def test_position_checks_say_why(monkeypatch):
    """float64, a width other than 3 and an inner stride other than 1 are refused with a reason (the device check is
    stubbed out here: these inputs would reach it first on a CPU-only box)."""
    monkeypatch.setattr(neighbors, "_require_cuda", lambda t, what: None)
    with pytest.raises(TypeError, match="float32"):
        neighbors._check_points(torch.zeros(4, 3, dtype=torch.float64), "x")
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        neighbors._check_points(torch.zeros(4, 2), "x")
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        neighbors._check_points(torch.zeros(4, 3, 1), "x")
    with pytest.raises(ValueError, match="inner stride"):
        neighbors._check_points(torch.zeros(3, 4).t(), "x")
    neighbors._check_points(torch.zeros(4, 8)[:, 2:5], "x")                  # a row stride is fine
    with pytest.raises(ValueError, match="sorted int64"):
        neighbors._check_batch(torch.zeros(4, dtype=torch.int32), 4, torch.device("cpu"), "batch")
    with pytest.raises(ValueError, match="sorted int64"):
        neighbors._check_batch(torch.zeros(3, dtype=torch.int64), 4, torch.device("cpu"), "batch")


def test_pyg_alias_exports_the_graph_builders():
    dc.install_as_torch_geometric()
    try:
        import torch_geometric.nn as tgnn
        from torch_geometric.nn import knn, knn_graph, radius, radius_graph
        assert knn_graph is dc.nn.knn_graph and radius_graph is dc.nn.radius_graph
        assert knn is dc.nn.knn and radius is dc.nn.radius
        assert knn is neighbors.knn and knn_graph is neighbors.knn_graph
        assert radius is neighbors.radius and radius_graph is neighbors.radius_graph
        assert tgnn.knn is dc.nn.conv.knn
    finally:
        for k in ("torch_geometric", "torch_geometric.nn", "torch_geometric.data"):
            sys.modules.pop(k, None)
