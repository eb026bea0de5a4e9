"""GPU: kNN / radius graph construction (``deformcontact_amd.neighbors``, csrc/dc_neighbors.hip) against a numpy
restatement of its rules, bit for bit.

The reference below is not the code under test.  Candidates of a query come from brute force for graphs of up to
4,096 points, and from scipy's cKDTree ``query_ball_point`` with the radius inflated by 1e-4 relative for larger
clouds; ``d2 = ((dx*dx + dy*dy) + dz*dz)`` is then recomputed in float32 numpy (one rounding per operation), ranked by
``(d2, j)`` (``np.lexsort``) and cut at the cap.  Every comparison is ``torch.equal`` on the edge index."""
import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, neighbors, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BRUTE_MAX = 4096


# ---------------------------------------------------------------------------------------------------------------- #
# the reference: rules 1-5 restated in numpy
# ---------------------------------------------------------------------------------------------------------------- #
def _d2(xc, yq):
    d = xc - yq                                                     # float32, x_j - y_i
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _rank_and_cut(i, j, d2, cap):
    """(query, neighbour) pairs in output order: by query, then (d2, j); at most cap per query."""
    o = np.lexsort((j, d2, i))
    i, j = i[o], j[o]
    if i.size == 0:
        return i, j
    starts = np.r_[0, np.flatnonzero(np.diff(i)) + 1]
    first = np.repeat(starts, np.diff(np.r_[starts, i.size]))
    keep = np.arange(i.size) - first < cap
    return i[keep], j[keep]


def _graph_pairs(x, y, xi, yi, cap, r, exclude_self):
    """The kept (query, neighbour) pairs of one graph: xi / yi = its global point indices in x / y."""
    r2 = None if r is None else np.float32(r) * np.float32(r)
    out_i, out_j = [], []
    if xi.size == 0 or yi.size == 0 or cap == 0:
        return out_i, out_j
    if xi.size <= BRUTE_MAX:
        for c in range(0, yi.size, 512):
            q = yi[c:c + 512]
            d2 = _d2(x[xi][None, :, :], y[q][:, None, :])           # [q, n] float32
            keep = np.ones(d2.shape, bool)
            if exclude_self:
                keep &= xi[None, :] != q[:, None]
            if r2 is not None:
                keep &= d2 < r2
            qi, cj = np.nonzero(keep)
            a, b = _rank_and_cut(q[qi], xi[cj], d2[qi, cj], cap)       # (a query's pairs are all in this chunk)
            out_i.append(a), out_j.append(b)
    else:
        from scipy.spatial import cKDTree
        assert r is not None, "the reference takes big clouds for radius searches only"
        tree = cKDTree(x[xi].astype(np.float64))
        for c in range(0, yi.size, 8192):
            q = yi[c:c + 8192]
            cand = tree.query_ball_point(y[q].astype(np.float64), r * (1 + 1e-4), workers=16)
            lens = np.fromiter((len(v) for v in cand), np.int64, len(cand))
            qq = np.repeat(q, lens)
            jj = xi[np.fromiter((v for lst in cand for v in lst), np.int64, int(lens.sum()))]
            d2 = _d2(x[jj], y[qq])
            keep = d2 < r2
            if exclude_self:
                keep &= jj != qq
            a, b = _rank_and_cut(qq[keep], jj[keep], d2[keep], cap)
            out_i.append(a), out_j.append(b)
    return out_i, out_j


def reference(x, y, cap, r=None, batch_x=None, batch_y=None, exclude_self=False):
    """(query index, neighbour index) int64 arrays in the order rule 5 prescribes."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    bx = np.zeros(len(x), np.int64) if batch_x is None else np.asarray(batch_x)
    by = np.zeros(len(y), np.int64) if batch_y is None else np.asarray(batch_y)
    ii, jj, dd = [], [], []
    for g in np.unique(by):
        pi, pj = _graph_pairs(x, y, np.flatnonzero(bx == g), np.flatnonzero(by == g), cap, r, exclude_self)
        for a, b in zip(pi, pj):
            ii.append(a), jj.append(b), dd.append(_d2(x[b], y[a]))
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return _rank_and_cut(np.concatenate(ii), np.concatenate(jj), np.concatenate(dd), cap)


def ref_graph(pos, cap, r=None, batch=None, loop=False, flow="source_to_target"):
    i, j = reference(pos, pos, cap, r, batch, batch, exclude_self=not loop)
    rows = (j, i) if flow == "source_to_target" else (i, j)
    return torch.from_numpy(np.stack(rows).astype(np.int64).reshape(2, -1))


def ref_between(x, y, cap, r=None, batch_x=None, batch_y=None):
    i, j = reference(x, y, cap, r, batch_x, batch_y)
    return torch.from_numpy(np.stack([i, j]).astype(np.int64).reshape(2, -1))


def _np(t):
    return None if t is None else t.cpu().numpy()


def check_graph(pos, cap, r=None, batch=None, loop=False, flow="source_to_target"):
    p, b = pos.to(DEV), None if batch is None else batch.to(DEV)
    if r is None:
        got = dc.nn.knn_graph(p, cap, b, loop=loop, flow=flow)
    else:
        got = dc.nn.radius_graph(p, r, b, loop=loop, max_num_neighbors=cap, flow=flow)
    want = ref_graph(_np(pos), cap, r, _np(batch), loop, flow)
    assert got.dtype == torch.int64 and got.is_contiguous() and got.device == p.device
    print(f"  {'knn' if r is None else 'radius'} N={pos.shape[0]} cap={cap} r={r} loop={loop} {flow}: "
          f"{got.shape[1]} edges (reference {want.shape[1]})")
    assert torch.equal(got.cpu(), want)
    return got


@pytest.fixture(scope="module")
def everyday():
    rest, deff, rig = synth.make_batch(32)
    return rest, deff, rig


# ---------------------------------------------------------------------------------------------------------------- #
# cases
# ---------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("k", [5, 7])
def test_knn_graph_everyday_batch(everyday, k):
    """B = 32 soft meshes and B = 32 rigid UV spheres (symmetric: many equal or nearly equal distances)."""
    rest, _, rig = everyday
    for g in (rest, rig):
        check_graph(g.pos, k, None, g.batch)


def test_radius_graph_everyday_batch(everyday):
    rest, _, rig = everyday
    for g in (rest, rig):
        check_graph(g.pos, 32, 0.15, g.batch)


@pytest.fixture(scope="module")
def cloud100k():
    return synth.radius_graph_points(100_000, 0.02, 32)


def test_radius_graph_configs4_cloud(cloud100k):
    """BASELINE configs[4]: 100,000 points, r = 0.02, cap 32 (cKDTree candidates in the reference)."""
    pos, _ = cloud100k
    check_graph(pos, 32, 0.02)


def test_radius_graph_equals_the_host_builder(cloud100k):
    """Independent cross-check: ``synth.radius_graph_points`` (cKDTree, ranked in float64) on the same cloud, as sets
    of (source, target).  Equal by condition, not tolerance: the fp32 rules give the same 1,118,107 edges for this
    seed (no pair on the radius or the rank-32/33 boundary where float64 and fp32 could disagree)."""
    pos, ei = cloud100k
    got = dc.nn.radius_graph(pos.to(DEV), 0.02, max_num_neighbors=32).cpu()
    a = set(zip(got[0].tolist(), got[1].tolist()))
    b = set(zip(ei[0].tolist(), ei[1].tolist()))
    print(f"  device {len(a)} edges, host builder {len(b)}, differing {len(a ^ b)}")
    assert got.shape[1] == ei.shape[1] == 1_118_107
    assert a == b


def test_knn_and_radius_between_different_sets(everyday):
    """x = the rigid spheres, y = the soft meshes (and the other way round), per graph via batch_x / batch_y."""
    rest, deff, rig = everyday
    for (x, bx), (y, by) in (((rig.pos, rig.batch), (rest.pos, rest.batch)),
                             ((rest.pos, rest.batch), (deff.pos, deff.batch))):
        for k in (1, 7, 64):
            got = dc.nn.knn(x.to(DEV), y.to(DEV), k, bx.to(DEV), by.to(DEV))
            assert torch.equal(got.cpu(), ref_between(x.numpy(), y.numpy(), k, None, bx.numpy(), by.numpy()))
        got = dc.nn.radius(x.to(DEV), y.to(DEV), 0.05, bx.to(DEV), by.to(DEV), max_num_neighbors=20)
        assert torch.equal(got.cpu(), ref_between(x.numpy(), y.numpy(), 20, 0.05, bx.numpy(), by.numpy()))
    # no batch at all: every x is a candidate of every y
    x, y = rig.pos[:3000], rest.pos[:2000]
    got = dc.nn.knn(x.to(DEV), y.to(DEV), 9)
    assert torch.equal(got.cpu(), ref_between(x.numpy(), y.numpy(), 9))
    # graphs present in y only: their queries have no candidates
    by = torch.zeros(y.shape[0], dtype=torch.int64)
    by[1000:] = 1
    bx = torch.zeros(x.shape[0], dtype=torch.int64)
    got = dc.nn.knn(x.to(DEV), y.to(DEV), 4, bx.to(DEV), by.to(DEV))
    assert torch.equal(got.cpu(), ref_between(x.numpy(), y.numpy(), 4, None, bx.numpy(), by.numpy()))
    assert int(got[0].max()) < 1000


def _dup_cloud():
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    p = np.concatenate([p, p[:200], p[100:150]])                    # duplicates, one point three times
    return torch.from_numpy(p)


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_loop_flow_and_duplicate_points(loop, flow):
    pos = _dup_cloud()
    got = check_graph(pos, 6, None, None, loop, flow)
    check_graph(pos, 16, 0.1, None, loop, flow)
    centre = got[1 if flow == "source_to_target" else 0]
    nb = got[0 if flow == "source_to_target" else 1]
    assert bool((centre == nb).any()) == loop                        # j == i only with loop=True
    dup = (centre == 3000) & (nb == 0)                                # point 3000 is a copy of point 0
    assert int(dup.sum()) == 1


def test_small_and_empty_graphs():
    """Graphs with fewer than k + 1 points, a one-point graph, an empty graph inside the batch, N = 0, k = 0."""
    rng = np.random.default_rng(5)
    sizes = (4, 1, 0, 9, 2)
    pos = torch.from_numpy(rng.normal(size=(sum(sizes), 3)).astype(np.float32))
    batch = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes).astype(np.int64))
    for loop in (False, True):
        check_graph(pos, 7, None, batch, loop)
        check_graph(pos, 7, 10.0, batch, loop)
    empty = torch.zeros(0, 3, device=DEV)
    for out in (dc.nn.knn_graph(empty, 5), dc.nn.radius_graph(empty, 0.1), dc.nn.knn(empty, empty, 3),
                dc.nn.knn(pos.to(DEV), empty, 3), dc.nn.knn(empty, pos.to(DEV), 3),
                dc.nn.radius(empty, pos.to(DEV), 1.0), dc.nn.knn_graph(pos.to(DEV), 0),
                dc.nn.radius_graph(pos.to(DEV), 1.0, max_num_neighbors=0),
                dc.nn.knn_graph(pos.to(DEV), 0, batch.to(DEV)),
                dc.nn.knn_graph(empty, 3, torch.zeros(0, dtype=torch.int64, device=DEV))):
        assert out.shape == (2, 0) and out.dtype == torch.int64
    nbr, cnt = neighbors.knn_padded(empty, pos.to(DEV), 3)
    assert nbr.shape == (sum(sizes), 3) and int(cnt.abs().sum()) == 0 and bool((nbr == -1).all())


def test_radius_larger_than_the_extent_and_zero():
    rng = np.random.default_rng(11)
    pos = torch.from_numpy(rng.uniform(-0.2, 0.2, (3000, 3)).astype(np.float32))
    batch = torch.from_numpy(np.repeat(np.arange(3), 1000).astype(np.int64))
    for r in (1.0, 1e6, float("inf")):
        check_graph(pos, 64, r, batch)
    check_graph(pos, 5, 0.0, batch)                                 # d2 < 0 holds for nothing
    check_graph(pos, 5, 0.0, batch, loop=True)


def test_flat_clouds():
    """All points on a plane, and on a line: a zero-width axis of the box (two for the line)."""
    rng = np.random.default_rng(13)
    plane = rng.uniform(0, 1, (4000, 3)).astype(np.float32)
    plane[:, 2] = 0.25
    line = np.zeros((3000, 3), np.float32)
    line[:, 0] = rng.uniform(-1, 1, 3000)
    line[::7, 0] = line[1::7, 0][: line[::7, 0].size]               # repeated coordinates: ties
    for p in (plane, line):
        t = torch.from_numpy(p)
        check_graph(t, 7)
        check_graph(t, 32, 0.05)


def test_offset_coordinates_and_lattice_ties():
    """Coordinates near 1e3 (cell faces met at a coarse ulp) and an integer lattice (exact distance ties; radius 1
    excludes the d2 == 1 neighbours: d2 < r2 is strict)."""
    rng = np.random.default_rng(17)
    p = (1000.0 + rng.uniform(0, 0.5, (3000, 3))).astype(np.float32)
    batch = torch.from_numpy(np.repeat(np.arange(3), 1000).astype(np.int64))
    check_graph(torch.from_numpy(p), 7, None, batch)
    check_graph(torch.from_numpy(p), 32, 0.03, batch)
    g = np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    lat = torch.from_numpy(g)
    check_graph(lat, 7)
    check_graph(lat, 20, 1.5)
    e = check_graph(lat, 20, 1.0)
    assert e.shape[1] == 0
    check_graph(torch.from_numpy(g * np.float32(0.1) - np.float32(500)), 13)


def test_cap_64_is_accepted_65_raises(everyday):
    rest = everyday[0]
    pos, b = rest.pos[:4096], rest.batch[:4096]
    check_graph(pos, 64, None, b)
    check_graph(pos, 64, 0.2, b)
    with pytest.raises(ValueError, match="65"):
        dc.nn.knn_graph(pos.to(DEV), 65, b.to(DEV))
    with pytest.raises(ValueError, match="65"):
        dc.nn.radius_graph(pos.to(DEV), 0.2, b.to(DEV), max_num_neighbors=65)
    with pytest.raises(ValueError, match="65"):
        dc.nn.knn(pos.to(DEV), pos.to(DEV), 65)


def test_row_stride_is_allowed(everyday):
    rest = everyday[0]
    wide = torch.zeros(rest.pos.shape[0], 7)
    wide[:, 2:5] = rest.pos
    got = dc.nn.knn_graph(wide.to(DEV)[:, 2:5], 7, rest.batch.to(DEV))
    assert torch.equal(got, dc.nn.knn_graph(rest.pos.to(DEV), 7, rest.batch.to(DEV)))


# ---------------------------------------------------------------------------------------------------------------- #
# other checks
# ---------------------------------------------------------------------------------------------------------------- #
def test_two_calls_are_bit_identical(everyday, cloud100k):
    pos = cloud100k[0].to(DEV)
    a = dc.nn.radius_graph(pos, 0.02)
    b = dc.nn.radius_graph(pos, 0.02)
    assert torch.equal(a, b)
    rest = everyday[0]
    p, bt = rest.pos.to(DEV), rest.batch.to(DEV)
    for k in (5, 7):
        assert torch.equal(dc.nn.knn_graph(p, k, bt), dc.nn.knn_graph(p, k, bt))


def test_capture_and_replay_on_new_positions(everyday):
    """The no-sync form recorded in torch.cuda.graph, replayed on positions written into the static input, equals the
    eager call (padded array and counts)."""
    rest, deff, _ = everyday
    batch = rest.batch.to(DEV)
    static = rest.pos.to(DEV).clone()

    def run(p):
        a = neighbors.knn_padded(p, p, 7, batch, batch, exclude_self=True)
        b = neighbors.radius_padded(p, p, 0.05, batch, batch, 32, exclude_self=True)
        return a + b
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static)                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(static)
    for new in (deff.pos, rest.pos * 1.5 + 0.1):
        static.copy_(new.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        want = run(new.to(DEV).contiguous())
        for a, b in zip(outs, want):
            assert torch.equal(a, b)
    assert int(outs[1].sum()) == 7 * rest.pos.shape[0]               # every soft mesh has more than 7 points


def test_tagged_knn_graph_feeds_the_segmented_build(everyday):
    """``TAGConv`` over ``knn_graph(pos, 7, batch)`` (which carries the batch layout) equals the same call on an
    untagged copy of the same edge_index, bit for bit; the tagged call builds its adjacency in the one-launch
    segmented build, the copy in the global pipeline (launch log)."""
    rest = everyday[0]
    pos, batch, x = rest.pos.to(DEV), rest.batch.to(DEV), rest.x.to(DEV)
    ei = dc.nn.knn_graph(pos, 7, batch)
    plain = ei.clone()
    torch.manual_seed(0)
    conv = dc.nn.TAGConv(21, 64).to(DEV)
    _lib.kernel_trace(True)
    try:
        ya = conv(x, ei).detach().clone()
        torch.cuda.synchronize()
        tagged = _lib.kernel_trace_counts()
        _lib.kernel_trace(True)
        yb = conv(x, plain).detach().clone()
        torch.cuda.synchronize()
        untagged = _lib.kernel_trace_counts()
    finally:
        _lib.kernel_trace(False)
    assert tagged.get("k_build_segment", 0) >= 1, tagged
    assert untagged.get("k_build_segment", 0) == 0, untagged
    assert torch.equal(ya, yb)
