"""GPU: kNN over rows of any width (``neighbors.knn_padded_nd``, csrc/dc_neighbors_nd.hip) against the numpy
restatement of its rule in tests/nd_reference.py, bit for bit: an explicit float32 loop over the columns for ``d2``,
``np.lexsort((j, d2, i))``, a cut at the cap.  Every comparison is ``torch.equal`` on the padded neighbour array, the
counts or the ``[2, M]`` edge index; nothing is tolerance-based.

Shapes are the smallest at which the kernel can go wrong: widths 1..5 and around the kernel's column chunk
(``neighbors.ND_CHUNK``: W-1, W, W+1, 2W+2), graphs below, at and above one 64-candidate tile and one 32-query
workgroup, a ragged batch whose workgroups straddle graph borders, ``knn(x, y)`` with a graph that has no candidates,
tie-rich inputs, a strided operand, the three-column grid path as a second witness, one DGCNN-sized batch."""
import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import neighbors
from deformcontact_amd.graph import edge_layout
from tests import nd_reference as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = ref.cases()


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _run(c, fn=None):
    fn = fn or neighbors.knn_padded_nd
    x = _dev(c["x"])
    y = x if c["same"] else _dev(c["y"])
    bx = _dev(c["bx"])
    by = bx if c["same"] else _dev(c["by"])
    return fn(x, y, c["k"], bx, by, exclude_self=c["exclude_self"])


def _assert_case(c, name, fn=None):
    nbr, counts = _run(c, fn)
    rn, rc = ref.knn_ref(c["x"], c["y"], c["k"], c["bx"], c["by"], c["exclude_self"])
    assert nbr.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(nbr.shape) == rn.shape
    assert torch.equal(counts.cpu(), torch.from_numpy(rc)), name
    assert torch.equal(nbr.cpu(), torch.from_numpy(rn)), name
    return nbr, counts


@pytest.mark.parametrize("f", ref.WIDTHS)
def test_every_width_matches_the_column_loop(f):
    for ex in (0, 1):
        _assert_case(CASES[f"width{f}-ex{ex}"], f"width {f}")
    if f != 3:                                                      # knn_padded sends every width but 3 here
        _assert_case(CASES[f"width{f}-ex1"], f"width {f} through knn_padded", fn=neighbors.knn_padded)


@pytest.mark.parametrize("n", ref.ONE_GRAPH_N)
def test_one_graph_below_at_and_above_a_tile(n):
    for k in ref.ONE_GRAPH_K:
        for ex in (0, 1):
            name = f"one-n{n}-k{k}-ex{ex}"
            _, counts = _assert_case(CASES[name], name)
            assert int(counts.max()) == min(k, n - ex)


@pytest.mark.parametrize("ex", [0, 1])
def test_ragged_batch_with_an_empty_graph(ex):
    c = CASES[f"ragged-ex{ex}"]
    _, counts = _assert_case(c, "ragged")
    want = ref.expected_counts(20, c["bx"], c["bx"], c["x"].shape[0], c["x"].shape[0], bool(ex))
    assert torch.equal(counts.cpu(), torch.from_numpy(want))
    assert sorted(set(want.tolist())) == sorted({min(20, n - ex) for n in ref.RAGGED})


def test_knn_of_two_sets():
    c = CASES["xy"]
    _, counts = _assert_case(c, "xy")
    assert int(counts[50:71].sum()) == 0                            # graph 1 has no point in x
    _assert_case(CASES["xy-no-batch"], "xy without batch vectors")
    # the PyG-shaped function: row 0 indexes y, row 1 indexes x
    ei = dc.nn.knn(_dev(c["x"]), _dev(c["y"]), c["k"], _dev(c["bx"]), _dev(c["by"]))
    want = ref.edges_ref(*ref.knn_ref(c["x"], c["y"], c["k"], c["bx"], c["by"]), 0)
    assert ei.dtype == torch.int64 and torch.equal(ei.cpu(), torch.from_numpy(want))
    # one batch vector only: the other side is "all in graph 0"
    x, y = _dev(c["x"]), _dev(c["y"])
    for bx, by in ((c["bx"], None), (None, c["by"])):
        nbr, counts = neighbors.knn_padded_nd(x, y, 5, _dev(bx), _dev(by))
        rn, rc = ref.knn_ref(c["x"], c["y"], 5, bx, by)
        assert torch.equal(nbr.cpu(), torch.from_numpy(rn)) and torch.equal(counts.cpu(), torch.from_numpy(rc))


@pytest.mark.parametrize("kind", ["zeros", "twice", "small_int", "half_zero"])
def test_ties_rank_by_index(kind):
    for ex in (0, 1):
        c = CASES[f"ties-{kind}-ex{ex}"]
        nbr, _ = _assert_case(c, f"ties {kind}")
        if kind == "zeros" and not ex:                              # the rank is j alone
            first = int(np.flatnonzero(c["bx"] == 1)[0])
            assert nbr[0].tolist() == list(range(20)) and nbr[-1].tolist() == list(range(first, first + 20))
        if kind == "twice" and ex:                                  # the duplicate j != i stays, at distance 0
            x = c["x"]
            twin = [int(np.flatnonzero((x == x[i]).all(1) & (np.arange(x.shape[0]) != i))[0]) for i in (0, 149)]
            same_graph = [c["bx"][t] == c["bx"][i] for t, i in zip(twin, (0, 149))]
            for t, i, s in zip(twin, (0, 149), same_graph):
                assert (int(nbr[i, 0]) == t) == bool(s)


def test_a_column_slice_is_taken_as_it_is():
    c = CASES["ragged-ex1"]
    f = c["x"].shape[1]
    buf = torch.full((c["x"].shape[0], f + 3), 1.0e6, device=DEV)
    x = buf[:, 2:2 + f]
    x.copy_(_dev(c["x"]))
    assert x.stride() == (f + 3, 1)
    bx = _dev(c["bx"])
    nbr, counts = neighbors.knn_padded_nd(x, x, 20, bx, bx, exclude_self=True)
    rn, rc = ref.knn_ref(c["x"], c["x"], 20, c["bx"], c["bx"], True)
    assert torch.equal(nbr.cpu(), torch.from_numpy(rn)) and torch.equal(counts.cpu(), torch.from_numpy(rc))
    # a strided y against a contiguous x
    nbr2, counts2 = neighbors.knn_padded_nd(x.contiguous(), x, 20, bx, bx, exclude_self=True)
    assert torch.equal(nbr2, nbr) and torch.equal(counts2, counts)


def test_three_columns_equal_the_grid_path():
    rng = np.random.default_rng(7)
    pts = rng.standard_normal((2000, 3)).astype(np.float32)
    half = rng.standard_normal((75, 3)).astype(np.float32)
    twice = np.concatenate([half, half])[rng.permutation(150)]
    for pos, b in ((pts, ref.batch_of([700, 900, 400])), (twice, ref.batch_of([100, 50]))):
        x, bx = _dev(pos), _dev(b)
        for ex in (False, True):
            grid = neighbors.knn_padded(x, x, 20, bx, bx, exclude_self=ex)
            brute = neighbors.knn_padded_nd(x, x, 20, bx, bx, exclude_self=ex)
            assert torch.equal(grid[0], brute[0]) and torch.equal(grid[1], brute[1])
    rn, rc = ref.knn_ref(twice, twice, 20, b, b, True)
    assert torch.equal(brute[0].cpu(), torch.from_numpy(rn)) and torch.equal(brute[1].cpu(), torch.from_numpy(rc))


def test_dgcnn_sized_knn_graph_carries_the_batch_layout():
    rng = np.random.default_rng(11)
    feats = np.maximum(rng.standard_normal((4 * 256, 64)), 0).astype(np.float32)     # post-ReLU: many zeros
    b = ref.batch_of([256] * 4)
    x, batch = _dev(feats), _dev(b)
    conv = dc.nn.EdgeConv(torch.nn.Linear(128, 16)).to(DEV)
    for loop in (False, True):
        nbr, counts = ref.knn_ref(feats, feats, 20, b, b, exclude_self=not loop)
        assert int(counts.min()) == 20
        for flow, row in (("source_to_target", 1), ("target_to_source", 0)):
            ei = dc.nn.knn_graph(x, 20, batch, loop=loop, flow=flow)
            assert torch.equal(ei.cpu(), torch.from_numpy(ref.edges_ref(nbr, counts, row)))
            seg = edge_layout(ei)
            assert seg is not None and tuple(seg[0]) == (0, 256, 512, 768, 1024)
            assert tuple(seg[1]) == tuple(range(0, 5 * 5120, 5120))
            if flow == "source_to_target":                          # a layer takes the tagged list as a plain copy
                plain = ei.clone()
                assert edge_layout(plain) is None
                assert torch.equal(conv(x, ei), conv(x, plain))
    assert torch.equal(dc.nn.knn_graph(x, 20, loop=True).cpu(),
                       torch.from_numpy(ref.edges_ref(*ref.knn_ref(feats, feats, 20), 1)))


def test_two_calls_are_bit_identical_and_empty_inputs_give_empty_results():
    c = CASES["ties-half_zero-ex0"]
    a, b = _run(c), _run(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    x = _dev(c["x"])
    none = torch.empty(0, x.size(1), device=DEV)
    nbr, counts = neighbors.knn_padded_nd(none, x, 5)               # no candidates: every count 0
    assert int(counts.abs().sum()) == 0 and bool((nbr == -1).all())
    nbr, counts = neighbors.knn_padded_nd(x, none, 5)
    assert tuple(nbr.shape) == (0, 5) and tuple(counts.shape) == (0,)
    nbr, counts = neighbors.knn_padded_nd(x, x, 0, _dev(c["bx"]), _dev(c["bx"]))
    assert tuple(nbr.shape) == (x.size(0), 0) and int(counts.abs().sum()) == 0
    assert tuple(dc.nn.knn_graph(x, 0, _dev(c["bx"])).shape) == (2, 0)
    assert tuple(dc.nn.knn_graph(none, 5).shape) == (2, 0)
