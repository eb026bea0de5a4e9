"""The width-F kNN rule restated in numpy, and the inputs of its tests (tests/test_neighbors_nd*.py,
tests/test_dynamic_edge_conv.py).  Not the code under test: an explicit float32 loop over the columns for ``d2`` (one
rounding per difference, product and sum, in column order), ``np.lexsort((j, d2, i))`` and a cut at the cap."""
import numpy as np

from deformcontact_amd import neighbors

W = neighbors.ND_CHUNK            # the kernel's column chunk: widths around it take different code paths
WIDTHS = [1, 2, 3, 4, 5, W - 1, W, W + 1, 2 * W + 2]
ONE_GRAPH_N = [1, 2, 5, 63, 64, 65, 300]
ONE_GRAPH_K = [0, 1, 5, 20, 64]
RAGGED = [1, 5, 64, 130, 67]      # node counts of the ragged batch; one graph id is skipped


def d2_columns(xc, yq):
    """[q, n] float32: d2 = d_0*d_0, then d2 = d2 + d_c*d_c in column order, d_c = x[j, c] - y[i, c]"""
    assert xc.dtype == np.float32 and yq.dtype == np.float32
    d = xc[None, :, 0] - yq[:, None, 0]
    d2 = d * d
    for c in range(1, xc.shape[1]):
        d = xc[None, :, c] - yq[:, None, c]
        d2 = d2 + d * d
    assert d2.dtype == np.float32
    return d2


def knn_ref(x, y, k, bx=None, by=None, exclude_self=False):
    """-> (nbr [ny, k] int32: rank order then -1, counts [ny] int32)"""
    nx, ny = x.shape[0], y.shape[0]
    bx = np.zeros(nx, np.int64) if bx is None else bx
    by = np.zeros(ny, np.int64) if by is None else by
    nbr = np.full((ny, k), -1, np.int32)
    counts = np.zeros(ny, np.int32)
    for g in np.unique(by):
        xi, yi = np.flatnonzero(bx == g), np.flatnonzero(by == g)
        if xi.size == 0 or k == 0:
            continue
        d2 = d2_columns(x[xi], y[yi])
        keep = np.ones(d2.shape, bool)
        if exclude_self:
            keep &= xi[None, :] != yi[:, None]
        qi, cj = np.nonzero(keep)
        i, j, d = yi[qi], xi[cj], d2[qi, cj]
        o = np.lexsort((j, d, i))
        i, j = i[o], j[o]
        if i.size == 0:
            continue
        starts = np.r_[0, np.flatnonzero(np.diff(i)) + 1]
        rank = np.arange(i.size) - np.repeat(starts, np.diff(np.r_[starts, i.size]))
        cut = rank < k
        nbr[i[cut], rank[cut]] = j[cut]
        counts[:] += np.bincount(i[cut], minlength=ny).astype(np.int32)
    return nbr, counts


def edges_ref(nbr, counts, query_row):
    """the [2, M] int64 edge list of a padded result: grouped by query, rank order; row ``query_row`` = the query"""
    q, t = np.nonzero(np.arange(nbr.shape[1])[None, :] < counts[:, None])
    out = np.empty((2, q.size), np.int64)
    out[query_row], out[1 - query_row] = q, nbr[q, t]
    return out


def expected_counts(k, bx, by, nx, ny, exclude_self):
    """min(k, n_g), or min(k, n_g - 1) where the query itself is a candidate that is dropped"""
    bx = np.zeros(nx, np.int64) if bx is None else bx
    by = np.zeros(ny, np.int64) if by is None else by
    n_g = np.array([(bx == g).sum() for g in by], np.int64).reshape(-1)
    own = np.array([exclude_self and i < nx and bx[i] == by[i] for i in range(ny)], bool).reshape(-1)
    return np.minimum(k, n_g - own).astype(np.int32)


def batch_of(counts, skip=None):
    """sorted graph ids for graphs of these sizes; ``skip``: an id left out (an empty graph in between)"""
    ids = [g if skip is None or g < skip else g + 1 for g in range(len(counts))]
    return np.repeat(np.array(ids, np.int64), counts)


def _case(x, k, y=None, bx=None, by=None, exclude_self=False, same=None):
    same = y is None if same is None else same
    y = x if y is None else y
    by = bx if same and by is None else by
    return dict(x=x, y=y, k=k, bx=bx, by=by, exclude_self=exclude_self, same=same)


def tie_inputs(rng, n=150, f=W + 1):
    """the tie-rich inputs post-ReLU features produce: name -> x"""
    half = rng.standard_normal((n // 2, f)).astype(np.float32)
    sparse = rng.standard_normal((n, f)).astype(np.float32)
    sparse[rng.random((n, f)) < 0.5] = 0.0
    return {"zeros": np.zeros((n, f), np.float32),
            "twice": np.concatenate([half, half])[rng.permutation(2 * (n // 2))],
            "small_int": rng.integers(0, 3, (n, f)).astype(np.float32),
            "half_zero": sparse}


def cases():
    """name -> case dict (x, y, k, bx, by, exclude_self; numpy).  Every input of tests/test_neighbors_nd.py that is
    compared against ``knn_ref``; deterministic."""
    rng = np.random.default_rng(20250)
    out = {}
    for f in WIDTHS:                                                # two graphs, both settings of exclude_self
        x = rng.standard_normal((130, f)).astype(np.float32)
        for ex in (False, True):
            out[f"width{f}-ex{int(ex)}"] = _case(x, 20, bx=batch_of([70, 60]), exclude_self=ex)
    for n in ONE_GRAPH_N:
        x = rng.standard_normal((n, W + 1)).astype(np.float32)
        for k in ONE_GRAPH_K:
            for ex in (False, True):
                out[f"one-n{n}-k{k}-ex{int(ex)}"] = _case(x, k, exclude_self=ex)
    x = rng.standard_normal((sum(RAGGED), W + 1)).astype(np.float32)
    for ex in (False, True):
        out[f"ragged-ex{int(ex)}"] = _case(x, 20, bx=batch_of(RAGGED, skip=2), exclude_self=ex)
    # knn(x, y): nx != ny, graph 1 present in y only (no neighbour), graph 3 in x only
    x = rng.standard_normal((40 + 90 + 33, 7)).astype(np.float32)
    y = rng.standard_normal((50 + 21 + 100, 7)).astype(np.float32)
    out["xy"] = _case(x, 20, y=y, bx=np.repeat(np.array([0, 2, 3], np.int64), [40, 90, 33]),
                      by=np.repeat(np.array([0, 1, 2], np.int64), [50, 21, 100]))
    out["xy-no-batch"] = _case(x, 5, y=y)
    for name, x in tie_inputs(rng).items():
        for ex in (False, True):
            out[f"ties-{name}-ex{int(ex)}"] = _case(x, 20, bx=batch_of([x.shape[0] - 50, 50]), exclude_self=ex)
    return out
