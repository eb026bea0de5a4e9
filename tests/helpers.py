"""Shared test helpers (tests may import oracle/; the product may not)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def rel_err(a, b):
    """max |a-b| / max |b|  -- the tolerance north_star states is 1e-5 on this."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_rel_err(a, b):
    """max over rows i of  max_j |a_ij - b_ij| / max_j |b_ij|  (rows of b that are all zero are
    compared absolutely against the global scale): stricter than ``rel_err`` for rows whose
    magnitude is far below the tensor's maximum."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    scale = np.abs(b).max(axis=1)
    scale = np.where(scale > 0, scale, max(np.abs(b).max(), 1e-30))
    return float((np.abs(a - b).max(axis=1) / scale).max())


#: every parity comparison of a test run: (test id, tensor, HIP-vs-fp32-oracle distance, did the float64 widening fire,
#: HIP-vs-float64, oracle-vs-float64) - tests/conftest.py writes it to gpurun_out/parity_distances.json at session end
#: ("nothing records how often the widening fires or the worst HIP-vs-fp32-oracle distance")
PARITY_LOG = []


def record_parity(name, d, widened=False, e_h=None, e_o=None, tol=1e-5, metric="rel_err", special=None):
    """``special``: why this comparison is not on north_star's 1e-5 scale (e.g. a gradient that is mathematically zero,
    parameters after several Adam steps) - listed apart and kept out of the summary's worst-case figures."""
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    PARITY_LOG.append({"test": test, "tensor": name, "special": special,
                       "hip_vs_fp32_oracle": None if d is None else float(d),
                       "tol": tol, "metric": metric, "float64_widening_fired": bool(widened),
                       "hip_vs_float64": None if e_h is None else float(e_h),
                       "fp32_oracle_vs_float64": None if e_o is None else float(e_o)})


def three_way(d, e_h_fn, e_o_fn, tol=1e-5, name="", metric="rel_err", special=None, special_bound=None):
    """The parity rule on already computed distances: ``d`` (HIP vs fp32 oracle) < tol, or - evaluated lazily - HIP
    within ``tol`` of the float64 truth (round 5: the ``2 x the oracle's own distance`` allowance is gone; every
    widened comparison of round 4 was within 4.4e-6 of float64).  Only a comparison registered ``special`` (a stated
    reason why it is not on north_star's scale) may pass a wider ``special_bound(e_o)``.  Records the outcome."""
    if d < tol:
        record_parity(name, d, tol=tol, metric=metric, special=special)
        return d
    e_h, e_o = e_h_fn(), e_o_fn()
    record_parity(name, d, True, e_h, e_o, tol=tol, metric=metric, special=special)
    bound = tol if special is None else max(tol, special_bound(e_o))
    assert e_h <= bound, (
        f"{name}: HIP vs fp32 oracle {d:.2e} >= {tol:g}, and vs the float64 truth the HIP path is off by "
        f"{e_h:.2e} > {bound:.2e} (the fp32 oracle is off by {e_o:.2e})")
    return d


def assert_parity(got, ref32, truth64=None, tol=1e-5, name="", metric=None, special=None, special_bound=None):
    """north_star's bar: ``metric(got, fp32 oracle) < tol`` (1e-5).  Where two correct fp32 evaluations legitimately
    differ by more (gradients through several layers: different but equally valid summation orders), the HIP result has
    to be within ``tol`` of a float64 evaluation of the same maths - nothing wider, unless the comparison is registered
    ``special`` with its own stated bound (``three_way``).  Returns the HIP-vs-oracle distance."""
    metric = metric or rel_err
    d = metric(got, ref32)
    if d >= tol:
        assert truth64 is not None, f"{name}: {d:.2e} >= {tol:g} vs the fp32 oracle and no float64 truth given"
    return three_way(d, lambda: metric(got, truth64), lambda: metric(ref32, truth64), tol=tol, name=name,
                     metric=metric.__name__, special=special, special_bound=special_bound)


class G:
    """duck-typed graph batch"""

    def __init__(self, x, edge_index, pos=None):
        self.x, self.edge_index, self.pos = x, edge_index, pos

    def clone(self):
        return G(self.x.clone(), self.edge_index.clone(),
                 None if self.pos is None else self.pos.clone())


def golden_graphs(z, device="cpu"):
    t = lambda k, dt=None: torch.from_numpy(z[k]).to(device)
    rest = G(t("rest_x"), t("rest_edge_index"), t("rest_pos"))
    rig = G(t("rig_x"), t("rig_edge_index"), t("rig_pos"))
    return rest, rig


def random_multigraph(n, e, seed, self_loops=True, isolated=True):
    """edge_index with duplicate edges, self loops and zero-in-degree nodes."""
    rng = np.random.default_rng(seed)
    hi = n - (max(1, n // 10) if isolated else 0)      # last nodes never a target
    src = rng.integers(0, n, e)
    dst = rng.integers(0, max(hi, 1), e)
    if e >= 8:
        src[:4] = src[4:8]                              # duplicates
        dst[:4] = dst[4:8]
        if self_loops:
            src[8:12] = dst[8:12]
    return np.stack([src, dst]).astype(np.int64)


# --------------------------------------------------------------------------- #
# non-finite values (tests/test_nonfinite.py): ONE poison in clean finite inputs.  No tolerance:
# every assertion is isfinite, a float64 equality or torch.equal on bits.
# --------------------------------------------------------------------------- #
#: the three poisons, NaN first (its float64 restatement defines the reach set)
POISONS = (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")))


def poisoned(inputs, name, index, value):
    """A copy of the dict of tensors ``inputs`` with ``inputs[name][index] = value`` (``index``: a tuple; a whole row is
    ``(r,)`` or ``(r, slice(None))``); the other tensors are shared, none is modified."""
    out = dict(inputs)
    t = inputs[name].clone()
    t[index] = value
    out[name] = t
    return out


def reach_sets(ref, inputs64, name, index, value=float("nan")):
    """-> list of bool tensors, one per output of ``ref`` (a float64 restatement: dict of float64 CPU tensors -> list
    of float64 tensors): where the restatement is NON-FINITE with ``value`` placed at ``inputs64[name][index]``.  With
    the NaN poison this is the reach set R."""
    outs = ref(poisoned(inputs64, name, index, value))
    return [~torch.isfinite(o) for o in outs]


def assert_not_swallowed(out, must, what=""):
    """Rule 1: ``out`` (any device / float dtype) is non-finite at every position of the bool mask ``must``."""
    bad = torch.isfinite(out.detach().cpu().float()) & must
    assert not bool(bad.any()), (f"{what}: a non-finite value was swallowed at {int(bad.sum())} of {int(must.sum())} "
                                 f"positions, first {tuple(int(v) for v in bad.nonzero()[0])}")


def assert_contained(out, clean, reach, what=""):
    """Rule 2: outside the reach set ``reach`` the output has the bits of the same kernel's output on the clean inputs."""
    keep = ~reach
    a, b = out.detach().cpu(), clean.detach().cpu()
    assert a.shape == b.shape == keep.shape, (what, a.shape, b.shape, keep.shape)
    a, b = a[keep], b[keep]
    same = torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32))
    if not same:
        diff = (out.detach().cpu() != clean.detach().cpu()) & keep     # (a clean output is finite: != is a bit difference
        raise AssertionError(f"{what}: {int(diff.sum())} positions outside the reach set changed, first "   # up to +-0)
                             f"{tuple(int(v) for v in diff.nonzero()[0]) if diff.any() else 'a sign of zero'}")


def assert_selection(out, ref64, what=""):
    """Rule 3: the output equals the float64 restatement exactly, everywhere (+-Inf compare equal to themselves)."""
    a = out.detach().cpu().double()
    assert a.shape == ref64.shape, (what, a.shape, ref64.shape)
    bad = ~((a == ref64) | (torch.isnan(a) & torch.isnan(ref64)))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} positions differ from the float64 restatement"


def graph_rows(edge_index, n):
    """Rows the poison placements use: a MID row with in-edges and out-edges that is neither row 0 nor the last, and
    the last row.  ``edge_index``: int array [2, E]."""
    src, dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    both = sorted(set(src.tolist()) & set(dst.tolist()) - {0, n - 1})
    mid = both[len(both) // 2] if both else 0
    return mid, n - 1


def element_placements(edge_index, n, f):
    """The placements of a poison in a node-valued [n, f] input: element [0, 0] (padded lanes and tail iterations
    conventionally read element 0: the containment probe), an element of a mid row with in- and out-edges, an
    element of the last row, an element in the last column."""
    mid, last = graph_rows(edge_index, n)
    out = {"first": (0, 0), "mid": (mid, f // 2), "lastrow": (last, min(1, f - 1)), "lastcol": (mid // 2, f - 1)}
    return {k: v for k, v in out.items() if k == "first" or n > 1}


def edge_placements(edge_index, c, unroll=8):
    """The placements of a poison in an edge-valued [E, c] input: edge 0, and the last input edge of a destination
    whose in-degree is not a multiple of the kernels' unroll (its tail iteration is partly predicated off)."""
    dst = np.asarray(edge_index[1])
    out = {"edge0": (0, 0)}
    deg = np.bincount(dst)
    odd = [d for d in np.nonzero(deg % unroll)[0] if deg[d] >= 2]
    if odd:
        d = odd[len(odd) // 2]
        out["segtail"] = (int(np.nonzero(dst == d)[0][-1]), c - 1)
    return out


def linear_spline_basis(a, kernel_size, is_open):
    """The degree-1 B-spline basis of SplineConv in float32, as the kernel forms it: for
    pseudo-coordinates ``a`` [E, D] in [0, 1] -> (b float32 [E, 2^D], wi int64 [E, 2^D]).  Per dimension ``v = a_d *
    (kernel_size_d - open_d)``, ``f = v - floor(v)``; slot ``s`` takes digit ``k_d = (s >> d) & 1`` (dimension 0 runs
    fastest), the factor ``1 - f - k_d + 2 f k_d`` and the index digit ``(floor(v) + k_d) mod kernel_size_d``."""
    a = np.asarray(a, np.float32).reshape(len(a), -1)
    dim = a.shape[1]
    slots = np.arange(2 ** dim)
    b = np.ones((a.shape[0], len(slots)), np.float32)
    wi = np.zeros(b.shape, np.int64)
    off = 1
    for d in range(dim):
        v = a[:, d] * np.float32(kernel_size[d] - int(bool(is_open[d])))
        fl = np.floor(v)
        f = (v - fl).astype(np.float32)[:, None]
        k = ((slots >> d) & 1)[None]
        wi += ((fl.astype(np.int64)[:, None] + k) % kernel_size[d]) * off
        off *= kernel_size[d]
        kf = k.astype(np.float32)
        b = (b * (1 - f - kf + 2 * f * kf)).astype(np.float32)
    return b, wi
