"""The arithmetic of the fp16x2 ("h2") dense kernels restated in numpy, float64 inside.

An operand row (or tensor, or node chunk) with reference magnitude ``ref`` is multiplied by the exact power of two
``2^(141 - e)``, ``e`` = biased fp32 exponent of ``ref`` clamped to [15, 254] (``h2_exp`` / ``h2_scale`` of
``csrc/dc_dense.h``), written as two fp16 planes ``h = fp16(x)``, ``l = fp16(x - h)`` (``split4_h2``), multiplied as
``h.h + h.l + l.h`` with fp32 accumulation, and multiplied back by ``2^(e - 141)`` per operand (``h2_unscale``).
Everything but the order and rounding of the fp32 accumulation is therefore a function of the inputs alone:

  * ``planes`` / ``product``  the planes and the three plane products summed in float64 - what the kernel would give with
                              an exact accumulator (``exact``), and the same sum over absolute values (``S``), the
                              natural unit of its accumulation error;
  * ``restated_fp32``         the same planes accumulated in fp32, in k order - a yardstick for the accumulation error;
  * ``apriori_bound``         how far ``exact`` can be from the float64 product of the unsplit operands, for any valid
                              reference up to a given one.

Operands are row-major with the reduction LAST: ``a [M, K]``, ``b [N, K]``, result ``[M, N]`` (forward: x and W; dX: g and
W^T; dW: g^T and x^T).  References are scalars or one per row.
"""
import numpy as np

F16_DENORMAL_STEP = 2.0 ** -24


def h2_exp(ref):
    """Biased fp32 exponent of ``ref`` clamped to [15, 254] (int64 array)."""
    bits = np.ascontiguousarray(ref, dtype=np.float32).view(np.uint32)
    return np.clip((bits >> 23) & 0xFF, 15, 254).astype(np.int64)


def h2_scale(ref):
    return np.ldexp(1.0, 141 - h2_exp(ref))


def h2_unscale(ref):
    return np.ldexp(1.0, h2_exp(ref) - 141)


def _per_row(ref, rows):
    ref = np.asarray(ref, dtype=np.float32)
    return np.broadcast_to(ref.reshape(-1), (rows,)) if ref.ndim else np.full(rows, ref, np.float32)


def planes(a, ref):
    """(h, l, unscale): the fp16 planes of ``a * h2_scale(ref)`` and the per-row factor that undoes the scale."""
    a = np.asarray(a, dtype=np.float32)
    assert a.ndim == 2
    ref = _per_row(ref, a.shape[0])
    sc = h2_scale(ref)[:, None]
    with np.errstate(over="raise"):
        x64 = a.astype(np.float64) * sc
        x = x64.astype(np.float32)
    # the scaling is exact in fp32 - or the value lies below fp32's normal range, 2^100 times below the fp16 grid, where
    # both planes are (signed) zeros however fp32 rounds or flushes it
    normal = np.abs(x64) >= 2.0 ** -126
    assert np.array_equal(x.astype(np.float64)[normal], x64[normal]), "a * scale is not exact in fp32"
    h = x.astype(np.float16)                                   # round to nearest even, as v_cvt_f16_f32
    assert np.isfinite(h).all(), "the reference is no upper bound: the scaled operand leaves the fp16 range"
    l = (x - h.astype(np.float32)).astype(np.float16)          # the remainder is exact in fp32
    return h, l, h2_unscale(ref)


def _sum3(ha, la, hb, lb, absolute=False):
    ha, la, hb, lb = (np.asarray(p, np.float64) for p in (ha, la, hb, lb))
    if absolute:
        ha, la, hb, lb = np.abs(ha), np.abs(la), np.abs(hb), np.abs(lb)
    return la @ hb.T + ha @ lb.T + ha @ hb.T


def product_of_planes(pa, pb):
    """(exact, S) from two ``planes`` results."""
    (ha, la, ua), (hb, lb, ub) = pa, pb
    u = ua[:, None] * ub[None, :]
    return _sum3(ha, la, hb, lb) * u, _sum3(ha, la, hb, lb, True) * u


def product(a, aref, b, bref):
    """(exact, S): hh + hl + lh summed in float64 and unscaled; the same sum over absolute values."""
    return product_of_planes(planes(a, aref), planes(b, bref))


def restated_fp32_of_planes(pa, pb, step=8):
    (ha, la, ua), (hb, lb, ub) = pa, pb
    ha, la, hb, lb = (np.asarray(p, np.float64) for p in (ha, la, hb, lb))
    acc = np.zeros((ha.shape[0], hb.shape[0]), np.float32)
    for k in range(0, ha.shape[1], step):
        s = slice(k, k + step)
        for x, y in ((la, hb), (ha, lb), (ha, hb)):           # smallest terms first, as the kernels issue them
            acc = (acc.astype(np.float64) + x[:, s] @ y[:, s].T).astype(np.float32)
    return acc.astype(np.float64) * (ua[:, None] * ub[None, :])


def restated_fp32(a, aref, b, bref, step=8):
    """The same planes accumulated in fp32 in k order, ``step`` at a time, three products per step (each group of
    ``step`` products exact, one rounding per group: a matrix-core instruction)."""
    return restated_fp32_of_planes(planes(a, aref), planes(b, bref), step)


def chunked(fn, g, gref, x, xref, chunk_rows):
    """dW: sum over node chunks of ``fn(g_c^T, max gref_c, x_c^T, max xref_c)`` - one scale per operand and chunk.
    ``fn`` is ``product`` (returns the pair summed component-wise) or ``restated_fp32``."""
    n = g.shape[0]
    gref, xref = _per_row(gref, n), _per_row(xref, n)
    total = None
    for c in range(0, n, chunk_rows):
        s = slice(c, min(c + chunk_rows, n))
        r = fn(g[s].T, gref[s].max(), x[s].T, xref[s].max())
        total = r if total is None else (tuple(p + q for p, q in zip(total, r)) if isinstance(r, tuple) else total + r)
    return total


def _rep(x, unscale_max):
    """Per element: (|x^ - x| <=, |l| <=) for x^ = h + l at any scale whose unscale factor is <= unscale_max."""
    ax = np.abs(np.asarray(x, np.float64))
    floor = F16_DENORMAL_STEP * unscale_max[:, None]
    nz = ax > 0
    return np.where(nz, np.maximum(2.0 ** -22 * ax, floor), 0.0), np.where(nz, np.maximum(2.0 ** -11 * ax, floor), 0.0)


def apriori_bound(a, aref_max, b, bref_max):
    """Component-wise bound on |exact - a b^T| (float64 product of the unsplit operands) for ANY valid references - upper
    bounds of the rows' magnitudes - that are not above ``aref_max`` / ``bref_max``.

    Derivation, in the operand's own units (u = h2_unscale(ref), x' = x / u the scaled value, |x'| < 2^15):
      * h = fp16(x') has 11 significant bits: r = x' - h is exact in fp32 and |r| <= 2^-11 |x'| (half an ulp of h, the
        ulp taken in x's binade; below 2^-14 the fp16 grid is 2^-24 wide and |r| <= 2^-25).
      * l = fp16(r): rounding is monotone and both bounds of r are fp16 numbers, so |l| <= max(2^-11 |x'|, 2^-24); its
        own rounding error is at most 2^-11 |r| <= 2^-22 |x'|, or half a denormal step, 2^-25.
      So x^ = (h + l) u satisfies |x^ - x| <= d(x) := max(2^-22 |x|, 2^-24 u) and |l u| <= m(x) := max(2^-11 |x|, 2^-24 u);
      x = 0 gives h = l = 0.  Both grow with u, u grows with the reference, so evaluating them at the largest admissible
      reference bounds every smaller one: the bound cannot grow when a reference shrinks.
      * the kernel's sum is sum_k (a^ b^ - la lb):  |a^ b^ - a b| <= |a| d(b) + |b| d(a) + d(a) d(b), and the dropped
        term is at most m(a) m(b).
    The fp32 accumulation error comes on top of this and is bounded separately (tests: (3K + chunks + 2) 2^-23 S)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    da, ma = _rep(a, h2_unscale(_per_row(aref_max, a.shape[0])))
    db, mb = _rep(b, h2_unscale(_per_row(bref_max, b.shape[0])))
    return np.abs(a) @ db.T + da @ np.abs(b).T + da @ db.T + ma @ mb.T


# ---- the bf16 split forms of dc_dense_split.hip (the first layers' arithmetic) ----------------------------------------
#: plane pairs (of a, of b) in the order `mma_split` issues them; 0 = hi, 1 = mid, 2 = lo
BF16_PRODUCTS = {6: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)), 3: ((1, 0), (0, 1), (0, 0)), 1: ((0, 0),)}


def planes_bf16(a):
    """`split1`: x = hi + mid + lo, each the bf16 (round to nearest even) of what the ones before it left - exactly, unless
    a remainder falls below bf16's (= fp32's) denormal range.  Returns float64 arrays."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    hi = x.to(torch.bfloat16).float()
    r = x - hi                                                  # exact
    mid = r.to(torch.bfloat16).float()
    lo = (r - mid).to(torch.bfloat16).float()
    return tuple(t.double().numpy() for t in (hi, mid, lo))


def product_bf16(a, b, products):
    """(exact, S) of the 6- / 3- / 1-product form: the plane products of BF16_PRODUCTS summed in float64."""
    pa, pb = planes_bf16(a), planes_bf16(b)
    exact = sum(pa[i] @ pb[j].T for i, j in BF16_PRODUCTS[products])
    return exact, sum(np.abs(pa[i]) @ np.abs(pb[j]).T for i, j in BF16_PRODUCTS[products])


def restated_bf16_fp32(a, b, products, step=8):
    """the same plane products accumulated in fp32 in k order, ``step`` at a time (cf. ``restated_fp32``)"""
    pa, pb = planes_bf16(a), planes_bf16(b)
    acc = np.zeros((pa[0].shape[0], pb[0].shape[0]), np.float32)
    for k in range(0, pa[0].shape[1], step):
        s = slice(k, k + step)
        for i, j in BF16_PRODUCTS[products]:
            acc = (acc.astype(np.float64) + pa[i][:, s] @ pb[j][:, s].T).astype(np.float32)
    return acc.astype(np.float64)


def apriori_bound_bf16(a, b, products):
    """|exact - a b^T| <= c sum |a||b| component-wise: hi keeps 8 significant bits, so |mid| <= 2^-8 |x| and
    |lo| <= 2^-16 |x| (half an ulp of the plane before), and hi + mid + lo = x exactly (24 bits and the signs of the
    remainders; operands are assumed far above the denormal range).  The error is the sum of the dropped plane products:
    6: mid lo + lo mid + lo lo <= 2 2^-24 + 2^-32;   3: those + hi lo + lo hi + mid mid <= 3 2^-16 (1 + 2^-7);
    1: everything but hi hi <= 2 2^-8 (1 + 2^-7)."""
    c = {6: 2.0 ** -23 + 2.0 ** -32, 3: 3 * 2.0 ** -16 * (1 + 2.0 ** -7), 1: 2.0 ** -7 * (1 + 2.0 ** -7)}[products]
    return c * (np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)).T)


# ---- the regimes the tests of this family share -----------------------------------------------------------------------
def uniform(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).uniform(-1.0, 1.0, shape) * scale).astype(np.float32)


def pow2_rows(n, log2_span, descending=False):
    """[n, 1] fp32 row factors on a log-spaced scale over 2^log2_span (the largest is 1)."""
    t = np.linspace(-float(log2_span), 0.0, n) if n > 1 else np.zeros(1)
    f = np.exp2(t).astype(np.float32)
    return (f[::-1] if descending else f).reshape(n, 1).copy()


REGIMES = ("flat", "rows_2^20", "anti_2^30", "spike_vs_zero")


def make_case(regime, m, k, n, seed):
    """(a [m, k], b [n, k]) fp32 for one regime.  ``rows_2^20``: the rows of ``a`` on log-spaced scales over 2^20;
    ``anti_2^30``: the reduction index scaled over 2^30 in ``a`` and the other way round in ``b`` (what a shared scale
    over the reduction loses most on - beyond the accuracy envelope, the model must still be matched);
    ``spike_vs_zero``: one row of ``a`` 2^20 above the rest and one row of ``b`` all zero."""
    a, b = uniform((m, k), seed), uniform((n, k), seed + 1, 1.0 / np.sqrt(k))
    if regime == "rows_2^20":
        a = a * pow2_rows(m, 20)
    elif regime == "anti_2^30":
        a = a * pow2_rows(k, 30).T
        b = b * pow2_rows(k, 30, descending=True).T
    elif regime == "spike_vs_zero":
        a[m // 2] *= np.float32(2.0 ** 20)
        b[n // 2] = 0.0
    else:
        assert regime == "flat", regime
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def rowmax(a):
    return np.abs(np.asarray(a, np.float32)).max(axis=1)


def anti_correlated(n, fo, fi, log2_spread, seed=7):
    """dW operands whose node rows are anti-correlated: g rows fall over 2^log2_spread while x rows rise."""
    g = uniform((n, fo), seed) * pow2_rows(n, log2_spread, descending=True)
    x = uniform((n, fi), seed + 1) * pow2_rows(n, log2_spread)
    return g.astype(np.float32), x.astype(np.float32)
