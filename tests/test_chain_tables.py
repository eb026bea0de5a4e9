"""The hop chain's adjacency tables as an image written by the segmented build (``dc_graph_build_segmented_image``) and
read by ``dc_hop_chain_image_f32`` instead of being derived from ``ptr`` / ``other`` / ``deg_ptr`` in every workgroup.
The bar: the image holds exactly the tables computed in numpy from the finished adjacency (``dis`` bit for bit), nothing
around it is written, and a chain that reads it leaves the same blocks and row maxima, bit for bit, as the chain that
builds its tables itself and as K single ``dc_spmm_f32`` hops - eagerly and in a replayed hipGraph, also when the build
has flagged an edge."""
import ctypes

import numpy as np
import pytest
import torch

from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import SortedAdjacency, current_stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0x5ca1ab1e
PAD = 0xffff

# 1,024: the last slice row and the row of zeros meet; an empty graph in the middle; 7 / 130 / 257: no multiples of 8
SIZES_8 = (7, 130, 0, 1024, 1, 257)
SIZES_2 = (256, 100, 0, 33)                       # largest graph 256 nodes: k_hop_chain_gcn<2>
SIZES_7 = (800, 513, 5)                           # largest graph 800 nodes: k_hop_chain_gcn<7>


def make_batch(sizes, seed):
    """Block-diagonal batch of symmetric graphs (every edge in both directions, so in- and out-degrees agree and both
    sides see the same degrees): a ring over all but the last 8 nodes (those keep degree 0), nodes 10 / 30 / 50 of every
    graph of >= 130 nodes brought to degree 8 / 9 / 17, random pairs among the other nodes; edges shuffled per graph.
    The edge COUNT of a graph depends on its size alone: batches of different seeds share their layout."""
    rng = np.random.default_rng(seed)
    srcs, dsts, nptr, eptr = [], [], [0], [0]
    for n in sizes:
        u, v = [], []
        m = n - 8 if n >= 130 else n
        if m >= 3:
            u += list(range(m))
            v += [(i + 1) % m for i in range(m)]
        if n >= 130:
            nxt = 64
            for hubnode, deg in ((10, 8), (30, 9), (50, 17)):
                for _ in range(deg - 2):
                    u.append(hubnode), v.append(nxt)
                    nxt += 1
            a = rng.integers(96, m, 2 * n)
            b = rng.integers(96, m, 2 * n)
            b = np.where(a == b, (b - 96 + 1) % (m - 96) + 96, b)
            u += a.tolist()
            v += b.tolist()
        u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
        s, t = np.concatenate([u, v]), np.concatenate([v, u])
        order = rng.permutation(len(s))
        srcs.append(s[order] + nptr[-1]), dsts.append(t[order] + nptr[-1])
        nptr.append(nptr[-1] + n), eptr.append(eptr[-1] + len(s))
    ei = np.stack([np.concatenate(srcs), np.concatenate(dsts)]).astype(np.int64)
    return ei, tuple(nptr), tuple(eptr)


class Built:
    """The arrays of one ``dc_graph_build_segmented_image`` call; each image sits between two canary words."""

    def __init__(self, ei, nptr, eptr, edge_buffer=None):
        L = _lib.lib()
        self.n, self.e, self.nseg = nptr[-1], eptr[-1], len(nptr) - 1
        self.nptr, self.eptr = nptr, eptr
        self.c_nptr, self.c_eptr = (ctypes.c_int64 * len(nptr))(*nptr), (ctypes.c_int64 * len(eptr))(*eptr)
        self.ei = edge_buffer if edge_buffer is not None else torch.from_numpy(ei).to(DEV)
        i32 = dict(dtype=torch.int32, device=DEV)
        self.sides = [SortedAdjacency(torch.empty(self.n + 1, **i32), torch.empty(self.e, **i32), torch.empty(self.e, **i32),
                                      torch.empty(self.e, dtype=torch.float32, device=DEV)) for _ in range(2)]
        self.nbytes = int(L.dc_hop_chain_image_bytes(self.n))
        assert self.nbytes >= 28 * self.n + 4 and self.nbytes % 16 == 0
        self.raw = [torch.full((self.nbytes // 4 + 8,), CANARY, **i32) for _ in range(2)]      # 16 B | image | 16 B
        self.images = [r[4:4 + self.nbytes // 4] for r in self.raw]
        self.status = torch.zeros(1, **i32)

    def build(self):
        f, b = self.sides
        rc = _lib.lib().dc_graph_build_segmented_image(
            self.ei.data_ptr(), self.e, self.n, self.c_nptr, self.c_eptr, self.nseg,
            f.ptr.data_ptr(), f.other.data_ptr(), f.perm.data_ptr(), f.w.data_ptr(),
            b.ptr.data_ptr(), b.other.data_ptr(), b.perm.data_ptr(), b.w.data_ptr(),
            self.images[0].data_ptr(), self.images[1].data_ptr(), self.status.data_ptr(), current_stream_ptr(self.ei.device))
        _lib.check(rc, "dc_graph_build_segmented_image")
        return self

    def chain(self, side, slab, f, k, rowmax, mode, image, src=0, direction=1):
        adj = self.sides[side]
        rc = _lib.lib().dc_hop_chain_image_f32(
            adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), self.sides[0].ptr.data_ptr(), adj.other.numel(),
            self.c_nptr, self.nseg, slab.data_ptr(), slab.stride(0), slab.size(0), f, k, src, direction,
            rowmax.data_ptr() if rowmax is not None else None, mode,
            self.images[side].data_ptr() if image else None, current_stream_ptr(slab.device))
        _lib.check(rc, "dc_hop_chain_image_f32")


_BUILT = {}


def built(sizes, seed=0):
    """One build per batch, shared by the tests (nothing below writes to it)."""
    if (sizes, seed) not in _BUILT:
        _BUILT[sizes, seed] = Built(*make_batch(sizes, seed)).build()
        torch.cuda.synchronize()
    return _BUILT[sizes, seed]


def tables_numpy(ptr, other, deg_ptr, nptr):
    """What k_hop_chain_gcn derives from the finished arrays: padded local ids, {first edge, degree}, dis."""
    n = len(ptr) - 1
    ids = np.full((n, 8), PAD, np.uint16)
    bounds = np.zeros((n, 2), np.int32)
    for g in range(len(nptr) - 1):
        for r in range(nptr[g], nptr[g + 1]):
            b, d = int(ptr[r]), int(ptr[r + 1] - ptr[r])
            bounds[r] = (b, d)
            m = min(d, 8)
            ids[r, :m] = other[b:b + m] - nptr[g]
    din = (deg_ptr[1:] - deg_ptr[:-1]).astype(np.float32)
    with np.errstate(divide="ignore"):
        dis = np.where(din > 0, np.float32(1.0) / np.sqrt(din), np.float32(0.0)).astype(np.float32)
    return ids, bounds, np.concatenate([dis, np.zeros(1, np.float32)])


def test_image_holds_the_tables_of_both_sides_and_nothing_around_it_is_written():
    bt = built(SIZES_8)
    n = bt.n
    assert int(bt.status.item()) == 0
    deg_ptr = bt.sides[0].ptr.cpu().numpy()
    for side in (0, 1):
        ptr, other = bt.sides[side].ptr.cpu().numpy(), bt.sides[side].other.cpu().numpy()
        deg = ptr[1:] - ptr[:-1]
        for want in (0, 8, 9, 17):                              # degree 0, a full id row, the tail path
            assert (deg == want).any(), f"the batch has no node of degree {want} on side {side}"
        raw = bt.raw[side].cpu().numpy()
        assert (raw[:4] == CANARY).all() and (raw[4 + bt.nbytes // 4:] == CANARY).all(), "a word around the image changed"
        img = raw[4:4 + bt.nbytes // 4].view(np.uint8)
        ids = img[:16 * n].view(np.uint16).reshape(n, 8)
        bounds = img[16 * n:24 * n].view(np.int32).reshape(n, 2)
        dis = img[24 * n:28 * n + 4].view(np.uint32)
        want_ids, want_bounds, want_dis = tables_numpy(ptr, other, deg_ptr, bt.nptr)
        assert np.array_equal(ids, want_ids)
        assert np.array_equal(bounds, want_bounds)
        assert np.array_equal(dis, want_dis.view(np.uint32)), "dis differs in bits"
        sizes = np.repeat(np.diff(bt.nptr), np.diff(bt.nptr))
        assert ((ids == PAD) | (ids < sizes[:, None])).all()     # every id is local to its graph


def reference_chain(adj, slab, f, k, rowmax, mode, src=0, direction=1):
    for j in range(k):
        a, b = src + j * direction, src + (j + 1) * direction
        ops.hop(adj, slab[:, a * f:(a + 1) * f], out=slab[:, b * f:(b + 1) * f], weighted=True, rowmax=rowmax,
                rowmax_mode=(mode if j == 0 else 2) if rowmax is not None else 0)


def check_chains(bt, f, k, mode, side, seed, check_single_hops=True, guard=0):
    """Chain with the image, chain without, K single hops: the same slab and row maxima, bit for bit.  ``guard`` rows of a
    canary value in front of and behind the slab must stay what they were."""
    torch.manual_seed(seed)
    n = bt.n
    big = ops._alloc_slab(n + 2 * guard, (k + 1) * f, DEV)
    big.normal_()
    big[:, :f] *= torch.logspace(-3, 3, n + 2 * guard, device=DEV)[:, None]
    if guard:
        big[:guard] = 7.25
        big[n + guard:] = 7.25
    rm0 = torch.rand(n, device=DEV) * (10.0 if mode & 2 else 0.0) if mode else None
    out = []
    for image in (True, False):
        full = big.clone()
        slab = full[guard:guard + n]
        rm = rm0.clone() if rm0 is not None else None
        bt.chain(side, slab, f, k, rm, mode, image)
        out.append((full, rm))
    if check_single_hops:
        full = big.clone()
        rm = rm0.clone() if rm0 is not None else None
        reference_chain(bt.sides[side], full[guard:guard + n], f, k, rm, mode)
        out.append((full, rm))
    torch.cuda.synchronize()
    for other, what in zip(out[1:], ("the chain without it", "K single hops")):
        assert torch.equal(out[0][0], other[0]), \
            f"chain with image vs {what}: {(out[0][0] != other[0]).sum().item()} slab elements differ"
        if mode:
            assert torch.equal(out[0][1], other[1]), f"chain with image vs {what}: row maxima differ"
    if guard:
        assert (out[0][0][:guard] == 7.25).all() and (out[0][0][n + guard:] == 7.25).all(), "a row outside the slab changed"


@pytest.mark.parametrize("sizes", [SIZES_8, SIZES_2, SIZES_7], ids=["steps8", "steps2", "steps7"])
def test_chain_with_image_equals_chain_without_and_single_hops(sizes):
    bt = built(sizes)
    seed = 0
    for k in (1, 2, 3):
        for f in (32, 64):
            for mode in (0, 1, 2, 3):
                for side in (0, 1):
                    seed += 1
                    check_chains(bt, f, k, mode, side, seed)


def test_flagged_edge_image_and_in_kernel_tables_agree_and_stay_inside_the_graph():
    ei, nptr, eptr = make_batch((130, 257, 40), seed=3)
    e = eptr[1] + 5                                              # an edge of graph 1 ...
    ei[0, e] = 3                                                 # ... whose source is a node of graph 0
    bt = Built(ei, nptr, eptr).build()
    assert int(bt.status.item()) & 1, "the build did not flag the edge that leaves its graph"
    for side in (0, 1):
        raw = bt.raw[side].cpu().numpy()
        assert (raw[:4] == CANARY).all() and (raw[4 + bt.nbytes // 4:] == CANARY).all()
        ids = raw[4:4 + bt.nbytes // 4].view(np.uint8)[:16 * bt.n].view(np.uint16).reshape(bt.n, 8)
        want = tables_numpy(bt.sides[side].ptr.cpu().numpy(), bt.sides[side].other.cpu().numpy(),
                            bt.sides[0].ptr.cpu().numpy(), nptr)[0]
        assert np.array_equal(ids, want)                         # (the flagged edge sits on node 0 of its graph)
        for k, mode in ((3, 1), (2, 3), (1, 0)):
            check_chains(bt, 64, k, mode, side, seed=10 * side + k, guard=8)


def test_build_and_both_chains_replayed_from_a_hipgraph_on_new_batches():
    sizes, f, k = (130, 257, 0, 1024, 7), 64, 3
    batches = [make_batch(sizes, seed) for seed in (11, 12)]
    assert batches[0][1:] == batches[1][1:] and not np.array_equal(batches[0][0], batches[1][0])
    n = batches[0][1][-1]
    torch.manual_seed(4)
    x = [torch.randn(n, f, device=DEV) for _ in batches]
    # eager results, each on buffers of its own
    eager = []
    for (ei, nptr, eptr), x0 in zip(batches, x):
        bt = Built(ei, nptr, eptr).build()
        res = []
        for side in (0, 1):
            slab = ops._alloc_slab(n, (k + 1) * f, DEV).zero_()
            slab[:, :f] = x0
            rm = torch.zeros(n, device=DEV)
            bt.chain(side, slab, f, k, rm, 1, True)
            res += [slab, rm]
        eager.append(res)
    # one captured graph: build with image, forward chain, transposed chain
    edges = torch.from_numpy(batches[0][0]).to(DEV)
    bt = Built(*batches[0], edge_buffer=edges)
    slabs = [ops._alloc_slab(n, (k + 1) * f, DEV).zero_() for _ in range(2)]
    rms = [torch.zeros(n, device=DEV) for _ in range(2)]
    for s in slabs:
        s[:, :f] = x[0]
    bt.build()                                                   # (warm-up outside the capture)
    for side in (0, 1):
        bt.chain(side, slabs[side], f, k, rms[side], 1, True)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        bt.build()
        for side in (0, 1):
            bt.chain(side, slabs[side], f, k, rms[side], 1, True)
    for i in (1, 0, 1):
        edges.copy_(torch.from_numpy(batches[i][0]))
        for s in slabs:
            s.zero_()
            s[:, :f] = x[i]
        for img in bt.raw:
            img.fill_(CANARY)                                    # nothing of the last replay's image may be needed
        gr.replay()
        torch.cuda.synchronize()
        for side in (0, 1):
            assert torch.equal(slabs[side], eager[i][2 * side]), f"replay on batch {i}, side {side}: blocks differ"
            assert torch.equal(rms[side], eager[i][2 * side + 1]), f"replay on batch {i}, side {side}: row maxima differ"
        assert int(bt.status.item()) == 0
