"""``fps`` (``deformcontact_amd.pointops``, csrc/dc_pointops.hip): farthest point sampling.

CPU: the count rule, argument errors of the Python function and of the C entry, the exported names.
GPU: bit for bit against a numpy restatement of the rules: fp32 arrays, so every operation
rounds as the kernel's does; ``np.argmax`` takes the first maximum - the lowest index among equally far points."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import deformcontact_amd as dc
from deformcontact_amd import _lib, neighbors, pointops

DEV = torch.device("cuda:0")
EINVAL = -1
R = pointops.FPS_RESIDENT_POINTS


# ---------------------------------------------------------------------------------------------------------------- #
# CPU
# ---------------------------------------------------------------------------------------------------------------- #
def test_count_rule_on_the_host():
    for n, ratio, want in ((10, .3, 3), (7, .25, 2), (65, .1, 7), (3, .01, 1), (1000, .7, 700)):
        assert pointops.fps_count(n, ratio) == want, (n, ratio)
    for n in (1, 2, 63, 1025, 100000, (1 << 24) + 3):                # (2^24 + 3 rounds UP in fp32: never more than n)
        assert pointops.fps_count(n, 1.0) == n
    got = pointops.fps_count(np.array([1, 5, 64, 130, 0, 7]), 0.5)
    assert got.dtype == np.int64 and got.tolist() == [1, 3, 32, 65, 0, 4]


def test_argument_errors(monkeypatch):
    pos = torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        dc.nn.fps(pos)
    for bad in (0, 0.0, 1.5, -0.25, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            dc.nn.fps(pos, ratio=bad)
    with pytest.raises(TypeError, match="ratio"):
        dc.nn.fps(pos, ratio=torch.tensor(0.5))
    with pytest.raises(ValueError, match="not both"):
        dc.nn.fps(pos, torch.zeros(6, dtype=torch.int64), ptr=torch.tensor([0, 6]))
    # the checks below come after the device check: stub it out
    monkeypatch.setattr(neighbors, "_require_cuda", lambda t, what: None)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        dc.nn.fps(torch.zeros(6, 2))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        dc.nn.fps(torch.zeros(6, 4))
    with pytest.raises(TypeError, match="float32"):
        dc.nn.fps(torch.zeros(6, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="inner stride"):
        dc.nn.fps(torch.zeros(3, 6).t())


def test_entry_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.dc_fps_resident_points() == R
    assert L.dc_fps_workspace_bytes(-1, 0) < 0 and L.dc_fps_workspace_bytes(10, 11) < 0
    assert L.dc_fps_workspace_bytes(10, -1) < 0
    assert L.dc_fps_workspace_bytes(R, R) == 0 and L.dc_fps_workspace_bytes(R + 1, R + 1) == 16 * (R + 1)
    assert L.dc_fps_workspace_bytes(3 * R, R) == 0
    fake = ctypes.c_void_p(64)                      # never dereferenced: every call below fails its checks first

    def call(x=fake, ldx=3, n=10, ptr=None, optr=None, b=1, max_n=None, start=None, out=fake, m=5, ws=None, nbytes=0):
        return L.dc_fps(x, ldx, n, ptr, optr, b, n if max_n is None else max_n, start, out, m, ws, nbytes, None)
    for kw, msg in ((dict(n=-1), b"bad sizes"), (dict(m=-1), b"bad sizes"), (dict(m=11), b"bad sizes"),
                    (dict(b=-1), b"bad sizes"), (dict(max_n=-1), b"bad sizes"), (dict(max_n=11), b"bad sizes"),
                    (dict(n=1 << 31, m=1), b"bad sizes"), (dict(ldx=2), b"leading"),
                    (dict(ptr=fake), b"ptr and optr"), (dict(optr=fake), b"ptr and optr"), (dict(b=2), b"need ptr"),
                    (dict(x=None), b"null"), (dict(out=None), b"null"),
                    (dict(n=R + 1, m=4), b"null"),                                  # a big graph: the workspace
                    (dict(n=R + 1, m=4, ws=fake, nbytes=16 * R), b"workspace too small"),
                    (dict(n=R + 1, m=4, ws=ctypes.c_void_p(72), nbytes=1 << 30), b"aligned")):
        assert call(**kw) == EINVAL, kw
        assert msg in L.dc_last_error() and b"dc_fps" in L.dc_last_error(), (kw, L.dc_last_error())
    for kw in (dict(n=0, m=0, x=None, out=None), dict(m=0, x=None, out=None), dict(b=0, x=None, out=None),
               dict(max_n=0, x=None, out=None)):
        assert call(**kw) == 0, kw                  # nothing to do: nothing is read, written or launched
    assert call(n=0, m=0, ldx=2, x=None) == EINVAL  # ... but the arguments are still checked


def test_exports_alias_and_position_in_all():
    assert dc.nn.fps is pointops.fps and dc.nn.knn_interpolate is pointops.knn_interpolate
    names = dc.nn.__all__
    at = names.index("EdgeConv")
    assert names[at:at + 4] == ["EdgeConv", "fps", "knn_interpolate", "SplineConv"]
    assert sorted(n for n in _lib.exported_names() if n.startswith("dc_fps")) == \
        ["dc_fps", "dc_fps_resident_points", "dc_fps_workspace_bytes"]
    dc.install_as_torch_geometric()
    try:
        from torch_geometric.nn import fps
        assert fps is pointops.fps
    finally:
        for k in ("torch_geometric", "torch_geometric.nn", "torch_geometric.data"):
            sys.modules.pop(k, None)


# ---------------------------------------------------------------------------------------------------------------- #
# the reference: the rules restated in numpy
# ---------------------------------------------------------------------------------------------------------------- #
def _d2(p, c):
    d = p - c                                                        # float32
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _count(n, ratio):
    return min(int(np.ceil(np.float32(n) * np.float32(ratio))), n)


def ref_graph(p, m, s=0):
    """the m picks (local indices) of one graph with the fp32 points p, started at s"""
    assert p.dtype == np.float32
    out = [s]
    dist = _d2(p, p[s])
    for _ in range(1, m):
        j = int(np.argmax(dist))                                     # the first maximum: the lowest index
        out.append(j)
        dist = np.minimum(dist, _d2(p, p[j]))
    return np.asarray(out[:m], np.int64)


def ref_batch(p, sizes, ratio, starts=None):
    out, a = [], 0
    for g, n in enumerate(sizes):
        if n:
            s = 0 if starts is None else int(starts[g]) - a
            out.append(a + ref_graph(p[a:a + n], _count(n, ratio), s))
        a += n
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def _cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def _check(got, want):
    assert got.dtype == torch.int64 and got.dim() == 1 and got.is_contiguous() and got.device.type == "cuda"
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (got.cpu()[:16], want[:16])


# ---------------------------------------------------------------------------------------------------------------- #
# GPU
# ---------------------------------------------------------------------------------------------------------------- #
# 1 .. 65: one wave and its edges; 300 / 1000 / 1025: 2, 4 and 8 points per thread (1025: one past 1024 threads x 1);
# R: the last resident size (1024 threads x 8 points); R + 1: the workspace kernel
SIZES = [1, 2, 63, 64, 65, 300, 1000, 1025, R, R + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_single_cloud_matches_the_restatement(n):
    p = _cloud(n, 100 + n)
    x = torch.from_numpy(p).to(DEV)
    big = n >= R                                                     # a small ratio there: at most 64 picks
    for ratio in ((63.0 / n, 17.0 / n, 1.0 / n) if big else (1.0, 0.5, 1.0 / n)):
        m = _count(n, ratio)
        assert 1 <= m <= (64 if big else n)
        got = dc.nn.fps(x, ratio=ratio, random_start=False)
        print(f"  fps N={n} ratio={ratio:.5f}: {m} picks")
        _check(got, ref_graph(p, m))
    assert dc.nn.fps(x[:0], ratio=0.5).shape == (0,)


@pytest.mark.gpu
def test_workspace_kernel_equals_the_resident_kernel_on_a_batch():
    """A batch whose largest graph is one past the resident limit runs every graph on the workspace kernel; its small
    graphs must come out as they do alone (on the resident kernel)."""
    sizes = [70, R + 1, 0, 200]
    p = _cloud(sum(sizes), 5)
    ptr = np.r_[0, np.cumsum(sizes)]
    x = torch.from_numpy(p).to(DEV)
    ratio = 0.02                                                     # 2, 164 and 4 picks
    got = dc.nn.fps(x, ptr=torch.from_numpy(ptr).to(DEV), ratio=ratio, random_start=False)
    _check(got, ref_batch(p, sizes, ratio))
    alone = [a + dc.nn.fps(x[a:b], ratio=ratio, random_start=False) for a, b in zip(ptr[:-1], ptr[1:]) if b > a]
    assert torch.equal(got, torch.cat(alone))


@pytest.mark.gpu
def test_batch_and_ptr_give_the_same_picks():
    sizes = [1, 5, 64, 130, 0, 7]                                    # id 4 owns no node
    p = _cloud(sum(sizes), 7)
    x = torch.from_numpy(p).to(DEV)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    ptr = torch.from_numpy(np.r_[0, np.cumsum(sizes)]).to(DEV)
    for ratio in (0.5, 1.0, 0.01):
        want = ref_batch(p, sizes, ratio)
        a = dc.nn.fps(x, batch, ratio, random_start=False)
        b = dc.nn.fps(x, ptr=ptr, ratio=ratio, random_start=False)
        c = dc.nn.fps(x, batch, ratio, random_start=False, batch_size=len(sizes))
        _check(a, want), _check(b, want), _check(c, want)
    with pytest.raises(ValueError, match="node offsets"):
        dc.nn.fps(x, batch, 0.5, batch_size=3)                       # ids beyond batch_size
    with pytest.raises(ValueError, match="node offsets"):
        dc.nn.fps(x, ptr=ptr[:-1], ratio=0.5)


@pytest.mark.gpu
def test_ties_take_the_lowest_index_and_the_tail_is_the_first_node():
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    lattice = g[rng.permutation(len(g))]                             # integer coordinates: many exact ties
    got = dc.nn.fps(torch.from_numpy(lattice).to(DEV), ratio=1.0, random_start=False)
    _check(got, ref_graph(lattice, len(lattice)))
    assert sorted(got.tolist()) == list(range(len(lattice)))         # all distinct: every point once
    half = _cloud(40, 12)
    twice = np.concatenate([half, half])                             # every point duplicated
    got = dc.nn.fps(torch.from_numpy(twice).to(DEV), ratio=1.0, random_start=False)
    _check(got, ref_graph(twice, 80))
    assert sorted(got[:40].tolist()) == list(range(40))              # the lower copy of every point ...
    assert got[40:].tolist() == [0] * 40                             # ... then all distances are 0: the first node


@pytest.mark.gpu
def test_strided_positions():
    wide = torch.from_numpy(np.random.default_rng(3).random((333, 4), dtype=np.float32)).to(DEV)
    x = wide[:, :3]
    assert x.stride() == (4, 1)
    got = dc.nn.fps(x, ratio=0.25, random_start=False)
    _check(got, ref_graph(np.ascontiguousarray(wide.cpu().numpy()[:, :3]), _count(333, 0.25)))
    assert torch.equal(got, dc.nn.fps(x.contiguous(), ratio=0.25, random_start=False))


@pytest.mark.gpu
def test_random_start_lies_in_the_graph_and_the_rest_follows_from_it():
    sizes = [1, 5, 64, 130, 0, 7]
    p = _cloud(sum(sizes), 21)
    x = torch.from_numpy(p).to(DEV)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    ptr = np.r_[0, np.cumsum(sizes)]
    optr = np.r_[0, np.cumsum([_count(n, 0.5) for n in sizes])]
    torch.manual_seed(1234)
    firsts = set()
    for _ in range(3):
        got = dc.nn.fps(x, batch, 0.5, random_start=True)
        starts = [int(got[optr[g]]) if sizes[g] else -1 for g in range(len(sizes))]
        for g, n in enumerate(sizes):
            assert n == 0 or ptr[g] <= starts[g] < ptr[g + 1], (g, starts[g])
        _check(got, ref_batch(p, sizes, 0.5, starts))
        firsts.add(starts[3])
    assert len(firsts) > 1                                           # 130 nodes, three draws: the start does move
    one = dc.nn.fps(x[6:70], ratio=0.5)                              # a single cloud, random_start by default
    assert 0 <= int(one[0]) < 64
    _check(one, ref_graph(p[6:70], 32, int(one[0])))


@pytest.mark.gpu
def test_capture_and_replay_on_new_positions():
    """The single-cloud call reads nothing on the host: recorded in torch.cuda.graph and replayed on positions written
    into the static input, it equals the eager call."""
    static = torch.from_numpy(_cloud(1000, 31)).to(DEV)
    run = lambda p: dc.nn.fps(p, ratio=0.25, random_start=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static)                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(static)
    for seed in (32, 33):
        new = _cloud(1000, seed)
        static.copy_(torch.from_numpy(new).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, run(torch.from_numpy(new).to(DEV)))
        _check(out, ref_graph(new, 250))


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    sizes = [257, 1024, 3]
    x = torch.from_numpy(_cloud(sum(sizes), 41)).to(DEV)
    ptr = torch.from_numpy(np.r_[0, np.cumsum(sizes)]).to(DEV)
    assert torch.equal(dc.nn.fps(x, ptr=ptr, ratio=0.25, random_start=False),
                       dc.nn.fps(x, ptr=ptr, ratio=0.25, random_start=False))
    big = torch.from_numpy(_cloud(R + 100, 42)).to(DEV)
    assert torch.equal(dc.nn.fps(big, ratio=0.004, random_start=False), dc.nn.fps(big, ratio=0.004, random_start=False))
