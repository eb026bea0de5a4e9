"""``TAGConv`` / ``GCNConv`` / ``GATConv`` / ``GATv2Conv`` / ``TransformerConv`` / ``SAGEConv`` / ``GINConv`` / ``GINEConv`` /
``EdgeConv`` / ``ChebConv`` / ``GMMConv`` / ``SplineConv`` on the HIP hop kernels.

Drop-in for the PyG classes the reference instantiates at
``/root/reference/models/model.py:39-50`` and calls at ``:71,77``.  Parameter
names, shapes and default initialisers follow PyG 2.5.2 so reference
checkpoints (``eval.py:36,89``: ``load_state_dict(torch.load(...))``) load
unchanged:

* ``TAGConv``: ``lins.{0..K}.weight [out,in]`` (no per-lin bias), ``bias [out]``;
* ``GCNConv``: ``lin.weight [out,in]`` (glorot), ``bias [out]``;
* ``GATConv``: ``lin.weight [H*out,in]`` (glorot), ``att_src/att_dst [1,H,out]``,
  ``bias [H*out]`` (``concat=False``: ``[out]``); with ``edge_dim=D`` also
  ``lin_edge.weight [H*out,D]`` (glorot) and ``att_edge [1,H,out]``;
* ``GATv2Conv``: ``lin_l.weight`` / ``lin_r.weight [H*out,in]`` (glorot) with ``lin_l.bias`` / ``lin_r.bias [H*out]``,
  ``att [1,H,out]``, ``bias [H*out]`` (``concat=False``: ``[out]``); ``share_weights=True``: ``lin_r is lin_l``;
* ``TransformerConv``: ``lin_key`` / ``lin_query`` / ``lin_value`` ``.weight [H*out,in]`` and ``.bias [H*out]``,
  ``lin_skip.weight [W,in]`` (``W = H*out``, ``concat=False``: ``out``) with ``lin_skip.bias [W]`` when ``bias``, and
  ``lin_beta.weight [1,3W]`` when ``beta`` - all ``U(+-1/sqrt(fan_in))``; no ``bias`` of the layer itself;
* ``SAGEConv``: ``lin_l.weight [out,in]`` with ``lin_l.bias [out]`` when ``bias``, ``lin_r.weight [out,in]`` when
  ``root_weight``, ``lin.weight [in,in]`` and ``lin.bias [in]`` when ``project`` - all ``U(+-1/sqrt(fan_in))``;
* ``GINConv`` / ``GINEConv``: ``eps [1]`` (a parameter with ``train_eps``, else a buffer), the keys of the user's module
  under ``nn.``, and for ``GINEConv(edge_dim=D)`` ``lin.weight [in,D]`` and ``lin.bias [in]`` (``U(+-1/sqrt(D))``);
* ``EdgeConv``: the keys of the user's module under ``nn.`` and nothing else;
* ``ChebConv``: ``lins.{0..K-1}.weight [out,in]`` (glorot, no per-lin bias), ``bias [out]`` (zeros);
* ``GMMConv``: ``g [in,K*out]``, ``mu`` / ``sigma [K,dim]``, ``root.weight [out,in]`` when ``root_weight`` (all glorot),
  ``bias [out]`` (zeros);
* ``SplineConv``: ``weight [K,in,out]`` (``U(+-1/sqrt(K*in))``, ``K`` the product of ``kernel_size``), ``lin.weight
  [out,in]`` when ``root_weight`` (``U(+-1/sqrt(in))``), ``bias [out]`` (zeros), the buffers ``kernel_size [dim]`` int64
  and ``is_open_spline [dim]`` uint8.

No CPU path: calling a conv with CPU tensors raises.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops
from ..graph import GraphIndex, _require_cuda, graph_index
from ..deferred import deferred, resolve
from ..neighbors import MAX_CAP, knn_graph

#: a plain ``conv(x, edge_index)`` call returns a ``deferred.DeferredActivation``: the ``F.relu`` the reference applies
#: right behind it (``models/model.py:71,77``) then runs fused in the layer's epilogue, and the output lands in the hop
#: slab of the TAGConv layer that consumed it last time (``TAGConv._consumer_geom``) - the unchanged reference wiring on
#: the same launches as ``graphnet.ContactEncoder``.  False / ``DC_DEFER_ACT=0``: the conv returns its output directly.
DEFER_ACTIVATION = os.environ.get("DC_DEFER_ACT", "1") != "0"


#: OPT-IN (``DC_BRANCH_STREAMS=1`` or ``nn.conv.BRANCH_STREAMS = True``; default off): run the independent branches of a
#: forward pass written with plain conv calls - the resting loop and the rigid loop of ``models/model.py:69-78`` - on two HIP
#: streams, as ``graphnet.ContactEncoder`` does.  A conv whose input carries no producer tag starts a branch: the first
#: branch of a pass stays on the caller's stream, every further one runs on a side stream that waits only for the point at
#: which the pass began (an event recorded at the pass's first conv call), and the caller's stream waits for the side stream
#: behind every layer launched there, so whatever the caller enqueues later (the cross-attention) sees the results; autograd
#: replays the structure in backward.  CONTRACT, which is why this is opt-in: the inputs of EVERY branch (features and
#: ``edge_index`` of both graphs) must be complete on the caller's stream when the first conv of the pass is called - true of
#: a model whose ``forward`` receives its graphs as arguments, as the reference's does.  A pass ends when a branch's first
#: layer is called again.
BRANCH_STREAMS = os.environ.get("DC_BRANCH_STREAMS", "0") == "1"
_PASS = {}            # device index -> {"roots": set of module ids, "event", "main": stream handle, "count"}


def _branch_stream(module: nn.Module, x: Tensor):
    """The side stream this plain conv call's layer runs on, or None (the caller's stream).  See ``BRANCH_STREAMS``."""
    if not BRANCH_STREAMS:
        return None
    side = getattr(x, "_dc_branch", None)
    if side is not None:
        return side                                            # a later layer of a side branch follows its input
    if getattr(x, "_dc_producer", None) is not None or x.grad_fn is not None:
        return None                                            # not a graph input: ordinary stream semantics
    from ..graphnet import ContactEncoder
    dev = x.device
    main = torch.cuda.current_stream(dev)
    st = _PASS.get(dev.index)
    if st is None or id(module) in st["roots"] or st["main"] != main.cuda_stream:
        st = _PASS[dev.index] = {"roots": set(), "event": torch.cuda.Event(), "main": main.cuda_stream, "count": 0}
        st["event"].record(main)                               # the pass begins: every branch's inputs exist (contract)
    st["roots"].add(id(module))
    st["count"] += 1
    if st["count"] == 1:
        return None
    side = ContactEncoder._side_stream(dev)
    side.wait_event(st["event"])
    return side


def _on_branch(side, fn):
    """``fn()`` on ``side`` (None: here); the caller's stream then waits for it and the result remembers its stream."""
    if side is None:
        return fn()
    main = torch.cuda.current_stream(side.device)
    with torch.cuda.stream(side):
        out = fn()
    main.wait_stream(side)
    out.record_stream(main)
    out._dc_branch = side
    return out


def _grad_wanted(x: Tensor, module: nn.Module) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


class _Lin(nn.Module):
    """Parameter holder mirroring ``torch_geometric.nn.dense.Linear(bias=False)``; ``bias=True`` (GATv2Conv's linears):
    with a bias ``[out]``, PyG's default ``U(+-1/sqrt(in))``."""

    #: set by GATConv on its ``lin``: keep the six-product dense kernels (``ops.dense_linear(six_products=True)``)
    six_products = False

    def __init__(self, in_channels: int, out_channels: int, initializer: Optional[str] = None, bias: bool = False):
        super().__init__()
        self.in_channels, self.out_channels, self.initializer = in_channels, out_channels, initializer
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.initializer == "glorot":
            a = math.sqrt(6.0 / (self.in_channels + self.out_channels))
        else:  # kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in))
            a = 1.0 / math.sqrt(self.in_channels)
        with torch.no_grad():
            self.weight.uniform_(-a, a)
            if self.bias is not None:
                b = 1.0 / math.sqrt(self.in_channels)
                self.bias.uniform_(-b, b)

    def forward(self, x: Tensor) -> Tensor:
        x = resolve(x)
        if x.is_cuda and x.dim() == 2 and x.dtype == torch.float32:
            # the library's MFMA dense block
            return ops.dense_linear(x, self.weight, self.bias, six_products=self.six_products)
        return torch.nn.functional.linear(x, self.weight, self.bias)


def _check_inputs(x: Tensor, edge_index: Tensor, in_channels: int):
    _require_cuda(x, "x")
    _require_cuda(edge_index, "edge_index")
    if x.dim() != 2 or x.size(1) != in_channels:
        raise ValueError(f"x must be [N, {in_channels}], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"x must be float32, got {x.dtype}")
    if x.device != edge_index.device:
        raise RuntimeError(f"x is on {x.device} but edge_index is on {edge_index.device}")


def _check_edge_attr(edge_attr, edge_index, width: int, hint: str = "", width_note: str = "", mismatch=None) -> Tensor:
    """The third positional argument as PyG's ``edge_attr``, checked on the host for ``GATConv`` and ``GINEConv``: a
    tensor, resolved, float32, ``[E]`` -> ``[E, 1]`` where ``width`` is 1, 2-D of that width, one row per edge of
    ``edge_index``.  The layers' wordings differ and are kept: ``hint`` ends the type error, ``width_note`` follows the
    expected shape of a tensor that is not 2-D, ``mismatch(edge_attr)`` is the layer's own text for a wrong width."""
    if not isinstance(edge_attr, Tensor):
        raise TypeError(f"edge_attr (the third positional argument, as in PyG) must be a tensor, got "
                        f"{type(edge_attr).__name__}{hint}")
    edge_attr = resolve(edge_attr)
    if edge_attr.dtype != torch.float32:
        raise ValueError(f"edge_attr must be float32, got {edge_attr.dtype}")
    if edge_attr.dim() == 1 and width == 1:
        edge_attr = edge_attr.unsqueeze(-1)
    if edge_attr.dim() != 2:
        raise ValueError(f"edge_attr must be [E, {width}]{width_note}, got {tuple(edge_attr.shape)}")
    if edge_attr.size(1) != width:
        raise ValueError(mismatch(edge_attr) if mismatch is not None else
                         f"edge_attr must be [E, {width}] (edge_dim = {width}), got {tuple(edge_attr.shape)}")
    if isinstance(edge_index, Tensor) and edge_index.dim() == 2 and edge_attr.size(0) != edge_index.size(1):
        raise ValueError(f"edge_attr has {edge_attr.size(0)} rows but edge_index has {edge_index.size(1)} edges")
    return edge_attr


class _ConvBase(nn.Module):
    """What every conv layer shares: the adjacency it runs on.  A class states how its edge set is prepared as data
    (``_self_loops``, ``_gcn_norm``); ``graph_flags()`` / ``graph()`` are what the loaders and the encoder call."""

    _self_loops = False       # remove, then add, one self loop per node
    _gcn_norm = False         # weights deg^-1/2 [source] deg^-1/2 [destination]

    def graph_flags(self) -> dict:
        return dict(self_loops=self._self_loops, normalize=self._gcn_norm)

    def graph(self, edge_index: Tensor, num_nodes: int, segments=None) -> GraphIndex:
        return graph_index(edge_index, num_nodes, segments=segments, **self.graph_flags())

    def _init_bias(self, width: int, bias: bool) -> None:
        """``self.bias``: a zero Parameter ``[width]``, or None."""
        if bias:
            self.bias = nn.Parameter(torch.zeros(width))
        else:
            self.register_parameter("bias", None)


class _ReluConv(_ConvBase):
    """The layers that can run the ReLU behind them in their own epilogue (``relu=True``), and whose plain call returns
    a deferred result that lets what follows decide (``DEFER_ACTIVATION``)."""

    supports_fused_relu = True

    @property
    def out_width(self) -> int:
        """Width of the output of a layer with ``heads``: side by side (``concat``) or their mean."""
        return self.heads * self.out_channels if self.concat else self.out_channels

    def _dispatch(self, x: Tensor, edge_index: Tensor, relu: bool, next_conv, width: int, empty_none: bool = False,
                  layer=None, **extra: Optional[Tensor]) -> Tensor:
        """``self._layer(g, x, relu, *extra)`` now - or, for the plain PyG call, as a deferred result of ``width``
        columns on the branch's stream.  ``extra``: further tensors of the call (``edge_attr=...`` or None), which must
        be on ``x``'s device, are guarded with ``x`` and make the result want a gradient when they do.  ``empty_none``:
        no node -> no adjacency is built and ``g`` is None.  ``layer``: what runs in place of ``self._layer`` (same
        arguments) - a call that carries arguments which are no tensors binds them into it."""
        layer = layer if layer is not None else self._layer
        x = resolve(x)
        _check_inputs(x, edge_index, self.in_channels)
        for name, t in extra.items():
            if t is not None:
                _require_cuda(t, name)
                if t.device != x.device:
                    raise RuntimeError(f"x is on {x.device} but {name} is on {t.device}")
        extra = tuple(extra.values())

        def graph() -> Optional[GraphIndex]:
            return self.graph(edge_index, x.size(0)) if x.size(0) or not empty_none else None
        if DEFER_ACTIVATION and not relu and next_conv is None:
            side = _branch_stream(self, x)
            wanted = _grad_wanted(x, self) or (torch.is_grad_enabled()
                                               and any(t is not None and t.requires_grad for t in extra))
            return deferred(lambda act: _on_branch(side, lambda: layer(graph(), x, act, *extra)),
                            x.size(0), width, x, wanted).guard(x, edge_index, *extra, *self.parameters())
        return layer(graph(), x, relu, *extra)


class TAGConv(_ReluConv):
    def __init__(self, in_channels: int, out_channels: int, K: int = 3, bias: bool = True,
                 normalize: bool = True):
        super().__init__()
        self.in_channels, self.out_channels, self.K, self.normalize = \
            in_channels, out_channels, K, normalize
        self.lins = nn.ModuleList([_Lin(in_channels, out_channels) for _ in range(K + 1)])
        self._init_bias(out_channels, bias)
        #: {activation fused?: (width, padded width) of the hop slab of the layer that consumed the last output}
        self._consumer_geom = {}

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    _gcn_norm = property(lambda self: self.normalize)
    #: dtype of the output when the input is bfloat16 (the bf16-storage forward path)
    bf16_out = torch.bfloat16

    def slab_width(self) -> int:
        return ops.tag_slab_geometry(self.in_channels, self.K)[2]

    def forward(self, x: Tensor, edge_index: Tensor, relu: bool = False,
                next_conv: "Optional[TAGConv]" = None, out_into: Optional[Tensor] = None) -> Tensor:
        """``conv(x, edge_index)`` as PyG.  Extensions: ``relu=True`` fuses the ReLU the reference
        applies right after (``models/model.py:71,77``) into the MFMA epilogue; ``next_conv`` (the
        TAGConv that consumes this output) lets the output be written straight into that
        layer's hop slab; ``out_into`` (a ``[N, out]`` row-major view the caller owns, e.g. this
        branch's rows of a merged slab - ``ops.merged_slab_part``) receives the output instead."""
        if self.K + 1 > ops.MAX_SEG:   # (here, not in the dense block: before the adjacency build and a deferred first use)
            raise NotImplementedError(f"TAGConv K={self.K} > {ops.MAX_SEG - 1} is not supported by the fused dense block")
        x = resolve(x)                # (the deferred result of another plain conv call: its value, see deferred.py)
        if x.dtype == torch.bfloat16:
            # bf16-STORED features (BASELINE.json configs[4]): bf16 hops with fp32 accumulation + the
            # bf16 MFMA dense block; forward only.  ``out_dtype`` of the last layer: self.bf16_out
            _require_cuda(x, "x")
            _require_cuda(edge_index, "edge_index")
            if x.dim() != 2 or x.size(1) != self.in_channels:
                raise ValueError(f"x must be [N, {self.in_channels}], got {tuple(x.shape)}")
            g = self.graph(edge_index, x.size(0))
            nk = next_conv.K if (isinstance(next_conv, TAGConv)
                                 and next_conv.in_channels == self.out_channels) else None
            return ops.tag_conv_bf16(g, x, [lin.weight for lin in self.lins], self.bias, relu=relu,
                                     out_dtype=self.bf16_out, next_k=nk)
        _check_inputs(x, edge_index, self.in_channels)
        self._note_consumer(x)
        if DEFER_ACTIVATION and not relu and next_conv is None and out_into is None:
            # the PyG call as the reference makes it: what follows decides (deferred.py) - F.relu runs fused
            side = _branch_stream(self, x)

            def run(act: bool) -> Tensor:
                def layer():
                    g = self.graph(edge_index, x.size(0))
                    return self._mark(ops.tag_conv(g, x, [lin.weight for lin in self.lins], self.bias, relu=act,
                                                   next_geom=self._consumer_geom.get(act)), act)
                return _on_branch(side, layer)
            if side is None:
                self.graph(edge_index, x.size(0))        # the adjacency build starts at the call, as without deferral
            return deferred(run, x.size(0), self.out_channels, x, _grad_wanted(x, self)).guard(
                x, edge_index, *self.parameters())
        g = self.graph(edge_index, x.size(0))
        nxt = None
        if out_into is not None:
            nxt = ops.OutInto(out_into)
        elif isinstance(next_conv, TAGConv) and next_conv.in_channels == self.out_channels:
            nxt = ops.tag_slab_geometry(next_conv.in_channels, next_conv.K)[1:]
        return self._mark(ops.tag_conv(g, x, [lin.weight for lin in self.lins], self.bias, relu=relu,
                                       next_geom=nxt), relu)

    # ---- the consumer of a layer's output, discovered at call time ------------------------------------------------
    # ``models/model.py:69-78`` calls the layers one by one; nothing tells a conv who reads its output.  Every output
    # carries a weak reference to the layer that produced it; a TAGConv that is handed such a tensor and does NOT find
    # it sitting in block 0 of a hop slab of its own geometry tells the producer, which from its next call on
    # allocates its output as block 0 of that slab (one step of a training loop runs with the packing copy, every later
    # one without).  A wrong guess costs memory, never correctness: the output is a view either way.
    def _mark(self, out: Tensor, act: bool) -> Tensor:
        out._dc_producer = (weakref.ref(self), bool(act))
        return out

    def _note_consumer(self, x: Tensor) -> None:
        tag = getattr(x, "_dc_producer", None)
        if tag is None:
            return
        prod, act = tag[0](), tag[1]
        if isinstance(prod, TAGConv) and prod is not self and prod.out_channels == self.in_channels:
            geom = ops.tag_slab_geometry(self.in_channels, self.K)[1:]
            if prod._consumer_geom.get(act) != geom:
                prod._consumer_geom[act] = geom

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, K={self.K}"


class GCNConv(_ReluConv):
    _self_loops, _gcn_norm = True, True

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = _Lin(in_channels, out_channels, initializer="glorot")
        self._init_bias(out_channels, bias)

    def reset_parameters(self):
        self.lin.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, edge_index: Tensor, relu: bool = False, next_conv=None) -> Tensor:
        """``conv(x, edge_index)`` as PyG; ``relu=True`` fuses the ReLU the reference applies right after
        (``models/model.py:71,77``) - with the bias - into the aggregation launch (``ops.gcn_aggregate``)."""
        return self._dispatch(x, edge_index, relu, next_conv, self.out_channels)

    def _layer(self, g: GraphIndex, x: Tensor, relu: bool) -> Tensor:
        h = self.lin(x)
        if ops.fused_gnn_ok(h):
            return ops.gcn_aggregate(g, h, self.bias, relu)
        out = ops.propagate(g, h, weighted=True)
        if self.bias is not None:
            out = out + self.bias
        return torch.relu(out) if relu else out


class GATConv(_ReluConv):
    _self_loops = True

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, edge_dim: Optional[int] = None, fill_value="mean", bias: bool = True):
        super().__init__()
        if heads < 1:
            raise ValueError(f"heads must be >= 1, got {heads}")
        if edge_dim is not None and not 1 <= edge_dim <= ops.GAT_EDGE_MAX_DIM:
            raise ValueError(f"edge_dim must be within 1..{ops.GAT_EDGE_MAX_DIM} (the cap of the edge-feature kernels), "
                             f"got {edge_dim}")
        ops.gat_edge_fill(fill_value)                             # ("mean" or a Python float, else ValueError)
        self.edge_dim, self.fill_value = edge_dim, fill_value
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, bool(concat)
        self.negative_slope = negative_slope
        self.lin = _Lin(in_channels, heads * out_channels, initializer="glorot")
        self.lin.six_products = True             # the attention vectors' gradient cancels to 1 % of its terms: 24-bit products
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        if edge_dim is not None:
            self.lin_edge = _Lin(edge_dim, heads * out_channels, initializer="glorot")
            self.att_edge = nn.Parameter(torch.empty(1, heads, out_channels))
        else:
            self.lin_edge = None
            self.register_parameter("att_edge", None)
        self._init_bias(self.out_width, bias)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        a = math.sqrt(6.0 / (self.heads + self.out_channels))
        with torch.no_grad():
            self.att_src.uniform_(-a, a)
            self.att_dst.uniform_(-a, a)
            if self.att_edge is not None:
                self.att_edge.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()
        if self.lin_edge is not None:
            self.lin_edge.reset_parameters()

    def graph(self, edge_index: Tensor, num_nodes: int, segments=None) -> GraphIndex:
        # a layer with edge features lets a tagged batch take the one-launch self-loop build; without edge_dim: as before
        return graph_index(edge_index, num_nodes, segments=segments, loops_segmented=self.edge_dim is not None,
                           **self.graph_flags())

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor] = None, relu: bool = False,
                next_conv=None) -> Tensor:
        """``conv(x, edge_index)`` / ``conv(x, edge_index, edge_attr)`` as PyG; everything behind ``lin`` is one autograd
        node on fused kernels (``ops.gat_conv``, with several heads ``ops.gat_heads_conv``, with edge features
        ``ops.gat_heads_edge_conv``); ``relu=True`` also fuses the encoder's ReLU (``models/model.py:71,77``).
        ``edge_attr``: float32 ``[E, edge_dim]`` (``[E]`` with ``edge_dim=1``) in the order of ``edge_index``, on the
        device of ``x``; it enters the attention logits only.  A layer with ``edge_dim`` called without it has no edge
        term."""
        x = resolve(x)
        if edge_attr is not None:
            if isinstance(edge_attr, Tensor) and self.edge_dim is None:
                raise ValueError("edge_attr given to a GATConv built without edge_dim")
            edge_attr = _check_edge_attr(edge_attr, edge_index, self.edge_dim, hint="; pass relu= / next_conv= by keyword",
                                         width_note=f" (edge_dim = {self.edge_dim})")
        return self._dispatch(x, edge_index, relu, next_conv, self.out_width, edge_attr=edge_attr)

    def _layer(self, g: GraphIndex, x: Tensor, relu: bool, edge_attr: Optional[Tensor] = None) -> Tensor:
        h = self.lin(x)
        if self.edge_dim is not None:
            # a layer with edge features runs the multi-head kernels at every H >= 1, with or without edge_attr
            return self._layer_heads(g, h, relu, edge_attr)
        if self.heads > 1:
            return self._layer_heads(g, h, relu)
        # one head (the mean over one head is that head: either value of ``concat``): the single-head kernels
        if ops.fused_gnn_ok(h):
            return ops.gat_conv(g, h, self.att_src, self.att_dst, self.bias, self.negative_slope, relu)
        a_src = (h * self.att_src.view(1, -1)).sum(-1)
        a_dst = (h * self.att_dst.view(1, -1)).sum(-1)
        out = ops.gat_aggregate(g, h, a_src, a_dst, self.negative_slope)
        if self.bias is not None:
            out = out + self.bias
        return torch.relu(out) if relu else out

    def _layer_heads(self, g: GraphIndex, h: Tensor, relu: bool, edge_attr: Optional[Tensor] = None) -> Tensor:
        """Several heads: the per-edge work on the kernels of dc_gat_heads.hip at every width; the row-wise passes fused
        with it where ``ops.gat_heads_fused_ok``.  ``edge_attr``: the edge term of dc_gat_edge.hip joins the logits, through
        the folded ``M`` [edge_dim, H] (formed here, so autograd carries its gradient to ``lin_edge`` and ``att_edge``)."""
        nh, mean = self.heads, not self.concat
        edge_m = ops.gat_edge_fold(self.lin_edge.weight, self.att_edge) if edge_attr is not None else None
        if ops.gat_heads_fused_ok(h, nh, mean):
            if edge_attr is not None:
                return ops.gat_heads_edge_conv(g, h, self.att_src, self.att_dst, self.bias, self.negative_slope, edge_attr,
                                               edge_m, relu, nh, mean, self.fill_value)
            return ops.gat_heads_conv(g, h, self.att_src, self.att_dst, self.bias, self.negative_slope, relu, nh, mean)
        hv = h.view(-1, nh, self.out_channels)
        a_src = (hv * self.att_src).sum(-1)
        a_dst = (hv * self.att_dst).sum(-1)
        out = ops.gat_heads_aggregate(g, h, a_src, a_dst, self.negative_slope, nh, mean, edge_attr, edge_m,
                                      self.fill_value)
        if self.bias is not None:
            out = out + self.bias
        return torch.relu(out) if relu else out

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, heads={self.heads}" + ("" if self.concat else ", concat=False")
                + ("" if self.edge_dim is None else f", edge_dim={self.edge_dim}, fill_value={self.fill_value!r}"))


class GATv2Conv(_ReluConv):
    """PyG 2.5.2 ``GATv2Conv`` (dynamic attention): ``e_ij = att . leaky_relu(lin_l(x_j) + lin_r(x_i))`` per head, edge
    softmax over the incoming edges of i (self loops removed, then added), ``out_i = sum_j alpha_ij lin_l(x_j)``, the
    heads side by side (``concat``) or averaged, ``+ bias``.  Not supported, and absent from the signature as for
    ``GATConv``: attention dropout, ``add_self_loops=False``, ``edge_dim``, ``return_attention_weights``, bipartite
    input, bf16-stored input."""

    _self_loops = True

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, bias: bool = True, share_weights: bool = False):
        super().__init__()
        if heads < 1:
            raise ValueError(f"heads must be >= 1, got {heads}")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, bool(concat)
        self.negative_slope, self.share_weights = negative_slope, bool(share_weights)
        self.lin_l = _Lin(in_channels, heads * out_channels, initializer="glorot", bias=bias)
        self.lin_r = self.lin_l if share_weights else _Lin(in_channels, heads * out_channels, initializer="glorot",
                                                           bias=bias)
        # as GATConv's ``lin``: the attention vector's gradient is a sum of terms that cancel - 24-bit products
        self.lin_l.six_products = self.lin_r.six_products = True
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self._init_bias(self.out_width, bias)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        if not self.share_weights:
            self.lin_r.reset_parameters()
        a = math.sqrt(6.0 / (self.heads + self.out_channels))
        with torch.no_grad():
            self.att.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x: Tensor, edge_index: Tensor, relu: bool = False, next_conv=None) -> Tensor:
        """``conv(x, edge_index)`` as PyG; everything behind the two linears is one autograd node on the kernels of
        dc_gatv2.hip and dc_gat_heads.hip (``ops.gatv2_conv``); ``relu=True`` also fuses the ReLU that follows."""
        return self._dispatch(x, edge_index, relu, next_conv, self.out_width)

    def _layer(self, g: GraphIndex, x: Tensor, relu: bool) -> Tensor:
        xl = self.lin_l(x)
        xr = xl if self.share_weights else self.lin_r(x)
        nh, mean = self.heads, not self.concat
        if ops.gat_heads_fused_ok(xl, nh, mean):
            return ops.gatv2_conv(g, xl, xr, self.att, self.bias, self.negative_slope, relu, nh, mean)
        # widths the row-wise passes (mask, bias gradient) do not take: the per-edge kernels run all the same
        out = ops.gatv2_conv(g, xl, xr, self.att, None, self.negative_slope, False, nh, mean)
        if self.bias is not None:
            out = out + self.bias
        return torch.relu(out) if relu else out

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, heads={self.heads}" + ("" if self.concat else ", concat=False")
                + (", share_weights=True" if self.share_weights else ""))


class TransformerConv(_ReluConv):
    """PyG 2.5.2 ``TransformerConv`` (dot-product edge attention): ``e_ij = <lin_query(x_i), lin_key(x_j)> / sqrt(C)`` per
    head, edge softmax over the incoming edges of i - the edge set exactly as given: no self loop is removed or added,
    a node without in-edges aggregates 0 - ``out_i = sum_j alpha_ij lin_value(x_j)``, the heads side by side
    (``concat``) or averaged; with ``root_weight`` ``+ lin_skip(x_i)``, with ``beta`` blended with it by the gate
    ``sigmoid(lin_beta([out, r, out - r]))``.  ``bias`` governs ``lin_skip`` alone, which exists (and loads) also with
    ``root_weight=False``, where it is not used.  Not supported, and absent from the signature: attention dropout,
    ``edge_dim``, ``return_attention_weights``, bipartite input, bf16-stored input.  ``beta=True`` needs
    ``root_weight`` (PyG silently ignores the gate without it; here it is a ``ValueError``)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, beta: bool = False,
                 bias: bool = True, root_weight: bool = True):
        super().__init__()
        if heads < 1:
            raise ValueError(f"heads must be >= 1, got {heads}")
        if beta and not root_weight:
            raise ValueError("beta=True gates the skip connection: it needs root_weight=True")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, bool(concat)
        self.beta, self.root_weight = bool(beta), bool(root_weight)
        self.lin_key = _Lin(in_channels, heads * out_channels, bias=True)
        self.lin_query = _Lin(in_channels, heads * out_channels, bias=True)
        self.lin_value = _Lin(in_channels, heads * out_channels, bias=True)
        self.lin_skip = _Lin(in_channels, self.out_width, bias=bias)
        # the logit is a product of two linear outputs and feeds an exponential: 24-bit products in all of them
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
            lin.six_products = True
        self.lin_beta = _Lin(3 * self.out_width, 1) if beta else None

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, relu: bool = False, next_conv=None) -> Tensor:
        """``conv(x, edge_index)`` as PyG; the attention behind the three linears is one autograd node on the kernels of
        dc_transformer.hip and dc_gat_heads.hip (``ops.transformer_conv``), the skip connection and the gate are torch
        ops.  ``relu=True``: the ReLU that follows runs in the aggregation's epilogue with ``root_weight=False`` at
        widths that pass ``ops.gat_heads_fused_ok``, else as a ``torch.relu`` behind the skip / gate."""
        # (no node: no adjacency to build, and ``ops.transformer_conv`` launches nothing)
        return self._dispatch(x, edge_index, relu, next_conv, self.out_width, empty_none=True)

    def _layer(self, g: Optional[GraphIndex], x: Tensor, relu: bool) -> Tensor:
        q, k, v = self.lin_query(x), self.lin_key(x), self.lin_value(x)
        nh, mean = self.heads, not self.concat
        if not self.root_weight:
            fused = relu and ops.gat_heads_fused_ok(v, nh, mean)
            out = ops.transformer_conv(g, q, k, v, None, fused, nh, mean)
            return torch.relu(out) if relu and not fused else out
        out = ops.transformer_conv(g, q, k, v, None, False, nh, mean)
        r = self.lin_skip(x)
        if self.lin_beta is not None:
            b = torch.sigmoid(torch.nn.functional.linear(torch.cat([out, r, out - r], dim=-1), self.lin_beta.weight))
            out = b * r + (1 - b) * out
        else:
            out = out + r
        return torch.relu(out) if relu else out

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, heads={self.heads}" + ("" if self.concat else ", concat=False")
                + (", beta=True" if self.beta else "") + ("" if self.root_weight else ", root_weight=False"))


class SAGEConv(_ReluConv):
    """PyG 2.5.2 ``SAGEConv`` (GraphSAGE): ``out_i = lin_l(aggr_j x_j)`` over the incoming edges of i - the edge set
    exactly as given: no self loop is removed or added, duplicates count, a node without in-edges aggregates 0 - with
    ``root_weight`` ``+ lin_r(x_i)``, with ``normalize`` followed by ``F.normalize(out, p=2, dim=-1)``.  With ``project``
    the SOURCE features are ``relu(lin(x))``; the root term keeps the raw ``x``.  ``bias`` governs ``lin_l`` alone
    (``lin_r`` has none, ``lin`` always has one).  ``aggr``: ``"mean"``, ``"max"``, ``"sum"`` or its alias ``"add"``,
    on ``ops.aggregate``; the max sends the gradient of every maximum in EQUAL shares to all edges that attain it
    (INTEGRATION.md 1.5).  Not supported: any other ``aggr`` (lists and aggregation modules included; a
    ``ValueError``), and - absent from the signature - bipartite ``(x_src, x_dst)`` input, ``size=``, bf16-stored
    input."""

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean", normalize: bool = False,
                 root_weight: bool = True, project: bool = False, bias: bool = True):
        super().__init__()
        if not isinstance(in_channels, int):
            raise TypeError("SAGEConv: bipartite input (a pair of in_channels) is not supported")
        if not isinstance(aggr, str) or aggr not in ("mean", "max", "sum", "add"):
            raise ValueError(f"aggr must be 'mean', 'max', 'sum' or 'add', got {aggr!r}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aggr = "sum" if aggr == "add" else aggr
        self.normalize, self.root_weight, self.project = bool(normalize), bool(root_weight), bool(project)
        self.lin = _Lin(in_channels, in_channels, bias=True) if project else None
        self.lin_l = _Lin(in_channels, out_channels, bias=bias)
        self.lin_r = _Lin(in_channels, out_channels, bias=False) if root_weight else None

    def reset_parameters(self):
        for lin in (self.lin, self.lin_l, self.lin_r):
            if lin is not None:
                lin.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, relu: bool = False, next_conv=None) -> Tensor:
        """``conv(x, edge_index)`` as PyG; the aggregation is one autograd node on the kernels of dc_sage.hip (the sum:
        the unweighted hop), the linears run on the dense block.  ``relu=True``: the ReLU that follows runs in
        ``lin_l``'s epilogue when nothing stands between them (``root_weight=False, normalize=False``), else as a
        ``torch.relu`` behind the layer."""
        # (no node: no adjacency to build, and ``ops.aggregate`` launches nothing)
        return self._dispatch(x, edge_index, relu, next_conv, self.out_channels, empty_none=True)

    def _layer(self, g: Optional[GraphIndex], x: Tensor, relu: bool) -> Tensor:
        src = ops.dense_linear(x, self.lin.weight, self.lin.bias, relu=True) if self.lin is not None else x
        agg = ops.aggregate(g, src, self.aggr)
        if self.lin_r is None and not self.normalize:
            return ops.dense_linear(agg, self.lin_l.weight, self.lin_l.bias, relu=relu)
        out = self.lin_l(agg)
        if self.lin_r is not None:
            out = out + self.lin_r(x)
        if self.normalize:
            out = torch.nn.functional.normalize(out, p=2.0, dim=-1)
        return torch.relu(out) if relu else out

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}" + (", normalize=True" if self.normalize else "")
                + ("" if self.root_weight else ", root_weight=False") + (", project=True" if self.project else ""))


class ChebConv(_ReluConv):
    """PyG 2.5.2 ``ChebConv`` (Chebyshev spectral convolution): ``out = sum_k lins[k](Tx_k) + bias`` with ``Tx_0 = x``,
    ``Tx_1 = L^ x``, ``Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2}`` and ``L^ = 2 L / lambda_max - I`` the scaled Laplacian of
    ``get_laplacian``: self loops in ``edge_index`` are DROPPED and none is added, duplicates count, the degree is the
    OUT-degree over what remains (``deg[j]`` = edges with source j), the weight of an edge j -> i is
    ``-deg_j^-1/2 deg_i^-1/2`` (``"sym"``, ``deg = 0 -> 0``) or ``-1 / deg_j`` (``"rw"``), and every node - an isolated one
    too - has the diagonal term ``2 / lambda_max - 1``.  ``lambda_max``: None (2.0, the largest value PyG's default can
    take) or a Python number > 0.  ``K = 1`` is a plain linear layer and builds no adjacency.  The basis is one autograd
    node on the kernels of dc_cheb.hip (``ops.cheb_basis``), the K linears ONE product of the dense block over it.
    ``batch`` is accepted and ignored (PyG uses it for per-graph ``lambda_max`` only).  Not supported, each a worded
    error: ``edge_weight`` other than None; ``normalization=None``; a tensor ``lambda_max`` (per-graph values included)
    and ``lambda_max <= 0``; bipartite input; bf16-stored input."""

    # the edge set as given: the loops are dropped by their weight, the normalisation is the layer's own (dc_cheb_norm)
    _self_loops, _gcn_norm = False, False

    def __init__(self, in_channels: int, out_channels: int, K: int, normalization: Optional[str] = "sym",
                 bias: bool = True):
        super().__init__()
        if not isinstance(in_channels, int):
            raise TypeError("ChebConv: bipartite input (a pair of in_channels) is not supported")
        if not isinstance(K, int) or isinstance(K, bool) or K < 1:
            raise ValueError(f"ChebConv: K must be an int >= 1, got {K!r}")
        if normalization is None:
            raise NotImplementedError("ChebConv: normalization=None (the unnormalised Laplacian, whose lambda_max PyG "
                                      "does not default) is not supported; use 'sym' or 'rw'")
        if normalization not in ops.CHEB_MODES:
            raise ValueError(f"ChebConv: normalization must be 'sym' or 'rw', got {normalization!r}")
        self.in_channels, self.out_channels, self.K, self.normalization = in_channels, out_channels, K, normalization
        self.lins = nn.ModuleList([_Lin(in_channels, out_channels, initializer="glorot") for _ in range(K)])
        self._init_bias(out_channels, bias)

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight=None, batch=None, lambda_max=None, *,
                relu: bool = False, next_conv=None) -> Tensor:
        """``conv(x, edge_index, edge_weight=None, batch=None, lambda_max=None)`` in PyG's positional order;
        ``relu=True`` fuses the ReLU that follows into the dense block's epilogue, and a plain call returns the deferred
        result of the other layers."""
        if edge_weight is not None:
            raise NotImplementedError("ChebConv: edge_weight is not supported (the Laplacian is built from the edge "
                                      "set alone); pass None")
        lam = ops.cheb_lambda(lambda_max, "ChebConv")
        if isinstance(x, (tuple, list)):
            raise TypeError("ChebConv: bipartite input (x_src, x_dst) is not supported")
        x = resolve(x)
        if isinstance(x, Tensor) and x.dtype == torch.bfloat16:
            raise NotImplementedError("ChebConv: bf16-stored input is not supported; pass float32")

        def layer(g, x, act):
            return self._layer(g, x, act, lam)
        return self._dispatch(x, edge_index, relu, next_conv, self.out_channels, empty_none=True, layer=layer)

    def graph(self, edge_index: Tensor, num_nodes: int, segments=None) -> Optional[GraphIndex]:
        # K = 1 is x @ W^T + bias: no adjacency
        return super().graph(edge_index, num_nodes, segments=segments) if self.K > 1 else None

    def _layer(self, g: Optional[GraphIndex], x: Tensor, relu: bool, lam: float = 2.0) -> Tensor:
        slab = ops.cheb_basis(g, x, self.K, self.normalization, lam)
        weight = torch.cat([lin.weight for lin in self.lins], 1) if self.K > 1 else self.lins[0].weight
        return ops.dense_linear(slab, weight, self.bias, relu=relu)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, K={self.K}, normalization={self.normalization}"


class GMMConv(_ReluConv):
    """PyG 2.5.2 ``GMMConv`` (MoNet, the Gaussian-mixture mesh convolution) with ``separate_gaussians=False``:
    ``out_i = aggr_{j->i} sum_k w_k(e_ji) (x_j @ g)[k*M:(k+1)*M] + root(x_i) + bias`` with ``w_k(e) = exp(sum_d -0.5
    (e_d - mu[k,d])^2 / (1e-15 + sigma[k,d]^2))``, ``e = edge_attr`` the D-dimensional pseudo-coordinates of an edge,
    ``M = out_channels``, ``K = kernel_size``, ``D = dim``.  The edge set exactly as given: no self loop is removed or
    added, duplicates count (in the degree of ``"mean"`` too), a node without in-edges aggregates 0.  ``aggr``:
    ``"mean"`` (PyG's default) or ``"add"``.  Parameters as PyG: ``g [in, K*M]``, ``mu`` / ``sigma [K, D]``,
    ``root.weight [M, in]`` with ``root_weight``, ``bias [M]`` - glorot, the bias zeros.  ``x @ g`` and the root linear
    run on the dense block; the aggregation with the root term (and the ReLU of ``relu=True`` where the width allows,
    ``ops.gmm_relu_ok``) is one autograd node on the kernels of dc_gmm.hip (``ops.gmm_aggregate``), which read ``mu`` and
    ``sigma`` on the device.  ``1 <= kernel_size <= 64``, ``1 <= dim <= 16``.  Not supported, each
    a worded error: ``separate_gaussians=True``, bipartite input (a pair of ``in_channels``, a pair ``x``),
    ``aggr="max"``, bf16-stored input."""

    def __init__(self, in_channels: int, out_channels: int, dim: int, kernel_size: int,
                 separate_gaussians: bool = False, aggr: str = "mean", root_weight: bool = True, bias: bool = True):
        super().__init__()
        if separate_gaussians:
            raise NotImplementedError("GMMConv: separate_gaussians=True (one mixture per input channel) is not "
                                      "supported")
        if not isinstance(in_channels, int):
            raise NotImplementedError("GMMConv: bipartite input (a pair of in_channels) is not supported")
        if aggr == "max":
            raise NotImplementedError("GMMConv: aggr='max' is not supported; use 'mean' or 'add'")
        if not isinstance(aggr, str) or aggr not in ops.GMM_REDUCES:
            raise ValueError(f"GMMConv: aggr must be 'mean' or 'add', got {aggr!r}")
        for name, v, cap in (("kernel_size", kernel_size, ops.GMM_MAX_K), ("dim", dim, ops.GMM_MAX_D)):
            if not isinstance(v, int) or isinstance(v, bool) or not 1 <= v <= cap:
                raise ValueError(f"GMMConv: {name} must be an int within 1..{cap}, got {v!r}")
        self.in_channels, self.out_channels, self.dim, self.kernel_size = in_channels, out_channels, dim, kernel_size
        self.separate_gaussians, self.root_weight, self.aggr = False, bool(root_weight), aggr
        self.g = nn.Parameter(torch.empty(in_channels, out_channels * kernel_size))
        self.mu = nn.Parameter(torch.empty(kernel_size, dim))
        self.sigma = nn.Parameter(torch.empty(kernel_size, dim))
        self.root = _Lin(in_channels, out_channels, initializer="glorot") if root_weight else None
        self._init_bias(out_channels, bias)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for p in (self.g, self.mu, self.sigma):
                a = math.sqrt(6.0 / (p.size(-2) + p.size(-1)))
                p.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()
        if self.root is not None:
            self.root.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor] = None, relu: bool = False,
                next_conv=None) -> Tensor:
        """``conv(x, edge_index, edge_attr)`` as PyG.  ``edge_attr``: float32 ``[E, dim]`` (``[E]`` where ``dim`` is 1)
        with rows in the order of ``edge_index``, on the device of ``x``.  ``relu=True`` runs the ReLU that follows in
        the aggregation's epilogue (behind the layer at a width the mask pass does not take), and a plain call returns
        the deferred result of the other layers."""
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("GMMConv: bipartite input (x_src, x_dst) is not supported")
        x = resolve(x)
        if isinstance(x, Tensor) and x.dtype == torch.bfloat16:
            raise NotImplementedError("GMMConv: bf16-stored input is not supported; pass float32")
        if edge_attr is None:
            raise ValueError("GMMConv needs edge_attr: conv(x, edge_index, edge_attr)")
        edge_attr = _check_edge_attr(edge_attr, edge_index, self.dim, width_note=" (dim pseudo-coordinates per edge)")
        if edge_attr.size(0) > 0 and edge_attr.size(1) > 1 and edge_attr.stride(1) != 1:
            raise ValueError("edge_attr: innermost dimension must be contiguous")
        return self._dispatch(x, edge_index, relu, next_conv, self.out_channels, empty_none=True, edge_attr=edge_attr)

    def _layer(self, g: Optional[GraphIndex], x: Tensor, relu: bool, edge_attr: Tensor) -> Tensor:
        h = ops.dense_linear(x, self.g.t())
        # the root term with the bias is the gather's addend; a bias without a root term is added behind it
        base = ops.dense_linear(x, self.root.weight, self.bias) if self.root is not None else None
        late_bias = self.bias if self.root is None else None
        fused = relu and late_bias is None and ops.gmm_relu_ok(self.out_channels)
        out = ops.gmm_aggregate(g, h, edge_attr, self.mu, self.sigma, self.aggr, base, fused)
        if late_bias is not None:
            out = out + late_bias
        return torch.relu(out) if relu and not fused else out

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, dim={self.dim}"

    def __repr__(self) -> str:                                   # (PyG's one line, without the ``root`` child)
        return f"{self.__class__.__name__}({self.extra_repr()})"


class SplineConv(_ReluConv):
    """PyG 2.5.2 ``SplineConv`` (SplineCNN, the B-spline mesh convolution) with torch-spline-conv's basis and weighting:
    ``out_i = aggr_{j->i} sum_s b_s(e_ji) (x_j @ weight[wi_s(e_ji)]) + lin(x_i) + bias``, ``e = edge_attr`` the
    D-dimensional pseudo-coordinates of an edge in [0, 1], ``M = out_channels``, ``D = dim``.  Per dimension an open or
    closed B-spline of ``degree`` 1..3 with ``kernel_size[d]`` control points: an edge touches ``S = (degree+1)^D`` of
    the ``K = prod kernel_size`` weight matrices (INTEGRATION.md 1.9 states the basis and the index).  The edge set
    exactly as given: no self loop is removed or added, duplicates count (in the degree of ``"mean"`` too), a node
    without in-edges aggregates 0.  ``aggr``: ``"mean"`` (PyG's default) or ``"add"``.  Parameters as PyG: ``weight
    [K, in, M]``, ``lin.weight [M, in]`` with ``root_weight``, ``bias [M]``, and the buffers ``kernel_size`` /
    ``is_open_spline``; the kernels use the constructor's Python values, never the buffers.  ``x @ weight[k]`` for all
    k (one ``[N, K*M]`` product) and the root linear run on the dense block; the aggregation with the root term (and the
    ReLU of ``relu=True`` where the width allows, ``ops.gmm_relu_ok``) is one autograd node on the kernels of
    dc_spline.hip (``ops.spline_aggregate``).  Coordinates outside [0, 1] wrap (no out-of-bounds read), NaN propagates.
    ``1 <= dim <= 4``, ``S <= 64``, ``K <= 1024``.  Not supported, each a worded error: bipartite input (a pair of
    ``in_channels``, a pair ``x``), lazy ``in_channels``, ``aggr="max"``, bf16-stored input."""

    def __init__(self, in_channels: int, out_channels: int, dim: int, kernel_size, is_open_spline=True, degree: int = 1,
                 aggr: str = "mean", root_weight: bool = True, bias: bool = True):
        super().__init__()
        if isinstance(in_channels, (tuple, list)):
            raise NotImplementedError("SplineConv: bipartite input (a pair of in_channels) is not supported")
        if not isinstance(in_channels, int) or in_channels <= 0:
            raise NotImplementedError(f"SplineConv: in_channels must be a positive int (lazy initialisation is not "
                                      f"supported), got {in_channels!r}")
        if aggr == "max":
            raise NotImplementedError("SplineConv: aggr='max' is not supported; use 'mean' or 'add'")
        if not isinstance(aggr, str) or aggr not in ops.SPLINE_REDUCES:
            raise ValueError(f"SplineConv: aggr must be 'mean' or 'add', got {aggr!r}")
        self._geom = ops.spline_geometry(kernel_size, is_open_spline, degree, dim, who="SplineConv")
        ks, op, _, k, _ = self._geom
        self.in_channels, self.out_channels, self.dim, self.degree = in_channels, out_channels, dim, degree
        self.root_weight, self.aggr = bool(root_weight), aggr
        self.register_buffer("kernel_size", torch.tensor(ks, dtype=torch.long))
        self.register_buffer("is_open_spline", torch.tensor(op, dtype=torch.uint8))
        self.weight = nn.Parameter(torch.empty(k, in_channels, out_channels))
        self.lin = _Lin(in_channels, out_channels) if root_weight else None
        self._init_bias(out_channels, bias)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            a = 1.0 / math.sqrt(self.weight.size(0) * self.weight.size(1))
            self.weight.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()
        if self.lin is not None:
            self.lin.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor] = None, relu: bool = False,
                next_conv=None) -> Tensor:
        """``conv(x, edge_index, edge_attr)`` as PyG.  ``edge_attr``: float32 ``[E, dim]`` (``[E]`` where ``dim`` is 1)
        in [0, 1] with rows in the order of ``edge_index``, on the device of ``x``.  ``relu=True`` runs the ReLU that
        follows in the aggregation's epilogue (behind the layer at a width the mask pass does not take), and a plain
        call returns the deferred result of the other layers."""
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("SplineConv: bipartite input (x_src, x_dst) is not supported")
        x = resolve(x)
        if isinstance(x, Tensor) and x.dtype == torch.bfloat16:
            raise NotImplementedError("SplineConv: bf16-stored input is not supported; pass float32")
        if edge_attr is None:
            raise ValueError("SplineConv needs edge_attr: conv(x, edge_index, edge_attr)")
        edge_attr = _check_edge_attr(edge_attr, edge_index, self.dim, width_note=" (dim pseudo-coordinates per edge)")
        if edge_attr.size(0) > 0 and edge_attr.size(1) > 1 and edge_attr.stride(1) != 1:
            raise ValueError("edge_attr: innermost dimension must be contiguous")
        return self._dispatch(x, edge_index, relu, next_conv, self.out_channels, empty_none=True, edge_attr=edge_attr)

    def _layer(self, g: Optional[GraphIndex], x: Tensor, relu: bool, edge_attr: Tensor) -> Tensor:
        ks, op, degree, k, _ = self._geom
        # [K, in, M] -> [K*M, in]: row k*M + c is column c of weight[k] (a torch copy: autograd carries g_weight)
        w2 = self.weight.permute(0, 2, 1).reshape(k * self.out_channels, self.in_channels)
        h = ops.dense_linear(x, w2)
        # the root term with the bias is the gather's addend; a bias without a root term is added behind it
        base = ops.dense_linear(x, self.lin.weight, self.bias) if self.lin is not None else None
        late_bias = self.bias if self.lin is None else None
        fused = relu and late_bias is None and ops.gmm_relu_ok(self.out_channels)
        out = ops.spline_aggregate(g, h, edge_attr, ks, op, degree, self.aggr, base, fused)
        if late_bias is not None:
            out = out + late_bias
        return torch.relu(out) if relu and not fused else out

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, dim={self.dim}"

    def __repr__(self) -> str:                                   # (PyG's one line, without the ``lin`` child)
        return f"{self.__class__.__name__}({self.extra_repr()})"


def _reset_module(module: nn.Module) -> None:
    """PyG's ``inits.reset``: a module's own ``reset_parameters`` if it has one, else that of its children."""
    if hasattr(module, "reset_parameters"):
        module.reset_parameters()
    else:
        for child in module.children():
            _reset_module(child)


class _GinBase(_ConvBase):
    """What ``GINConv`` and ``GINEConv`` share: the user's ``nn``, ``eps`` as a float32 ``[1]`` tensor named ``eps`` (a
    Parameter with ``train_eps``, else a buffer), the edge set taken as it is given."""

    def __init__(self, nn_: nn.Module, eps: float, train_eps: bool):
        super().__init__()
        self.nn = nn_
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = nn.Parameter(torch.empty(1))
        else:
            self.register_buffer("eps", torch.empty(1))
        self.eps.data.fill_(self.initial_eps)

    def reset_parameters(self):
        _reset_module(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(nn={self.nn})"


class GINConv(_GinBase):
    """PyG 2.5.2 ``GINConv`` (graph isomorphism): ``out_i = nn((1 + eps) x_i + sum_j x_j)`` over the incoming edges
    of i - the edge set exactly as given: no self loop is removed or added, duplicates count, a node without in-edges
    gets ``(1 + eps) x_i``.  ``nn`` is any ``torch.nn.Module`` and is called as it is; the layer's result is ``nn``'s
    result, so there is no ``relu=`` / ``next_conv=`` and no deferred result.  ``eps``: a ``[1]`` tensor in
    ``state_dict`` either way, a Parameter with ``train_eps``.  The sum is the unweighted hop (``ops.aggregate(...,
    "sum")``), the root term a torch op.  Not supported, and absent from the signature: bipartite ``(x_src, x_dst)``
    input, ``size=``, bf16-stored input."""

    def __init__(self, nn: nn.Module, eps: float = 0.0, train_eps: bool = False):
        super().__init__(nn, eps, train_eps)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        """``conv(x, edge_index)`` as PyG; a deferred ``x`` is resolved."""
        x = resolve(x)
        _check_inputs(x, edge_index, x.size(1) if x.dim() == 2 else -1)
        g = self.graph(edge_index, x.size(0)) if x.size(0) else None
        return self.nn((1 + self.eps) * x + ops.aggregate(g, x, "sum"))


class GINEConv(_GinBase):
    """PyG 2.5.2 ``GINEConv`` (GIN with edge features): ``out_i = nn((1 + eps) x_i + sum_j relu(x_j + e_ji))`` over
    the incoming edges of i - the edge set exactly as given: no self loop is removed or added, duplicates count, a node
    without in-edges gets ``(1 + eps) x_i``.  With ``edge_dim`` ``e = lin(edge_attr)`` (``lin``: ``edge_dim ->
    in_channels`` with a bias, on the dense block; ``in_channels`` inferred from ``nn`` as PyG does), without it
    ``e = edge_attr``, whose width must then be ``x``'s.  The aggregation with the root term is one autograd node on
    the kernels of dc_gine.hip (``ops.gine_aggregate``): the ReLU mask is recomputed in the backward, ``relu'(0) = 0``,
    and ``eps`` is read on the device, so a trained ``eps`` may change between replays of a captured step
    (INTEGRATION.md 1.6).  ``nn`` is any ``torch.nn.Module`` and is called as it is; the layer's result is ``nn``'s
    result, so there is no ``relu=`` / ``next_conv=`` and no deferred result.  Not supported, and absent from the
    signature: bipartite ``(x_src, x_dst)`` input, ``size=``, bf16-stored input."""

    def __init__(self, nn: nn.Module, eps: float = 0.0, train_eps: bool = False, edge_dim: Optional[int] = None):
        super().__init__(nn, eps, train_eps)
        self.edge_dim = edge_dim
        if edge_dim is not None:
            first = nn[0] if isinstance(nn, torch.nn.Sequential) else nn
            if hasattr(first, "in_features"):
                in_channels = first.in_features
            elif hasattr(first, "in_channels"):
                in_channels = first.in_channels
            else:
                raise ValueError("Could not infer input channels from `nn`.")
            self.lin = _Lin(edge_dim, in_channels, bias=True)
        else:
            self.lin = None

    def reset_parameters(self):
        super().reset_parameters()
        if self.lin is not None:
            self.lin.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor] = None) -> Tensor:
        """``conv(x, edge_index, edge_attr)`` as PyG.  ``edge_attr``: float32 ``[E, edge_dim]`` (``[E]`` where that
        width is 1; without ``edge_dim`` ``[E, in_channels]``) with rows in the order of ``edge_index``, on the device
        of ``x``; a column slice passes.  A deferred ``x`` or ``edge_attr`` is resolved."""
        x = resolve(x)
        edge_attr = self._check_edge_attr(edge_attr, edge_index, x)
        _check_inputs(x, edge_index, self.lin.out_channels if self.lin is not None else (x.size(1) if x.dim() == 2
                                                                                          else -1))
        _require_cuda(edge_attr, "edge_attr")
        if edge_attr.device != x.device:
            raise RuntimeError(f"x is on {x.device} but edge_attr is on {edge_attr.device}")
        g = self.graph(edge_index, x.size(0)) if x.size(0) else None
        if self.lin is None:
            e = edge_attr
        elif edge_attr.size(0) == 0:
            e = torch.nn.functional.linear(edge_attr, self.lin.weight, self.lin.bias)    # no edge: nothing to launch
        else:
            e = self.lin(edge_attr.contiguous())
        return self.nn(ops.gine_aggregate(g, x, e, self.eps))

    def _check_edge_attr(self, edge_attr, edge_index, x: Tensor) -> Tensor:
        """``_check_edge_attr`` at the width of ``edge_dim``, or of ``x`` without it, and the layer's own checks."""
        if edge_attr is None:
            raise ValueError("GINEConv needs edge_attr: conv(x, edge_index, edge_attr)")
        mismatch = None
        if self.edge_dim is None:
            def mismatch(e):
                return ("Node and edge feature dimensionalities do not match. Consider setting the 'edge_dim' "
                        f"attribute of 'GINEConv' (x has {x.size(1)} columns, edge_attr {e.size(1)})")
        width = self.edge_dim if self.edge_dim is not None else (x.size(1) if x.dim() == 2 else -1)
        edge_attr = _check_edge_attr(edge_attr, edge_index, width, mismatch=mismatch)
        if edge_attr.size(0) > 0 and edge_attr.size(1) > 1 and edge_attr.stride(1) != 1:
            raise ValueError("edge_attr: innermost dimension must be contiguous")
        return edge_attr


class EdgeConv(_ConvBase):
    """PyG 2.5.2 ``EdgeConv`` (the layer of DGCNN): ``out_i = aggr_j nn([x_i, x_j - x_i])`` over the incoming edges
    ``j -> i`` - the edge set exactly as given: no self loop is removed or added, duplicates count, a node without
    in-edges gets 0.  ``nn`` is any ``torch.nn.Module`` and is called as it is, once, on the ``[E, 2 * in]`` rows of all
    edges in the order of ``edge_index``; its result must be float32 ``[E, C]``.  ``aggr``: ``"max"`` (default),
    ``"mean"``, ``"sum"`` or its alias ``"add"``.  The pair rows and the reduction are one autograd node each on the
    kernels of dc_edge.hip (``ops.edge_pairs``, ``ops.edge_aggregate``): every sum in a fixed order, no float atomics,
    and the gradient of a maximum goes in equal shares to all edges that attain it.  The
    layer's result is the reduction's, so there is no ``relu=`` / ``next_conv=`` and no deferred result.  Not
    supported: bipartite ``(x_src, x_dst)`` input (a ``TypeError``), aggregation lists or modules, bf16-stored input."""

    def __init__(self, nn: nn.Module, aggr: str = "max"):
        super().__init__()
        if not isinstance(aggr, str) or aggr not in ("max", "mean", "sum", "add"):
            raise ValueError(f"EdgeConv: aggr must be 'max', 'mean', 'sum' or 'add', got {aggr!r}")
        self.nn = nn
        self.aggr = "sum" if aggr == "add" else aggr

    def reset_parameters(self):
        _reset_module(self.nn)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        """``conv(x, edge_index)`` as PyG; a deferred ``x`` is resolved."""
        if isinstance(x, (tuple, list)):
            raise TypeError("EdgeConv: bipartite (x_src, x_dst) input is not supported; pass one [N, F] tensor")
        x = resolve(x)
        _check_inputs(x, edge_index, x.size(1) if x.dim() == 2 else -1)
        g = self.graph(edge_index, x.size(0)) if x.size(0) else None
        z = ops.edge_pairs(g, x)
        m = resolve(self.nn(z))              # (no edge: nn sees the empty [0, 2F] tensor and tells the output's width)
        if not isinstance(m, Tensor) or m.dim() != 2 or m.dtype != torch.float32 or m.size(0) != z.size(0) \
                or m.size(1) == 0:
            got = f"{tuple(m.shape)} {m.dtype}" if isinstance(m, Tensor) else type(m).__name__
            raise ValueError(f"EdgeConv: nn must return a float32 [E, C >= 1] tensor with E = {z.size(0)} rows, got {got}")
        return ops.edge_aggregate(g, m, self.aggr)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(nn={self.nn})"


class DynamicEdgeConv(EdgeConv):
    """PyG 2.5.2 ``DynamicEdgeConv`` (DGCNN): ``EdgeConv`` on the kNN graph of its own input, rebuilt in feature space
    at every call - ``conv(x, batch=None)`` is ``EdgeConv(nn, aggr)(x, knn_graph(x, k, batch, loop=True))``, i.e. PyG's
    ``knn(x, x, k, batch, batch).flip([0])``: every point is among its own ``k`` neighbours, a graph with fewer than
    ``k`` points gives all of them.  ``x``: float32 ``[N, F]`` of any width ``F >= 1`` on the device; ``batch``: sorted
    int64 graph ids or None.  The search runs on the device (``neighbors.knn_graph``: three columns take the grid
    search, any other width the exact brute force of dc_neighbors_nd.hip; rules 2-5 of ``neighbors``, so the edge set is
    bit-for-bit reproducible) on ``x.detach()`` - no gradient goes through the choice of neighbours, as in PyG; the
    gradient is ``EdgeConv``'s.  With ``batch`` the edge list carries the batch layout and the layer takes the one-launch
    segmented adjacency build.  ``1 <= k <= 64`` (``neighbors.MAX_CAP``); ``num_workers`` is accepted and ignored.  The
    layer reads the edge total on the host, as ``knn_graph`` does, so it is not capturable (a form on the padded
    neighbour array is a later change).  Not supported: bipartite ``(x_src, x_dst)`` / ``(batch_src, batch_dst)`` input
    (a ``TypeError``), ``cosine`` search, and what ``EdgeConv`` does not support."""

    def __init__(self, nn: nn.Module, k: int, aggr: str = "max", num_workers: int = 1):
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_CAP:
            raise ValueError(f"DynamicEdgeConv: k must be an integer in [1, {MAX_CAP}], got {k!r}")
        if not isinstance(aggr, str) or aggr not in ("max", "mean", "sum", "add"):
            raise ValueError(f"DynamicEdgeConv: aggr must be 'max', 'mean', 'sum' or 'add', got {aggr!r}")
        super().__init__(nn, aggr)
        self.k = k
        self.num_workers = num_workers

    def forward(self, x: Tensor, batch: Optional[Tensor] = None) -> Tensor:
        """``conv(x, batch)`` as PyG; a deferred ``x`` is resolved."""
        if isinstance(x, (tuple, list)) or isinstance(batch, (tuple, list)):
            raise TypeError("DynamicEdgeConv: bipartite (x_src, x_dst) / (batch_src, batch_dst) input is not "
                            "supported; pass one [N, F] tensor and one batch vector")
        x = resolve(x)
        if not isinstance(x, Tensor):
            raise TypeError(f"DynamicEdgeConv: x must be a tensor, got {type(x).__name__}")
        if x.dim() != 2:
            raise ValueError("Static graphs not supported in DynamicEdgeConv")
        edge_index = knn_graph(x.detach(), self.k, batch, loop=True, flow="source_to_target")
        return super().forward(x, edge_index)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(nn={self.nn}, k={self.k})"


def _pointnet_pos(pos, what: str) -> Tensor:
    """One position operand of ``PointNetConv``, checked in the order type, dtype, shape - before the device check of
    ``neighbors._check_points``, which repeats them and adds the stride rule."""
    if not isinstance(pos, Tensor):
        raise TypeError(f"PointNetConv: {what} must be a tensor, got {type(pos).__name__}")
    if pos.dtype != torch.float32:
        raise ValueError(f"PointNetConv: {what} must be float32, got {pos.dtype}")
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError(f"PointNetConv: {what} must be [N, 3] positions (position widths other than 3 are not "
                         f"supported), got {tuple(pos.shape)}")
    return pos


class PointNetConv(_ConvBase):
    """PyG 2.5.2 ``PointNetConv`` (the set-abstraction layer of PointNet++): ``out_i = global_nn(aggr_j local_nn([x_j,
    pos_j - pos_i]))`` over the incoming edges ``j -> i``.  Call ``conv(x, pos, edge_index)``.  ``x``: None (the message
    is the 3 position columns alone), a float32 ``[Ns, F]`` tensor, or a pair ``(x_src, x_dst)`` of which only ``x_src``
    is read, as in PyG (``x_dst`` may be None).  ``pos``: float32 ``[N, 3]`` or a pair ``(pos_src [Ns, 3], pos_dst
    [Nd, 3])``, as ``neighbors`` takes positions (on the device, a row stride allowed).  The output has ``Nd`` rows.
    ``local_nn`` and ``global_nn`` are any ``torch.nn.Module`` or None and are called as they are, once: ``local_nn`` on
    the ``[E', F + 3]`` rows of all edges in the order of ``edge_index``; its result must be float32 ``[E', C]``.  Where
    ``F % 4 == 0`` those rows come as a NON-CONTIGUOUS view (unit inner stride, row stride ``F + 4``, the padding column
    zero) - ``Linear``, norms and activations take it as it is; a module that calls ``.view()`` on its input must call
    ``.contiguous()`` first (``ops.POINTNET_PAD_Z = False`` gives contiguous rows everywhere).
    ``aggr``: ``"max"`` (default), ``"mean"``, ``"sum"`` or its alias ``"add"``.

    BIPARTITE input - a pair ``pos`` or ``x`` - needs ``add_self_loops=False`` (the form PointNet++ uses); with the
    default ``True`` it is a ``ValueError``.  ``add_self_loops=True`` on one node set is PyG's remove-then-add without a
    host read: ``E' = E + N``, the input edges in input order, then node ``i``'s loop at row ``E + i`` with the message
    row ``[x_i, 0, 0, 0]``; an input edge with ``src == dst`` keeps its row - ``local_nn`` sees it - but its result takes
    no part in the reduction and its gradient row is zero.

    The pair rows and the reduction are one autograd node each on the kernels of dc_pointnet.hip and dc_edge.hip
    (``ops.pointnet_pairs``, ``ops.pointnet_aggregate``): every sum in a fixed order, no float atomics, the gradient of
    a maximum in equal shares to all edge rows that attain it, forward and backward
    capturable.  The layer's result is ``global_nn``'s (or the reduction's), so there is no ``relu=`` / ``next_conv=`` and
    no deferred result; a deferred ``x`` is resolved.  Not supported: position widths other than 3, aggregation lists or
    modules, bf16-stored input, the deprecated ``PointConv`` name, ``SparseTensor`` adjacencies, ``PPFConv`` / ``XConv``."""

    def __init__(self, local_nn: Optional[nn.Module] = None, global_nn: Optional[nn.Module] = None,
                 add_self_loops: bool = True, aggr: str = "max"):
        super().__init__()
        if not isinstance(aggr, str) or aggr not in ("max", "mean", "sum", "add"):
            raise ValueError(f"PointNetConv: aggr must be 'max', 'mean', 'sum' or 'add', got {aggr!r}")
        self.local_nn = local_nn
        self.global_nn = global_nn
        self.add_self_loops = bool(add_self_loops)
        self._self_loops = self.add_self_loops
        self.aggr = "sum" if aggr == "add" else aggr

    def reset_parameters(self):
        for module in (self.local_nn, self.global_nn):
            if module is not None:
                _reset_module(module)

    def _operands(self, x, pos):
        """-> (x_src or None, pos_src, pos_dst), every host check that needs no device done"""
        pair = isinstance(pos, (tuple, list)) or isinstance(x, (tuple, list))
        if pair and self.add_self_loops:
            raise ValueError("PointNetConv: bipartite input (a pair pos or x) needs add_self_loops=False; pass "
                             "PointNetConv(..., add_self_loops=False)")
        for name, v in (("pos", pos), ("x", x)):
            if isinstance(v, (tuple, list)) and len(v) != 2:
                raise ValueError(f"PointNetConv: a pair {name} must have 2 entries, got {len(v)}")
        pos_src, pos_dst = pos if isinstance(pos, (tuple, list)) else (pos, pos)
        pos_src, pos_dst = _pointnet_pos(pos_src, "pos_src"), _pointnet_pos(pos_dst, "pos_dst")
        x_src, x_dst = x if isinstance(x, (tuple, list)) else (x, x)
        for name, v, rows in (("x_src", x_src, pos_src.size(0)), ("x_dst", x_dst, pos_dst.size(0))):
            if v is None:
                continue
            v = resolve(v)
            if not isinstance(v, Tensor):
                raise TypeError(f"PointNetConv: {name} must be a tensor or None, got {type(v).__name__}")
            if name == "x_src":
                x_src = v
                if v.dtype != torch.float32:
                    raise ValueError(f"PointNetConv: x must be float32, got {v.dtype}")
                if v.dim() != 2 or v.size(1) == 0:
                    raise ValueError(f"PointNetConv: x must be [Ns, F >= 1], got {tuple(v.shape)}")
            if v.dim() >= 1 and v.size(0) != rows:
                raise ValueError(f"PointNetConv: {name} has {v.size(0)} rows but its positions have {rows}")
        return x_src, pos_src, pos_dst

    def forward(self, x, pos, edge_index: Tensor) -> Tensor:
        """``conv(x, pos, edge_index)`` as PyG; ``x`` and ``pos`` may be pairs (class docstring)."""
        x_src, pos_src, pos_dst = self._operands(x, pos)
        if not isinstance(edge_index, Tensor):
            raise TypeError(f"PointNetConv: edge_index must be an int64 [2, E] tensor, got {type(edge_index).__name__} "
                            "(SparseTensor adjacencies are not supported)")
        for name, t in (("pos", pos_src), ("pos", pos_dst), ("x", x_src), ("edge_index", edge_index)):
            if t is not None:
                _require_cuda(t, name)
                if t.device != pos_src.device:
                    raise RuntimeError(f"pos is on {pos_src.device} but {name} is on {t.device}")
        ns, nd, loops = pos_src.size(0), pos_dst.size(0), self.add_self_loops
        g = ops.pointnet_graph(edge_index, ns, nd, loops) if max(ns, nd) else None
        z = ops.pointnet_pairs(g, x_src, pos_src, pos_dst, loops)
        m = resolve(self.local_nn(z)) if self.local_nn is not None else z
        if not isinstance(m, Tensor) or m.dim() != 2 or m.dtype != torch.float32 or m.size(0) != z.size(0) \
                or m.size(1) == 0:
            got = f"{tuple(m.shape)} {m.dtype}" if isinstance(m, Tensor) else type(m).__name__
            raise ValueError(f"PointNetConv: local_nn must return a float32 [E', C >= 1] tensor with E' = {z.size(0)} "
                             f"rows, got {got}")
        out = ops.pointnet_aggregate(g, m, self.aggr, nd, loops)
        return self.global_nn(out) if self.global_nn is not None else out

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(local_nn={self.local_nn}, global_nn={self.global_nn})"


# ``models/model.py:2`` imports ``knn`` from here (it never calls it): the device search of ``neighbors``
from ..neighbors import knn  # noqa: E402,F401
