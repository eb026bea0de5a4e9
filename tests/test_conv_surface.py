"""The surface of the eight conv classes of ``deformcontact_amd.nn``, pinned against literals: ordered ``state_dict``
keys with shapes, ``repr``, ``graph_flags()``, ``supports_fused_relu`` (its value, or its absence), and the exception
type and full text of every host-side ``edge_attr`` check of ``GATConv`` and ``GINEConv``.

One instance per class, with the options that change the surface set away from their defaults.  No GPU: the checks
under test run on the host, before anything asks for a device - where a call gets past them, the next error is the
one about ``x`` not being on a GPU, and that is asserted too.
"""
import pytest
import torch

from deformcontact_amd.nn import (GATConv, GATv2Conv, GCNConv, GINConv, GINEConv, SAGEConv, TAGConv, TransformerConv)

NO_LOOPS = dict(self_loops=False, normalize=False)

#: name -> (factory, ordered (key, shape) of state_dict(), repr, graph_flags(), supports_fused_relu or None: absent)
SURFACE = {
    "TAGConv": (
        lambda: TAGConv(5, 7, K=2, normalize=False),
        [("bias", (7,)), ("lins.0.weight", (7, 5)), ("lins.1.weight", (7, 5)), ("lins.2.weight", (7, 5))],
        "TAGConv(\n  5, 7, K=2\n  (lins): ModuleList(\n    (0-2): 3 x _Lin()\n  )\n)",
        dict(self_loops=False, normalize=False), True),
    "GCNConv": (
        lambda: GCNConv(5, 7),
        [("bias", (7,)), ("lin.weight", (7, 5))],
        "GCNConv(\n  (lin): _Lin()\n)",
        dict(self_loops=True, normalize=True), True),
    "GATConv": (
        lambda: GATConv(5, 4, heads=2, concat=False, edge_dim=3),
        [("att_src", (1, 2, 4)), ("att_dst", (1, 2, 4)), ("att_edge", (1, 2, 4)), ("bias", (4,)), ("lin.weight", (8, 5)),
         ("lin_edge.weight", (8, 3))],
        "GATConv(\n  5, 4, heads=2, concat=False, edge_dim=3, fill_value='mean'\n  (lin): _Lin()\n  (lin_edge): _Lin()\n)",
        dict(self_loops=True, normalize=False), True),
    "GATv2Conv": (
        lambda: GATv2Conv(5, 4, heads=2, concat=False, share_weights=True),
        [("att", (1, 2, 4)), ("bias", (4,)), ("lin_l.weight", (8, 5)), ("lin_l.bias", (8,)), ("lin_r.weight", (8, 5)),
         ("lin_r.bias", (8,))],
        "GATv2Conv(\n  5, 4, heads=2, concat=False, share_weights=True\n  (lin_l): _Lin()\n  (lin_r): _Lin()\n)",
        dict(self_loops=True, normalize=False), True),
    "TransformerConv": (
        lambda: TransformerConv(5, 4, heads=2, concat=False, beta=True),
        [("lin_key.weight", (8, 5)), ("lin_key.bias", (8,)), ("lin_query.weight", (8, 5)), ("lin_query.bias", (8,)),
         ("lin_value.weight", (8, 5)), ("lin_value.bias", (8,)), ("lin_skip.weight", (4, 5)), ("lin_skip.bias", (4,)),
         ("lin_beta.weight", (1, 12))],
        "TransformerConv(\n  5, 4, heads=2, concat=False, beta=True\n  (lin_key): _Lin()\n  (lin_query): _Lin()\n"
        "  (lin_value): _Lin()\n  (lin_skip): _Lin()\n  (lin_beta): _Lin()\n)",
        NO_LOOPS, True),
    "SAGEConv": (
        lambda: SAGEConv(5, 7, aggr="max", project=True),
        [("lin.weight", (5, 5)), ("lin.bias", (5,)), ("lin_l.weight", (7, 5)), ("lin_l.bias", (7,)),
         ("lin_r.weight", (7, 5))],
        "SAGEConv(\n  5, 7, aggr=max, project=True\n  (lin): _Lin()\n  (lin_l): _Lin()\n  (lin_r): _Lin()\n)",
        NO_LOOPS, True),
    "GINConv": (
        lambda: GINConv(torch.nn.Linear(5, 7), eps=0.25, train_eps=True),
        [("eps", (1,)), ("nn.weight", (7, 5)), ("nn.bias", (7,))],
        "GINConv(nn=Linear(in_features=5, out_features=7, bias=True))",
        NO_LOOPS, None),
    "GINEConv": (
        lambda: GINEConv(torch.nn.Linear(5, 7), train_eps=True, edge_dim=3),
        [("eps", (1,)), ("nn.weight", (7, 5)), ("nn.bias", (7,)), ("lin.weight", (5, 3)), ("lin.bias", (5,))],
        "GINEConv(nn=Linear(in_features=5, out_features=7, bias=True))",
        NO_LOOPS, None),
}


def observed(conv):
    return ([(k, tuple(v.shape)) for k, v in conv.state_dict().items()], repr(conv), conv.graph_flags(),
            getattr(conv, "supports_fused_relu", None))


@pytest.mark.parametrize("name", list(SURFACE))
def test_state_dict_repr_graph_flags_and_fused_relu_of_each_class(name):
    make, keys, text, flags, fused = SURFACE[name]
    conv = make()
    assert observed(conv) == (keys, text, flags, fused)
    assert hasattr(conv, "supports_fused_relu") == (fused is not None)
    assert [k for k, _ in conv.named_parameters()] == [k for k, _ in make().named_parameters()]


def test_train_eps_decides_whether_eps_is_a_parameter():
    for cls in (GINConv, GINEConv):
        assert [k for k, _ in cls(torch.nn.Linear(5, 7), train_eps=True).named_parameters()][0] == "eps"
        fixed = cls(torch.nn.Linear(5, 7))
        assert "eps" not in dict(fixed.named_parameters()) and list(fixed.state_dict())[0] == "eps"


E = 6
X = torch.zeros(4, 5)
EI = torch.zeros(2, E, dtype=torch.int64)
NOT_ON_GPU = (RuntimeError, "deformcontact_amd: x must live on a HIP device (got cpu). There is no CPU path in this package; "
                            "the CPU oracle under oracle/ is test-only.")


def gat(edge_dim=3):
    return GATConv(5, 4, heads=2, edge_dim=edge_dim)


def gine(edge_dim=3):
    return GINEConv(torch.nn.Linear(5, 7), edge_dim=edge_dim)


#: (layer, edge_attr, exception type, full message), every one with CPU tensors
EDGE_ATTR_ERRORS = {
    "gat_not_a_tensor": (gat, True, TypeError,
                         "edge_attr (the third positional argument, as in PyG) must be a tensor, got bool; pass relu= / "
                         "next_conv= by keyword"),
    "gat_not_a_tensor_without_edge_dim": (lambda: gat(None), 1.5, TypeError,
                                          "edge_attr (the third positional argument, as in PyG) must be a tensor, got "
                                          "float; pass relu= / next_conv= by keyword"),
    "gat_without_edge_dim": (lambda: gat(None), torch.zeros(E, 3, dtype=torch.float64), ValueError,
                             "edge_attr given to a GATConv built without edge_dim"),
    "gat_dtype": (gat, torch.zeros(E, 3, dtype=torch.float64), ValueError,
                  "edge_attr must be float32, got torch.float64"),
    "gat_width": (gat, torch.zeros(E, 2), ValueError, "edge_attr must be [E, 3] (edge_dim = 3), got (6, 2)"),
    "gat_one_dimension": (gat, torch.zeros(E), ValueError, "edge_attr must be [E, 3] (edge_dim = 3), got (6,)"),
    "gat_three_dimensions": (gat, torch.zeros(E, 3, 1), ValueError,
                             "edge_attr must be [E, 3] (edge_dim = 3), got (6, 3, 1)"),
    "gat_rows": (gat, torch.zeros(E + 1, 3), ValueError, "edge_attr has 7 rows but edge_index has 6 edges"),
    "gat_rows_at_width_one": (lambda: gat(1), torch.zeros(E - 1), ValueError,
                              "edge_attr has 5 rows but edge_index has 6 edges"),
    "gat_passes": (gat, torch.zeros(E, 3), *NOT_ON_GPU),
    "gat_passes_at_width_one": (lambda: gat(1), torch.zeros(E), *NOT_ON_GPU),
    "gat_passes_without_edge_attr": (gat, None, *NOT_ON_GPU),
    "gine_missing": (gine, None, ValueError, "GINEConv needs edge_attr: conv(x, edge_index, edge_attr)"),
    "gine_not_a_tensor": (gine, [1.0], TypeError,
                          "edge_attr (the third positional argument, as in PyG) must be a tensor, got list"),
    "gine_dtype": (gine, torch.zeros(E, 3, dtype=torch.int64), ValueError,
                   "edge_attr must be float32, got torch.int64"),
    "gine_one_dimension": (gine, torch.zeros(E), ValueError, "edge_attr must be [E, 3], got (6,)"),
    "gine_three_dimensions": (gine, torch.zeros(E, 3, 1), ValueError, "edge_attr must be [E, 3], got (6, 3, 1)"),
    "gine_width_with_edge_dim": (gine, torch.zeros(E, 2), ValueError,
                                 "edge_attr must be [E, 3] (edge_dim = 3), got (6, 2)"),
    "gine_width_without_edge_dim": (lambda: gine(None), torch.zeros(E, 3), ValueError,
                                    "Node and edge feature dimensionalities do not match. Consider setting the "
                                    "'edge_dim' attribute of 'GINEConv' (x has 5 columns, edge_attr 3)"),
    "gine_one_dimension_without_edge_dim": (lambda: gine(None), torch.zeros(E), ValueError,
                                            "edge_attr must be [E, 5], got (6,)"),
    "gine_rows": (gine, torch.zeros(E + 1, 3), ValueError, "edge_attr has 7 rows but edge_index has 6 edges"),
    "gine_inner_stride": (gine, torch.zeros(E, 6)[:, ::2], ValueError,
                          "edge_attr: innermost dimension must be contiguous"),
    "gine_passes": (gine, torch.zeros(E, 3), *NOT_ON_GPU),
    "gine_passes_at_width_one": (lambda: gine(1), torch.zeros(E), *NOT_ON_GPU),
    "gine_passes_without_edge_dim": (lambda: gine(None), torch.zeros(E, 5), *NOT_ON_GPU),
}


@pytest.mark.parametrize("case", list(EDGE_ATTR_ERRORS))
def test_edge_attr_checks_raise_the_same_type_and_text(case):
    make, edge_attr, kind, text = EDGE_ATTR_ERRORS[case]
    with pytest.raises(Exception) as err:
        make()(X, EI, edge_attr)
    assert (type(err.value), str(err.value)) == (kind, text)
