"""PyG-shaped conv operators backed by the gfx950 C-ABI library.

Same class names, constructor signature ``Conv(in_channels, out_channels)``, call
``conv(x, edge_index)`` and ``state_dict`` keys as ``torch_geometric.nn`` 2.5.2,
which is what ``/root/reference/models/model.py:2,39,45,49,71,77`` uses; and PyG's
graph construction (``knn``, ``knn_graph``, ``radius``, ``radius_graph``,
``/root/reference/utils/pointcloud_utils.py:7-13``) on the device search of
``deformcontact_amd.neighbors``, with the point-set sampling, transfer and per-graph pooling that go with it (``fps``,
``knn_interpolate``, ``global_add_pool`` / ``global_mean_pool`` / ``global_max_pool``: ``deformcontact_amd.pointops``).
"""
from ..neighbors import knn_graph, radius, radius_graph  # noqa: F401
from ..pointops import fps, global_add_pool, global_max_pool, global_mean_pool, knn_interpolate  # noqa: F401
from .conv import (ChebConv, DynamicEdgeConv, EdgeConv, GATConv, GATv2Conv, GCNConv, GINConv, GINEConv,  # noqa: F401
                   GMMConv, PointNetConv, SAGEConv, SplineConv, TAGConv, TransformerConv, knn)

__all__ = ["TAGConv", "GCNConv", "GATConv", "GATv2Conv", "TransformerConv", "knn", "knn_graph", "radius", "radius_graph",
           "DynamicEdgeConv", "SAGEConv", "PointNetConv", "global_add_pool", "global_mean_pool", "global_max_pool", "GINConv",
           "GINEConv", "EdgeConv", "fps", "knn_interpolate", "SplineConv", "GMMConv", "ChebConv"]
