"""The reference's import surface binds to this package through the torch_geometric alias: the names its
models/model.py imports (``from torch_geometric.nn import GATConv, GCNConv, TAGConv, knn``) resolve to this package's
modules, the model has exactly the reference GraphNet's state_dict layout (keys in order, shapes; stored in
tests/golden/reference_state_dict.npz by oracle/make_golden.py), a checkpoint of that layout loads, and a forward on
alias-built batches reaches our ops."""
import sys

import pytest
import torch

from tests.helpers import load_golden


def test_reference_graphnet_binds_to_this_package():
    import deformcontact_amd as dc
    from deformcontact_amd.graphnet import EVERYDAY_NETWORK, load_model as our_load
    z = load_golden("reference_state_dict.npz")
    ref_layout = [(str(k), tuple(int(d) for d in s[:n])) for k, n, s in zip(z["keys"], z["ndim"], z["shapes"])]
    dc.install_as_torch_geometric()
    try:
        from torch_geometric.nn import GATConv, GCNConv, TAGConv, knn
        assert (TAGConv, GCNConv, GATConv, knn) == (dc.nn.TAGConv, dc.nn.GCNConv, dc.nn.GATConv, dc.nn.knn)
        ours = our_load(EVERYDAY_NETWORK)
        assert all(isinstance(c, dc.nn.TAGConv) for c in list(ours.conv_layers_resting) + list(ours.conv_layers_rigid))
        sd_ours = ours.state_dict()
        assert [k for k, _ in ref_layout] == list(sd_ours)
        assert all(tuple(sd_ours[k].shape) == s for k, s in ref_layout)
        gen = torch.Generator().manual_seed(0)
        sd_ref = {k: torch.randn(s, generator=gen) for k, s in ref_layout}
        ours.load_state_dict(sd_ref)                     # reference checkpoint loads
        assert all(torch.equal(v, sd_ref[k]) for k, v in ours.state_dict().items())
        # forward reaches our conv (which refuses CPU tensors - no fallback)
        from torch_geometric.data import Batch, Data
        g = Data(x=torch.zeros(4, 21), edge_index=torch.tensor([[0, 1], [1, 2]]), pos=torch.zeros(4, 3))
        r = Data(x=torch.zeros(3, 25), edge_index=torch.tensor([[0, 1], [1, 2]]), pos=torch.zeros(3, 3))
        with pytest.raises(RuntimeError, match="HIP device"):
            ours(Batch.from_data_list([g]), Batch.from_data_list([r]))
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] == "torch_geometric"]:
            sys.modules.pop(k, None)
