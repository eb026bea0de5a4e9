"""CPU: pin the oracle -- against the fixtures generated from the reference's own
wiring, against the independent float64 closed forms, and against the scalar C hop."""
import numpy as np
import pytest
import torch

from oracle import closed_form, hop_c, pyg_ref
from oracle.weights import fill_state_dict_, hashed_uniform
from tests.helpers import golden_graphs, load_golden, random_multigraph, rel_err

TOL = 1e-5   # north_star: 1e-5 rel fp32


def _net(backbone, hidden):
    from deformcontact_amd.graphnet import EVERYDAY_NETWORK, load_model
    cfg = dict(EVERYDAY_NETWORK, hidden_dim=hidden, backbone=backbone)
    m = load_model(cfg, conv_module=pyg_ref)     # product wiring + ORACLE convs (CPU)
    fill_state_dict_(m)
    return m


@pytest.mark.parametrize("backbone,fname", [("TAGConv", "graphnet_tag_h32.npz"),
                                             ("GCNConv", "graphnet_gcn_h32.npz"),
                                             ("GATConv", "graphnet_gat_h32.npz")])
def test_config0_oracle_reproduces_reference_run(backbone, fname):
    """Fixtures came from /root/reference/models/model.py run end to end; the oracle convs
    inside the restated wiring must give the same activations, loss and gradients."""
    z = load_golden(fname)
    torch.set_num_threads(1)
    m = _net(backbone, int(z["hidden"])).train()
    rest, rig = golden_graphs(z)
    x_rest, x_rig = m.encode(rest, rig)
    assert rel_err(x_rest.detach(), z["conv_resting_1"].clip(min=0)) < TOL
    assert rel_err(x_rig.detach(), z["conv_rigid_1"].clip(min=0)) < TOL
    pred = m(rest, rig)
    assert rel_err(pred.pos.detach(), z["pred_pos"]) < TOL
    from deformcontact_amd.graphnet import gradient_consistency_loss
    pred.pos = pred.pos - rest.pos
    tgt = rest.clone()
    tgt.pos = torch.from_numpy(z["def_pos"]) - rest.pos
    l1 = torch.nn.functional.l1_loss(pred.pos, tgt.pos)
    gcl = gradient_consistency_loss(pred, tgt)
    assert abs(float(l1) - float(z["loss_l1"])) <= TOL * abs(float(z["loss_l1"]))
    assert abs(float(gcl) - float(z["loss_gcl"])) <= TOL * abs(float(z["loss_gcl"]))
    (l1 + gcl).backward()
    truth64 = _float64_grads(backbone, z) if backbone == "GATConv" else None
    for name, p in m.named_parameters():
        truth = truth64[name] if name.endswith("att_dst") else None
        scale = np.abs(z["grad." + name.replace("att_dst", "att_src")]).max()
        if truth is not None and np.abs(truth).max() < 1e-9 * scale:
            # softmax is invariant to a per-destination shift: where d loss / d att_dst is zero in float64, both fp32
            # gradients are rounding noise (~1e-13) whose bits depend on the CPU's vector kernels; as in
            # test_gpu_parity, compared against float64 on the scale of the sibling att_src gradient
            e_h = np.abs(p.grad.numpy() - truth).max()
            e_o = np.abs(z["grad." + name] - truth).max()
            assert e_h <= max(2 * e_o, 2e-5 * scale), (name, e_h, e_o, scale)
            continue
        assert rel_err(p.grad, z["grad." + name]) < 2e-5, name


def _float64_grads(backbone, z):
    """The parameter gradients of the fixture's step, oracle convs in float64."""
    from deformcontact_amd.graphnet import gradient_consistency_loss
    m = _net(backbone, int(z["hidden"])).double().train()
    rest, rig = golden_graphs(z)
    for b in (rest, rig):
        b.x, b.pos = b.x.double(), b.pos.double()
    pred = m(rest, rig)
    pred.pos = pred.pos - rest.pos
    tgt = rest.clone()
    tgt.pos = torch.from_numpy(z["def_pos"]).double() - rest.pos
    (torch.nn.functional.l1_loss(pred.pos, tgt.pos) + gradient_consistency_loss(pred, tgt)).backward()
    return {k: v.grad.numpy() for k, v in m.named_parameters()}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_vs_closed_form_tag(seed):
    n, e, fi, fo = 40, 260, 7, 5
    ei = random_multigraph(n, e, seed)
    x = hashed_uniform((n, fi), 3 + seed, 2.0)
    conv = pyg_ref.TAGConv(fi, fo)
    fill_state_dict_(conv, salt0=seed)
    out = conv(torch.from_numpy(x), torch.from_numpy(ei)).detach().numpy()
    ref = closed_form.tagconv(x, ei, [l.weight.detach().numpy() for l in conv.lins],
                              conv.bias.detach().numpy())
    assert rel_err(out, ref) < 2e-6


@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_vs_closed_form_gcn_gat(seed):
    n, e, fi, fo = 33, 200, 6, 8
    ei = random_multigraph(n, e, seed)
    x = hashed_uniform((n, fi), 9 + seed, 2.0)
    xt, et = torch.from_numpy(x), torch.from_numpy(ei)
    gcn = pyg_ref.GCNConv(fi, fo)
    fill_state_dict_(gcn, salt0=seed)
    ref = closed_form.gcnconv(x, ei, gcn.lin.weight.detach().numpy(), gcn.bias.detach().numpy())
    assert rel_err(gcn(xt, et).detach().numpy(), ref) < 2e-6
    gat = pyg_ref.GATConv(fi, fo)
    fill_state_dict_(gat, salt0=seed)
    ref = closed_form.gatconv(x, ei, gat.lin.weight.detach().numpy(), gat.att_src.detach().numpy(),
                              gat.att_dst.detach().numpy(), gat.bias.detach().numpy())
    assert rel_err(gat(xt, et).detach().numpy(), ref) < 2e-6


def test_c_hop_matches_torch_ops():
    n, e, f = 57, 400, 21
    ei = random_multigraph(n, e, 5)
    x = hashed_uniform((n, f), 21, 2.0)
    _, w = pyg_ref.gcn_norm(torch.from_numpy(ei), n, add_loops=False)
    wc = hop_c.gcn_norm(ei, n)
    assert rel_err(wc, w.numpy()) < 1e-6
    y = pyg_ref.propagate_sum(torch.from_numpy(ei), torch.from_numpy(x), w).numpy()
    yc = hop_c.hop(ei, w.numpy(), x)
    assert rel_err(yc, y) < 1e-6


def test_c_csr_matches_stable_argsort_and_golden():
    z = load_golden("mesh_graph_csr.npz")
    ei = z["batch_edge_index"]
    n = z["batch_x"].shape[0]
    ptr, other, perm = hop_c.csr_build(ei, n, key_row=1)
    assert np.array_equal(ptr, z["rowptr"]) and np.array_equal(perm, z["perm"])
    assert np.array_equal(other, z["src_sorted"])
    ptr, other, perm = hop_c.csr_build(ei, n, key_row=0)
    assert np.array_equal(ptr, z["colptr"]) and np.array_equal(perm, z["perm_t"])
    assert np.array_equal(other, z["dst_sorted"])
    with pytest.raises(ValueError):
        hop_c.csr_build(np.array([[0], [n]], dtype=np.int64), n)


def test_oracle_batch_matches_golden():
    z = load_golden("mesh_graph_csr.npz")
    g1 = pyg_ref.Data(x=torch.from_numpy(z["x1"]), edge_index=torch.from_numpy(z["ei1"]))
    g2 = pyg_ref.Data(x=torch.from_numpy(z["x2"]), edge_index=torch.from_numpy(z["ei2"]))
    b = pyg_ref.Batch.from_data_list([g1, g2, g1])
    assert np.array_equal(b.edge_index.numpy(), z["batch_edge_index"])
    assert np.array_equal(b.ptr.numpy(), z["batch_ptr"])
    assert np.array_equal(b.batch.numpy(), z["batch_vec"])
    assert np.array_equal(b[1].edge_index.numpy(), z["ei2"])


def test_c_csr_property_random_graphs():
    """hypothesis: the C counting sort equals numpy's stable argsort on arbitrary multigraphs
    (duplicates, self loops, isolated nodes, empty edge lists)."""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=60, deadline=None)
    @given(st.integers(1, 40).flatmap(lambda n: st.tuples(
        st.just(n), st.lists(st.tuples(st.integers(0, n - 1), st.integers(0, n - 1)), max_size=200))))
    def check(args):
        n, edges = args
        ei = np.array(edges, dtype=np.int64).reshape(-1, 2).T if edges else np.zeros((2, 0), np.int64)
        ei = np.ascontiguousarray(ei)
        for key_row in (0, 1):
            ptr, other, perm = hop_c.csr_build(ei, n, key_row)
            order = np.argsort(ei[key_row], kind="stable")
            assert np.array_equal(perm, order.astype(np.int32))
            assert np.array_equal(other, ei[1 - key_row][order].astype(np.int32))
            assert np.array_equal(ptr[1:], np.cumsum(np.bincount(ei[key_row], minlength=n)))
        if ei.shape[1]:
            w = hop_c.gcn_norm(ei, n)
            deg = np.bincount(ei[1], minlength=n).astype(np.float64)
            dis = np.zeros_like(deg)
            dis[deg > 0] = deg[deg > 0] ** -0.5
            assert np.allclose(w, dis[ei[0]] * dis[ei[1]], rtol=1e-6)

    check()


def test_bf16_hop_oracle_against_float64_and_fp32_oracle():
    """ref_hop_bf16: the fp32 result equals ref_hop over the widened rows bit
    for bit; the bf16 result is that sum rounded once to nearest even; both agree with float64."""
    n, e, f = 120, 900, 40
    ei = random_multigraph(n, e, 77)
    w = hop_c.gcn_norm(ei, n)
    xb = torch.from_numpy(hashed_uniform((n, f), 5, 2.0)).bfloat16()
    bits = xb.view(torch.int16).numpy().view(np.uint16)
    wide = xb.float().numpy()
    y32 = hop_c.hop_bf16(ei, w, bits, True)
    assert np.array_equal(y32, hop_c.hop(ei, w, wide))
    y16 = hop_c.hop_bf16(ei, w, bits, False)
    exp16 = torch.from_numpy(y32).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(y16, exp16)
    dense = np.zeros((n, n))
    np.add.at(dense, (ei[1], ei[0]), w.astype(np.float64))
    assert rel_err(y32, dense @ wide.astype(np.float64)) < 1e-6
    ones = hop_c.hop_bf16(ei, None, bits, True)                  # w == NULL: weight 1
    assert np.array_equal(ones, hop_c.hop(ei, np.ones(e, np.float32), wide))
