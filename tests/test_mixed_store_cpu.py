"""CPU: the padded layout of mixed-topology data (dataset.pad_batch, dataset.PaddedMixedDataset, MixedDataset.padded()).

* layout: every sample gets e_max edge slots, its branches first, then padding edges (from = to = the graph's first bus, every
  attribute 0 except imax_or_sn = 1); the per-sample counts; parts that disagree on the first-edge rule or the bus count are refused;
* the padding-edge argument, with the oracle's ``wls_partial_sums`` / ``loss_from_sums``: padding edges in the middle of a batch leave
  the five loss sums unchanged up to summation order, and -- divided by the REAL edge count -- the loss and d loss / d output bit for bit.
"""
import numpy as np
import pytest
import torch

from conftest import load_pkg

N_BUS = 15
GRIDS = ["cigre14", "cigre14_reswitched"]


def _part(pkg, grid, S, seed, stats=None, violate=0.0):
    """dataset.DeviceDataset.from_batch without the device requirement (the store itself is plain tensors)."""
    b = pkg.synthetic.make_batch([grid], S, seed=seed, stats=stats, violate=violate)
    n, e = b["x"].shape[0] // S, b["edge_attr"].shape[0] // S
    ei = b["edge_index"].view(2, S, e).permute(1, 0, 2) - (torch.arange(S) * n).view(S, 1, 1)
    return pkg.dataset.DeviceDataset(b["x"].view(S, n, -1).contiguous(), b["edge_attr"].view(S, e, -1).contiguous(),
                                     b["y"].view(S, n, -1).contiguous(), ei.contiguous())


def _parts(pkg, S=(5, 7)):
    full = pkg.synthetic.make_batch(GRIDS, 16, seed=0)
    return [_part(pkg, g, s, seed=1 + k, stats=full["stats"]) for k, (g, s) in enumerate(zip(GRIDS, S))]


def test_padded_store_layout_counts_and_padding_rows():
    pkg = load_pkg()
    parts = _parts(pkg)
    assert [p.e for p in parts] == [14, 15]
    mixed = pkg.dataset.MixedDataset(parts).shuffled(np.random.default_rng(3))
    st = mixed.padded()
    assert isinstance(st, pkg.dataset.PaddedMixedDataset) and isinstance(st, pkg.dataset.DeviceDataset)
    assert (st.S, st.n, st.e, len(st)) == (12, N_BUS, 15, 12) and not st.shared_topology
    assert tuple(st.x.shape) == (12, N_BUS, 11) and tuple(st.edge_attr.shape) == (12, 15, 13) and tuple(st.edge_index.shape) == (12, 2, 15)
    assert st.e_count.dtype == torch.int32 and st.e_count.tolist() == [14] * 5 + [15] * 7
    assert st.ids.tolist() == mixed.ids.tolist()                      # the mixed list's order (global sample numbers)
    # the real rows are the parts' rows; the one padding row of every 14-branch sample is the branch that carries nothing
    assert torch.equal(st.edge_attr[:5, :14], parts[0].edge_attr) and torch.equal(st.edge_attr[5:], parts[1].edge_attr)
    assert torch.equal(st.edge_index[:5, :, :14], parts[0].edge_index.expand(5, -1, -1)) and torch.equal(st.x[5:], parts[1].x)
    pad = st.edge_attr[:5, 14]
    assert torch.equal(pad, torch.tensor([0.0] * 12 + [1.0]).expand(5, -1))
    assert (st.edge_index[:5, :, 14] == 0).all()                      # from = to = the graph's first bus
    # degrees come from the parts, not from the padding self loops; one directedness for the whole store
    assert st.max_degree_doubled == max(p.max_degree_doubled for p in parts) and st.directed is True
    h = st.hint()
    assert (h.nodes_per_graph, h.edges_per_graph, h.max_edges_per_graph, h.directed) == (N_BUS, 15, 15, True)
    # slices keep the class (train / test splits); a single sample comes back without its padding
    assert isinstance(st[0:4], pkg.dataset.PaddedMixedDataset) and len(st[0:4]) == 4
    s0 = int(st.ids[0])
    one = st[0]
    assert one.edge_attr.shape[0] == int(st.e_count[s0]) == one.edge_index.shape[1]


def test_padded_store_refuses_what_one_recorded_step_cannot_serve():
    pkg = load_pkg()
    parts = _parts(pkg)
    # a part whose samples store both directions of their first edge: MPN.is_directed would differ with the batch's first sample
    und = parts[1]
    ei = und.edge_index.clone()
    ei[:, :, 1] = ei[:, :, 0].flip(1)
    both = pkg.dataset.DeviceDataset(und.x, und.edge_attr, und.y, ei)
    assert both.directed is False
    with pytest.raises(ValueError, match="first-edge rule"):
        pkg.dataset.MixedDataset([parts[0], both]).padded()
    # different bus counts: no padded store (and EpochTrainer keeps refusing the MixedDataset itself)
    ober = _part(pkg, "ober_sub", 2, seed=5)
    with pytest.raises(ValueError, match="different bus counts"):
        pkg.dataset.MixedDataset([parts[0], ober]).padded()


def test_pad_batch_layout():
    pkg = load_pkg()
    b = pkg.synthetic.make_batch(GRIDS, 6, seed=2)
    ei, ea = b["edge_index"], b["edge_attr"]
    eip, eap, cnt = pkg.dataset.pad_batch(ei, ea, N_BUS, 6)
    assert set(cnt.tolist()) == {14, 15} and int(cnt.sum()) == ei.shape[1]
    assert tuple(eip.shape) == (2, 90) and tuple(eap.shape) == (90, 13)
    k = 0
    for g, c in enumerate(cnt.tolist()):
        assert torch.equal(eip[:, 15 * g:15 * g + c], ei[:, k:k + c]) and torch.equal(eap[15 * g:15 * g + c], ea[k:k + c])
        assert (eip[:, 15 * g + c:15 * (g + 1)] == g * N_BUS).all()
        assert torch.equal(eap[15 * g + c:15 * (g + 1)], torch.tensor([0.0] * 12 + [1.0]).expand(15 - c, -1))
        k += c
    with pytest.raises(ValueError, match="does not fit"):
        pkg.dataset.pad_batch(ei, ea, N_BUS, 6, e_max=14)


def _loss_case(pkg, seed):
    b = pkg.synthetic.make_batch(GRIDS, 8, seed=seed, violate=0.3)
    x, ei, ea, st, y = b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["y"]
    out0 = torch.stack([(y[:, 0] - st[0][0]) / st[1][0], y[:, 1]], 1)       # the labels as the model's (normalised) output
    return x, ei, ea, st, out0


def test_padding_edges_leave_the_loss_and_its_gradient_unchanged(oracle):
    """8 mixed graphs, violate=0.3 (synthetic.make_batch's default seed: three 15-branch and five 14-branch graphs), the labels as the
    model output, so that all three penalty terms are non-zero.  The padded layout puts a padding edge behind every 14-branch graph:
    5 of them, in the middle of the batch.  fp32, like the kernels.  The sums may move by summation order only (torch sums a vector of
    another length in other chunks): the padded list adds EXACT zeros, so the bound is the reordering error of an fp32 sum of
    E <= 120 non-negative terms, E * 2^-24 relative to the sum itself; 1e-5 is a generous statement of that.  The loss and its gradient
    come out bit for bit when the divisor is the real edge count.  (The exact, order-free form of the claim -- per-edge quantities --
    is the next test; an fp32 reordering of a sum CAN reach the last bits of the loss on other batches, e.g. seeds 2 and 9 here.)"""
    pkg = load_pkg()
    x, ei, ea, st, out0 = _loss_case(pkg, 0)
    eip, eap, cnt = pkg.dataset.pad_batch(ei, ea, N_BUS, 8)
    assert eip.shape[1] - ei.shape[1] == 5 and 14 in cnt[:-1].tolist()      # (a padding edge in front of another graph's branches: mid-batch)
    reg = oracle.DEFAULT_REG_COEFS

    def run(ei_, ea_, n_edges):
        o_leaf = out0.clone().requires_grad_(True)
        o = torch.cat([o_leaf[:, :1], o_leaf[:, 1:] * (1.0 - x[:, 9:10])], 1)
        sums = oracle.wls_partial_sums(x[:, :8], ea_[:, :6], o, st[0], st[1], st[2], st[3], ei_, x[:, 8:], ea_[:, 6:], reg)
        loss = oracle.loss_from_sums(sums, x.shape[0], n_edges, reg["lam_reg"])
        loss.backward()
        return sums.detach(), loss.detach(), o_leaf.grad

    s0, l0, g0 = run(ei, ea, ei.shape[1])
    s1, l1, g1 = run(eip, eap, ei.shape[1])                # padded list, REAL edge count
    print("sums", s0.tolist(), s1.tolist(), "loss", l0.item(), l1.item(), "max |dgrad|", (g1 - g0).abs().max().item())
    assert (s0[2:] > 0).all(), s0                          # the three penalty terms are active
    assert torch.allclose(s1, s0, rtol=1e-5, atol=0), (s0, s1)
    assert torch.equal(l1, l0), (l0.item(), l1.item())
    assert torch.isfinite(g1).all() and torch.equal(g1, g0)
    # ... and the divisor matters: with the padded count the loss is another number
    _, l2, _ = run(eip, eap, eip.shape[1])
    assert not torch.equal(l2, l0)


@pytest.mark.parametrize("seed", [0, 2, 9, 11])
def test_a_padding_edge_carries_exactly_nothing(oracle, seed):
    """Order-free: per stored edge, the padded list's get_pflow quantities are the batch's own at the real slots, bit for bit, and at
    the padding slots the four flows and both currents are exactly 0 and the loadings exactly 0 (0 / imax with imax = 1: finite) --
    so every term a padding edge adds to a loss sum, a bus injection or a gradient is an exact zero."""
    pkg = load_pkg()
    x, ei, ea, st, out0 = _loss_case(pkg, seed)
    eip, eap, cnt = pkg.dataset.pad_batch(ei, ea, N_BUS, 8)
    yv = torch.cat([out0[:, :1] * st[1][:1] + st[0][:1], out0[:, 1:] * (1.0 - x[:, 9:10])], 1)
    real = torch.zeros(eip.shape[1], dtype=torch.bool)
    for g, c in enumerate(cnt.tolist()):
        real[15 * g:15 * g + c] = True
    q0 = torch.stack(oracle.get_pflow(yv, ei, x[:, 8:], ea[:, 6:]), 1)
    q1 = torch.stack(oracle.get_pflow(yv, eip, x[:, 8:], eap[:, 6:]), 1)
    assert torch.equal(q1[real], q0)
    assert (~real).sum() == eip.shape[1] - ei.shape[1] > 0 and (q1[~real] == 0).all()
    # no measurement on a padding edge (z = 1/var = 0: masked out of the edge WLS term), no angle difference (from = to)
    assert (eap[~real][:, :6] == 0).all() and (eip[0, ~real] == eip[1, ~real]).all()
