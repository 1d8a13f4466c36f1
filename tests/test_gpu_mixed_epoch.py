"""GPU: host-free training epochs on mixed-topology data (BASELINE config C5: cigre14 + cigre14_reswitched in one data list; the reference's
loop is /root/reference/dss2_run.py:131-147 with the shuffling loader of :68-69).

* ``runner.EpochTrainer`` on ``MixedDataset.padded()``: an epoch of replays -- cursor collation of features, edge lists and per-slot edge
  counts, ``Topology.rebuild()``, forward, loss, backward, Adamax, loss accumulation -- equals the same steps run eagerly on the same
  padded batches bit for bit (parameters, optimizer state, per-epoch loss sums), as a launch plan and as a hipGraph, with a short last step;
* the padded layout computes what the unpadded batch computes (``MixedDataset.collate`` on the GPU, ``oracle.train_step``, the golden
  ``case_mpn_mixed.npz``) within the tolerances of tests/test_gpu_parity.py;
* ``rebuild()`` gives the structure oracle's CSR / ELL of the unpadded batch, entry for entry after mapping edge ids; no padding edge id
  anywhere; a slot count above e_max raises the error flag;
* the batch composition varies inside an epoch; the recorded step holds library launches only."""
import importlib

import numpy as np
import pytest
import torch

import dss2_topology_oracle as topo_oracle
from conftest import CASES, PKG_NAME, case_batch, case_grads, case_state_dict, golden, rel_err, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
TOL_OUT, TOL_LOSS, TOL_GRAD = 1e-5, 1e-5, 1e-4        # tests/test_gpu_parity.py
GRIDS = ["cigre14", "cigre14_reswitched"]
N_BUS, E_MAX = 15, 15


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


def _mixed(pkg, S, seed=0, violate=0.2):
    """A shuffled mixed data list of 2 * S samples (S per case) and its statistics."""
    full = pkg.synthetic.make_batch(GRIDS, 64, seed=seed)
    parts = [pkg.dataset.DeviceDataset.from_batch(pkg.synthetic.make_batch([g], S, seed=seed + 1 + k, stats=full["stats"], violate=violate), device=DEV)
             for k, g in enumerate(GRIDS)]
    mixed = pkg.dataset.MixedDataset(parts).shuffled(np.random.default_rng(seed))
    return mixed, tuple(s.to(DEV) for s in full["stats"])


def _opt_state(opt):
    out = []
    for g in opt.param_groups:
        out.append(g["_step"])
        for p in g["params"]:
            out += [opt.state[p]["exp_avg"], opt.state[p]["exp_inf"]]
    return out


def _eager_epoch(pkg, model, opt, padded, stats, B):
    """runner.train_epoch on the padded batches in store order, the step losses summed in fp64 like dss2_accum_scalar does."""
    acc = torch.zeros((), dtype=torch.float64, device=DEV)
    counts = []
    for data in pkg.dataset.DataLoader(padded, batch_size=B, shuffle=False):
        opt.zero_grad()
        x, ei, ea = data.x, data.edge_index, data.edge_attr
        out = model(x[:, :8], ei, ea[:, :6])
        loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=stats[0], x_std=stats[1], edge_mean=stats[2],
                                edge_std=stats[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
        loss.backward(pkg.data.unit_grad(loss))
        opt.step()
        acc += loss.detach().double()
        counts.append(int((data.e_count == E_MAX).sum()))
    return acc, counts


@pytest.mark.parametrize("mode", ["plan", "graph"])
@pytest.mark.parametrize("cls,cargs,S,B", [
    ("MPN", (8, 6, 2, 64, 3, 2, 0.0), 50, 32),             # 3 full batches + one of 4
    ("SkipPFN", (8, 6, 2, 32, 3, 2, 0.0, 2), 35, 16),      # the whole-stack kernels; 4 full batches + one of 6
    ("MPN", (8, 6, 2, 256, 8, 2, 0.0), 20, 16),            # the C5 model; 2 full batches + one of 8
])
def test_mixed_epochs_of_replays_equal_the_eager_epochs(pkg, mode, cls, cargs, S, B):
    mixed, stats = _mixed(pkg, S, seed=4)
    padded = mixed.padded()
    torch.manual_seed(1)
    m1 = getattr(pkg, cls)(*cargs).to(DEV)
    m2 = getattr(pkg, cls)(*cargs).to(DEV)
    m2.load_state_dict(m1.state_dict())
    o1 = pkg.optim.FusedAdamax(m1.parameters(), lr=3e-3, capturable=True)
    o2 = pkg.optim.FusedAdamax(m2.parameters(), lr=3e-3, capturable=True)
    before = [p.detach().clone() for p in m2.parameters()]
    tr = pkg.runner.EpochTrainer(m2, o2, stats, REG, padded, B, shuffle=False, mode=mode)      # (AttributeError / ValueError before this feature)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, m2.parameters()))
    assert float(o2.param_groups[0]["_step"]) == 0.0 and tr.cursor.tolist() == [0, 2 * S]
    assert sorted(tr.steps) == sorted({B, (2 * S) % B} - {0})
    if mode == "plan":      # one C call per step: a single segment of library launches (no copy, no torch kernel in between)
        assert all(len(rec[0].segments) == 1 and rec[0].n_launches > 0 for rec in tr.steps.values())
    o1.init_state()
    for epoch in range(3):
        want, _ = _eager_epoch(pkg, m1, o1, padded, stats, B)
        got = tr.train_epoch()
        torch.cuda.synchronize()
        assert got[1].item() == -(-2 * S // B)
        assert torch.equal(got[0], want), (epoch, got[0].item(), want.item())
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b), (a - b).abs().max().item()
    for a, b in zip(_opt_state(o1), _opt_state(o2)):
        assert torch.equal(a, b)
    assert float(o2.param_groups[0]["_step"]) == 3 * -(-2 * S // B)


def test_the_composition_varies_from_step_to_step_and_shuffles_over_the_union(pkg):
    mixed, stats = _mixed(pkg, 80, seed=2)
    padded = mixed.padded()
    m = pkg.MPN(8, 6, 2, 32, 2, 2, 0.0).to(DEV)
    o = pkg.optim.FusedAdamax(m.parameters(), lr=1e-3, capturable=True)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    B = 32
    tr = pkg.runner.EpochTrainer(m, o, stats, REG, padded, B, shuffle=True, generator=g)
    tr.train_epoch()
    first = tr.ids.clone()
    tr.train_epoch()
    torch.cuda.synchronize()
    assert sorted(first.tolist()) == list(range(160)) and sorted(tr.ids.tolist()) == list(range(160)) and not torch.equal(first, tr.ids)
    assert tr.acc.tolist()[1] == 5.0 and int(tr.cursor[0]) == 0
    # one epoch step by step: the gathered counts are the permuted samples' own, and the number of reswitched graphs per batch changes
    rec, _, _, _, ei, cnt, topo = tr.steps[B]
    tr.cursor.copy_(tr._cursor0)
    resw = []
    for k in range(5):
        rec.replay()
        torch.cuda.synchronize()
        want = padded.e_count[tr.ids[B * k:B * (k + 1)]]
        assert torch.equal(cnt, want) and int(topo.edge_total) == int(want.sum())
        assert torch.equal(ei, padded.collate(tr.ids[B * k:B * (k + 1)].contiguous()).edge_index)
        resw.append(int((cnt == E_MAX).sum()))
    assert len(set(resw)) > 1, resw


def test_unsupported_models_and_stores_are_refused(pkg):
    mixed, stats = _mixed(pkg, 8)
    gat = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER).to(DEV)
    o = pkg.optim.FusedAdamax(gat.parameters(), lr=1e-3, capturable=True)
    with pytest.raises(ValueError, match="MPN, SkipMPN, PFN and SkipPFN"):
        pkg.runner.EpochTrainer(gat, o, stats, REG, mixed.padded(), 4)
    m = pkg.MPN(8, 6, 2, 32, 2, 2, 0.0).to(DEV)
    o = pkg.optim.FusedAdamax(m.parameters(), lr=1e-3, capturable=True)
    with pytest.raises(ValueError, match="single-topology DeviceDataset"):
        pkg.runner.EpochTrainer(m, o, stats, REG, mixed, 4)


def _step(pkg, model, x, ei, ea, st, keep_out_grad=True):
    for p in model.parameters():
        p.grad = None
    out = model(x[:, :8], ei, ea[:, :6])
    grads = {}
    if keep_out_grad:
        out.register_hook(lambda g: grads.__setitem__("out", g.detach().clone()))
    loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3],
                            edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.detach().clone(), grads.get("out"), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("violate", [0.0, 0.3])
def test_padded_batch_computes_what_the_unpadded_batch_computes(pkg, oracle, violate):
    mixed, stats = _mixed(pkg, 40, seed=6, violate=violate)
    padded = mixed.padded()
    ids = mixed.ids[:48]
    torch.manual_seed(2)
    ref = oracle.MPN(8, 6, 2, 64, 3, 2, 0.0)
    if violate:
        # a freshly initialised model answers every bus with a voltage inside the 0.9 .. 1.1 band (x_std[0] is ~0.03): its voltage row
        # four times as large, it leaves the band, so that all three penalty terms -- not only angle and loading -- are compared
        with torch.no_grad():
            for lin in ref.convs[-1].lins:
                lin.weight[0] *= 4.0
            ref.convs[-1].bias[0] *= 4.0
    model = pkg.MPN(8, 6, 2, 64, 3, 2, 0.0)
    model.load_state_dict(ref.state_dict())
    model = model.to(DEV)
    pb = padded.collate(torch.from_numpy(ids).to(DEV))
    ub = mixed.collate(ids)
    assert pb.edge_index.shape[1] == 48 * E_MAX > ub.edge_index.shape[1] == int(pb.e_count.sum())
    out_p, loss_p, gout_p, gr_p = _step(pkg, model, pb.x, pb.edge_index, pb.edge_attr, stats)
    out_u, loss_u, gout_u, gr_u = _step(pkg, model, ub.x, ub.edge_index, ub.edge_attr, stats)
    if violate:      # the three penalty terms are part of the comparison
        sums = oracle.wls_partial_sums(ub.x[:, :8].cpu(), ub.edge_attr[:, :6].cpu(), out_u.cpu(), *(s.cpu() for s in stats), ub.edge_index.cpu(),
                                       ub.x[:, 8:].cpu(), ub.edge_attr[:, 6:].cpu(), REG)
        assert (sums[2:] > 0).all(), sums
    print("padded vs unpadded", rel_err(out_p, out_u), abs(loss_p.item() - loss_u.item()) / abs(loss_u.item()), rel_err(gout_p, gout_u),
          max(rel_err(gr_p[k], gr_u[k]) for k in gr_u))
    assert rel_err(out_p, out_u) < TOL_OUT
    assert abs(loss_p.item() - loss_u.item()) <= TOL_LOSS * abs(loss_u.item())
    assert rel_err(gout_p, gout_u) < TOL_GRAD
    for k in gr_u:
        assert rel_err(gr_p[k], gr_u[k]) < TOL_GRAD, k
    # the oracle on the unpadded batch (fp32 oracle, gates not pinned: a flipped ReLU gate moves a gradient row by ~1 / N_nodes,
    # tests/test_gpu_parity.py's un-pinned tolerance)
    b = {"x": ub.x.cpu(), "edge_index": ub.edge_index.cpu(), "edge_attr": ub.edge_attr.cpu()}
    out_r, loss_r = oracle.train_step(ref, b, tuple(s.cpu() for s in stats), REG)
    tol_unpinned = max(TOL_GRAD, 8.0 / out_p.shape[0])
    print("padded vs oracle", rel_err(out_p, out_r), abs(loss_p.item() - loss_r.item()) / abs(loss_r.item()),
          max(rel_err(gr_p[k], q.grad) for k, q in ref.named_parameters()))
    assert rel_err(out_p, out_r) < TOL_OUT      # (out_p: after the loss masked theta at the slack, like the oracle's output tensor)
    assert abs(loss_p.item() - loss_r.item()) <= TOL_LOSS * abs(loss_r.item())
    for k, q in ref.named_parameters():
        assert rel_err(gr_p[k], q.grad) < tol_unpinned, k


def test_padded_layout_of_the_golden_mixed_case(pkg, oracle):
    cls, args, _ = CASES["mpn_mixed"]
    g = golden("case_mpn_mixed.npz")
    model = getattr(pkg, cls)(*args)
    model.load_state_dict(case_state_dict(g), strict=True)
    model = model.to(DEV)
    b = case_batch(g, device=DEV)
    x, st = b["x"], b["stats"]
    G = x.shape[0] // N_BUS
    ei, ea, cnt = pkg.dataset.pad_batch(b["edge_index"], b["edge_attr"], N_BUS, G, e_max=E_MAX)
    assert ei.shape[1] == G * E_MAX > b["edge_index"].shape[1]
    ref = topo_oracle.TopologyOracle(t(g["edge_index"]), x.shape[0])
    hint = pkg.topology.TopologyHint(directed=ref.directed, nodes_per_graph=N_BUS, max_degree=max(ref.max_deg, ref.max_degT),
                                     max_edges_per_graph=E_MAX, edges_per_graph=E_MAX)
    topo = pkg.topology.register_topology(ei, x.shape[0], pkg.topology.Topology(ei, x.shape[0], hint=hint, edge_count=cnt))
    out, loss, _, grads = _step(pkg, model, x, ei, ea, st, keep_out_grad=False)
    assert topo.stats()["error"] == 0
    assert abs(loss.item() - float(g["loss"])) <= TOL_LOSS * abs(float(g["loss"]))
    assert rel_err(out, t(g["out_after_loss"])) < TOL_OUT
    want = case_grads(g)
    for k, v in grads.items():
        assert rel_err(v, want[k]) < TOL_GRAD, k


CSR_INT = ["rowptr", "col", "rowptrT", "colT", "inc_rowptr", "deg"]


def _check_structure(pkg, topo, ei_u, cnt, N):
    """The padded structure against the structure oracle of the UNPADDED batch: stored edge j of graph g is unpadded edge off[g] + j and
    padded slot g * E_MAX + j; directed ids map the same way in both halves."""
    ref = topo_oracle.TopologyOracle(ei_u, N, nrb=topo.nrb)      # (the oracle's tiles at the height the closed-form choice took)
    cnt = cnt.cpu().long()
    G, Eu, Ep = cnt.numel(), int(cnt.sum()), cnt.numel() * E_MAX
    off = torch.cumsum(cnt, 0) - cnt
    slot = torch.cat([g * E_MAX + torch.arange(int(c)) for g, c in enumerate(cnt)])           # unpadded edge id -> padded slot
    assert (topo.N, topo.E, topo.E2, topo.directed, int(topo.edge_total)) == (N, Ep, 2 * Ep, True, Eu) and ref.directed and ref.E == Eu
    n2 = 2 * Eu
    flip = torch.tensor(-2 ** 31, dtype=torch.int32)

    def map_ent(e):      # stored edge id | flip bit
        e = e.to(torch.int32)
        return (slot[(e & 0x7fffffff).long()].to(torch.int32)) | (e & flip)

    def map_dir(d):      # directed id: e, or E + e for the reverse
        d = d.long()
        return torch.where(d >= Eu, slot[(d - Eu).clamp(min=0)] + Ep, slot[d.clamp(max=Eu - 1)]).to(torch.int32)
    for f in CSR_INT:
        a, b = getattr(topo, f).cpu(), getattr(ref, f)
        a = a[:n2] if f in ("col", "colT") else a
        assert a.dtype == b.dtype and torch.equal(a, b), f
    for f in ("w", "wT"):
        assert torch.equal(getattr(topo, f).cpu()[:n2].view(torch.int32), getattr(ref, f).view(torch.int32)), f
    for f in ("ent", "entT"):
        assert torch.equal(getattr(topo, f).cpu()[:n2], map_ent(getattr(ref, f))), f
    for f in ("perm", "permT"):
        assert torch.equal(getattr(topo, f).cpu()[:n2], map_dir(getattr(ref, f))), f
    assert torch.equal(topo.inc_ent.cpu()[:n2], map_ent(ref.inc_ent))
    assert torch.equal(topo.efrom.cpu()[slot], ref.efrom) and torch.equal(topo.eto.cpu()[slot], ref.eto)
    assert torch.equal(topo.deg_pows.cpu().view(torch.int32), ref.deg_pows.view(torch.int32))
    # tiles and ELL slices (the primary tiling and the 32-row one of the weight gradient)
    assert (topo.nrb, topo.ntiles, topo.ell, topo.ellT) == (ref.nrb, ref.ntiles, ref.ell, ref.ellT)
    assert torch.equal(topo.tile_start.cpu(), ref.tile_start)
    for f in ("ell_tiles", "ellT_tiles"):
        assert torch.equal(getattr(topo, f).cpu(), getattr(ref, f)), f
    pad_slot = torch.ones(Ep, dtype=torch.bool)
    pad_slot[slot] = False
    for f in ("ell_ent_tiles", "ellT_ent_tiles"):
        a, b = getattr(topo, f).cpu(), getattr(ref, f).clone()
        live = b[..., 1] != -1
        b[..., 1][live] = map_ent(b[..., 1][live])
        assert torch.equal(a, b), f
        ids = (a[..., 1][a[..., 1] != -1] & 0x7fffffff).long()
        assert not pad_slot[ids].any(), f                                                    # no padding edge id anywhere
    for f in ("ent", "entT", "inc_ent"):
        assert not pad_slot[(getattr(topo, f).cpu()[:n2] & 0x7fffffff).long()].any(), f
    assert topo.stats()["error"] == 0


@pytest.mark.parametrize("which", ["all14", "all15", "mix"])
def test_rebuild_gives_the_structure_of_the_unpadded_batch(pkg, which):
    grids = {"all14": GRIDS[:1], "all15": GRIDS[1:], "mix": GRIDS}[which]
    G = 37
    b = pkg.synthetic.make_batch(grids, G, seed=7)
    ei_u, N = b["edge_index"], b["x"].shape[0]
    ei, _, cnt = pkg.dataset.pad_batch(ei_u, b["edge_attr"], N_BUS, G, e_max=E_MAX)
    assert set(cnt.tolist()) == {"all14": {14}, "all15": {15}, "mix": {14, 15}}[which]
    hint = pkg.topology.TopologyHint(directed=True, nodes_per_graph=N_BUS, max_degree=int(topo_oracle.TopologyOracle(ei_u, N).max_deg),
                                     max_edges_per_graph=E_MAX, edges_per_graph=E_MAX)
    # built on OTHER content first (every slot a branch of the reswitched grid), then rebuilt in place from the new device data
    other = pkg.synthetic.make_batch(GRIDS[1:], G, seed=1)["edge_index"].to(DEV)
    sei, scnt = other.clone(), torch.full((G,), E_MAX, dtype=torch.int32, device=DEV)
    topo = pkg.topology.Topology(sei, N, hint=hint, edge_count=scnt)
    topo.tiles_for(1), topo.tiles_for(2), topo.nrb
    sei.copy_(ei)
    scnt.copy_(cnt)
    topo.rebuild()
    _check_structure(pkg, topo, ei_u, cnt, N)
    alt = topo.tiles_for(1)
    ref1 = topo_oracle.TopologyOracle(ei_u, N, nrb=1)
    assert alt is not None and alt.ntiles == ref1.ntiles and torch.equal(alt.ell_tiles.cpu(), ref1.ell_tiles)
    # a slot count above e_max: flagged, nothing read out of bounds (the graph gets no edges)
    scnt[3] = E_MAX + 1
    topo.rebuild()
    with pytest.raises(ValueError, match="edge_count"):
        topo.stats()
    assert int(topo.edge_total) == int(cnt.sum()) - int(cnt[3])


def test_a_recorded_mixed_step_holds_library_launches_only(pkg):
    """PlannedStep's ``verify``: the recorded step (collation, rebuild, forward, loss, backward -- no optimizer, so that it is a function
    of its inputs) is replayed once and must reproduce loss and gradients bit for bit; a torch kernel or a copy the plan does not carry
    would not be replayed.  A tiling first asked for while the plan records is refused like every structure build outside a step."""
    mixed, stats = _mixed(pkg, 30, seed=3)
    padded = mixed.padded()
    B = 24
    m = pkg.MPN(8, 6, 2, 64, 3, 2, 0.0).to(DEV)
    params = list(m.parameters())
    sx = torch.empty(B * N_BUS, 11, device=DEV)
    sea = torch.empty(B * E_MAX, 13, device=DEV)
    ei = torch.empty(2, B * E_MAX, dtype=torch.int64, device=DEV)
    cnt = torch.empty(B, dtype=torch.int32, device=DEV)
    descs = padded.collate_descs(sx, sea, edge_index=ei, e_count=cnt)
    cursor = torch.tensor([24, 60], dtype=torch.int64, device=DEV)
    padded.collate_into(descs, padded.ids, B, cursor=cursor, advance=False)
    topo = padded.padded_topology(ei, cnt)

    def step():
        padded.collate_into(descs, padded.ids, B, cursor=cursor, advance=False)
        topo.rebuild()
        for p in params:
            p.grad = None
        out = m(sx[:, :8], ei, sea[:, :6])
        loss = pkg.gsp_wls_edge(input=sx[:, :8], edge_input=sea[:, :6], output=out, x_mean=stats[0], x_std=stats[1], edge_mean=stats[2],
                                edge_std=stats[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=sx[:, 8:], edge_param=sea[:, 6:])
        loss.backward(pkg.data.unit_grad(loss))
        return loss
    holder = {}

    def step_keep():
        holder["loss"] = step()
        return holder["loss"]
    rec = pkg.graphs.PlannedStep(step_keep, verify=lambda: [holder["loss"]] + [p.grad for p in params])
    assert len(rec.segments) == 1 and rec.n_launches > 0
    # the replayed structure follows the device data: other samples under the cursor, same plan
    cursor[0] = 0
    rec.replay()
    torch.cuda.synchronize()
    assert torch.equal(cnt, padded.e_count[padded.ids[:B]]) and int(topo.edge_total) == int(cnt.sum())
    L = pkg._lib.lib()
    import ctypes as C
    h = C.c_void_p()
    assert L.dss2_plan_begin(C.byref(h)) == 0
    try:
        with pytest.raises(RuntimeError, match="not available while a launch plan records"):
            topo.tiles_for(6)
    finally:
        assert L.dss2_plan_end(h) == 0
        L.dss2_plan_destroy(h)
