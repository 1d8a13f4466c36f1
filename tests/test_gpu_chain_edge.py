"""GPU: the edge MLP's first Linear as a phase of the 64-row f16x3 chains (dss2_chain_edge, csrc/dss2_gemm_chain_sp.hip) against the two
edge launches of their own (flags.CHAIN_EDGE off), in one process.  The forward chain computes S with the edge kernel's arithmetic
(dss2_edge16_tile.hpp), so S, every activation, the output, the loss and every parameter gradient but dW1 / db1 are the same bits;
dW1 / db1 are now one slab per tile instead of one per workgroup of the edge backward -- another fixed summation order."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C2 = (8, 6, 2, 128, 4, 2, 0.0)
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
EDGE_W = ("edge_aggr.edge_aggr.0.weight", "edge_aggr.edge_aggr.0.bias")


def _batch(pkg, grids, B, seed=0, poison=False):
    b = pkg.synthetic.make_batch(grids, B, seed=seed, violate=0.3)
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    if poison:      # non-finite inputs: a NaN and an Inf node feature, an Inf edge feature
        x = x.clone()
        ea = ea.clone()
        x[3, 1] = float("nan")
        x[70, 4] = float("inf")
        ea[11, 2] = float("-inf")
    return x, ei, ea, tuple(s.to(DEV) for s in b["stats"])


def _step(pkg, model, data, on):
    x, ei, ea, st = data
    saved = pkg.flags.CHAIN_EDGE
    pkg.flags.CHAIN_EDGE = on
    try:
        for p in model.parameters():
            p.grad = None
        topo = pkg.topology.get_topology(ei, x.shape[0])
        with torch.no_grad():      # S and the block's output through the functional forward
            out_f, saved_t, _ = pkg.networks._mpn_forward(model, topo, x[:, :8], ea[:, :6], model._params())
        S = saved_t[2].clone()
        out = model(x[:, :8], ei, ea[:, :6])
        loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3],
                                edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
        loss.backward(pkg.data.unit_grad(loss))
        torch.cuda.synchronize()
        return dict(S=S, out_f=out_f.clone(), out=out.detach().clone(), loss=loss.detach().clone(),
                    grads={n: p.grad.clone() for n, p in model.named_parameters()})
    finally:
        pkg.flags.CHAIN_EDGE = saved


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _model(pkg, seed=0):
    torch.manual_seed(seed)
    model = pkg.MPN(*C2).to(DEV)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model


def _check(pkg, model, data, finite=True):
    x, ei = data[0], data[1]
    topo = pkg.topology.get_topology(ei, x.shape[0])
    # (64-row tiles; a batch of a few graphs gets a shorter tiling, on which the edge launches stay and both runs are the same route)
    assert topo.nrb != 2 or (pkg.networks.chain_edge_supported(topo, 3, 128, False) and pkg.networks.chain_edge_supported(topo, 3, 128, True))
    ref = _step(pkg, model, data, False)
    got = _step(pkg, model, data, True)
    again = _step(pkg, model, data, True)
    for k in ("S", "out_f", "out", "loss"):
        assert _same(got[k], ref[k]), k
        assert _same(again[k], got[k]), k
    for n, g in got["grads"].items():
        assert _same(again["grads"][n], g), n        # reproducible run to run
        if n in EDGE_W:
            if finite:
                assert rel_err(g, ref["grads"][n]) < 1e-6, (n, rel_err(g, ref["grads"][n]))
            else:
                assert torch.equal(g.isnan(), ref["grads"][n].isnan()), n
        else:
            assert _same(g, ref["grads"][n]), n
    return got


@pytest.mark.parametrize("B", [4096, 1, 5, 4097])
def test_fused_edge_phases_equal_the_edge_launches(pkg, B):
    """C2 (B = 4096: four graphs = 60 of a tile's 64 rows), a last tile of one graph (4097), and batches of one / five graphs."""
    _check(pkg, _model(pkg), _batch(pkg, ["cigre14"], B, seed=B))


def test_fused_edge_phases_mixed_topologies(pkg):
    """C5's mix of cigre14 and cigre14_reswitched graphs in one batch (different ELL rows per graph), on the C2 model."""
    _check(pkg, _model(pkg, 1), _batch(pkg, ["cigre14", "cigre14_reswitched"], 1000, seed=5))


def test_fused_edge_phases_non_finite_inputs(pkg):
    """NaN / Inf in the inputs propagate through the fused phases exactly as through the edge launches."""
    got = _check(pkg, _model(pkg, 2), _batch(pkg, ["cigre14"], 300, seed=6, poison=True), finite=False)
    assert not bool(torch.isfinite(got["S"]).all())


def test_fused_edge_gradients_against_the_oracle(pkg, oracle):
    """dW1 / db1 of the fused step against the oracle's training step (the parity suite's un-pinned tolerance)."""
    torch.manual_seed(0)
    b = pkg.synthetic.make_batch(["cigre14"], 512, seed=0)
    ref = oracle.MPN(*C2)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith("bias") and "convs" in n:
                p.uniform_(-0.1, 0.1)
    mine = pkg.MPN(*C2)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(DEV)
    oracle.train_step(ref, b, b["stats"])
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    st = tuple(s.to(DEV) for s in b["stats"])
    assert pkg.flags.CHAIN_EDGE
    out = mine(x[:, :8], ei, ea[:, :6])
    loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3],
                            edge_index=ei, reg_coefs=oracle.DEFAULT_REG_COEFS, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    loss.backward()
    tol = max(1e-4, 8.0 / out.shape[0])
    grads = dict(ref.named_parameters())
    for n, p in mine.named_parameters():
        if n in EDGE_W:
            assert rel_err(p.grad, grads[n].grad) < tol, (n, rel_err(p.grad, grads[n].grad))


def test_plan_replay_of_the_fused_step_is_bitwise_eager(pkg):
    model = _model(pkg, 3)
    x, ei, ea, st = _batch(pkg, ["cigre14"], 1024, seed=9)
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        out = model(x[:, :8], ei, ea[:, :6])
        loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3],
                                edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
        loss.backward(pkg.data.unit_grad(loss))
        return loss
    assert pkg.flags.CHAIN_EDGE
    loss_e = step().detach().clone()
    grads_e = [p.grad.detach().clone() for p in params]
    torch.cuda.synchronize()
    plan = pkg.graphs.PlannedStep(step)
    for p in params:
        p.grad.fill_(float("nan"))
    loss_p = plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_p, loss_e)
    for p, g in zip(params, grads_e):
        assert torch.equal(p.grad, g)
