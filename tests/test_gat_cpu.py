"""CPU: the GAT oracle against the hand-derived known answers, GAT_DSSE's construction (state_dict keys and shapes of the
reference's networks.py:113-156 through PyG's Sequential naming) and the options the kernels refuse."""
import json
import os

import pytest
import torch

import gat_oracle as go
from conftest import GOLDEN


def _known():
    with open(os.path.join(GOLDEN, "gat_known_answers.json")) as fh:
        return json.load(fh)["cases"]


def _t(v):
    return None if v is None else torch.tensor(v, dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(_known()))
def test_oracle_reproduces_the_known_answers(name):
    c = _known()[name]
    p = {k: _t(v) for k, v in c["params"].items()}
    out = go.gatv2(_t(c["x"]), torch.tensor(c["edge_index"]), _t(c["edge_attr"]), p, c["slope"], c["add_self_loops"])
    assert (out - _t(c["out"])).abs().max().item() < 1e-12


def test_oracle_attention_sums_to_one_per_target():
    x = torch.randn(5, 3, dtype=torch.float64)
    ei = torch.tensor([[0, 1, 2, 3, 3, 4, 4], [1, 2, 2, 2, 0, 4, 1]])
    p = {"att": torch.randn(1, 1, 3, dtype=torch.float64), "bias": None, "Wl": torch.randn(3, 3, dtype=torch.float64),
         "bl": torch.zeros(3, dtype=torch.float64), "Wr": torch.randn(3, 3, dtype=torch.float64), "br": torch.zeros(3, dtype=torch.float64)}
    _, alpha = go.gatv2(x, ei, None, p, return_alpha=True)
    _, tgt, _ = go.self_loops(ei, None, 5)
    s = torch.zeros(5, dtype=torch.float64).index_add(0, tgt, alpha)
    assert torch.allclose(s, torch.ones(5, dtype=torch.float64), atol=1e-12)


@pytest.mark.parametrize("num_layers", [1, 2, 8])
def test_state_dict_keys_shapes_and_strict_load(pkg, num_layers):
    m = pkg.GAT_DSSE(8, 32, 2, num_layers, 6)
    sd = m.state_dict()
    assert list(sd) == go.state_dict_keys(num_layers)
    ref = go.random_state_dict(num_layers)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    m.load_state_dict({k: v.float() for k, v in ref.items()}, strict=True)
    assert torch.equal(m.state_dict()["model.module_%d.weight" % (2 * (num_layers - 1))],
                       ref["model.module_%d.weight" % (2 * (num_layers - 1))].float())


def test_reference_attributes_and_initialisation(pkg):
    m = pkg.GAT_DSSE(dim_feat=8, dim_dense=32, dim_out=2, heads=1, num_layers=8, edge_dim=6)
    assert (m.dim_out, m.num_layers, m.dim_feat, m.dim_dense, m.edge_dim, m.dim_hidden, m.channels, m.heads, m.concat, m.slope,
            m.dropout, m.loop) == (2, 8, 8, 32, 6, 8, 8, 1, True, 0.2, 0.0, True)
    assert isinstance(m.nonlin, torch.nn.LeakyReLU) and m.model.module_1 is m.nonlin and m.model.module_13 is m.nonlin
    conv = m.model.module_0
    assert torch.count_nonzero(conv.bias) == 0
    a = (6.0 / (1 + 8)) ** 0.5
    assert conv.att.abs().max().item() <= a
    assert isinstance(pkg.GAT_DSSE(8, 32, 2, 3, 6, nonlin="tanh").nonlin, torch.nn.Tanh)
    assert isinstance(pkg.GAT_DSSE(8, 32, 2, 3, 6, nonlin="relu").nonlin, torch.nn.ReLU)


def test_runner_builds_the_driver_line(pkg):
    m = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER)
    assert isinstance(m, pkg.GAT_DSSE) and m.num_layers == 8 and m.dim_dense == 32 and m.edge_dim == 6 and m.heads == 1
    assert list(m.state_dict()) == go.state_dict_keys(8)


def test_unsupported_options_raise(pkg):
    with pytest.raises(ValueError, match="heads"):
        pkg.GAT_DSSE(8, 32, 2, 3, 6, heads=2)
    with pytest.raises(ValueError, match="dropout"):
        pkg.GAT_DSSE(8, 32, 2, 3, 6, dropout=0.1)
    with pytest.raises(ValueError, match="fill_value"):
        pkg.GATv2Conv(8, 8, edge_dim=6, fill_value="add")
    with pytest.raises(ValueError, match="bipartite"):
        pkg.GATv2Conv((8, 4), 8)
    with pytest.raises(ValueError, match="activation"):
        pkg.GAT_DSSE(8, 32, 2, 3, 6, nonlin="gelu")
    with pytest.raises(ValueError, match="32"):
        pkg.GATv2Conv(8, 33)
    with pytest.raises(ValueError, match="16"):
        pkg.GATv2Conv(8, 8, edge_dim=17)
    with pytest.raises(ValueError, match="32"):
        pkg.GAT_DSSE(8, 64, 2, 3, 6)
    conv = pkg.GATv2Conv(8, 8)
    x, ei = torch.randn(3, 8), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="return_attention_weights"):
        conv(x, ei, return_attention_weights=True)
    with pytest.raises(ValueError, match="bipartite"):
        conv((x, x), ei)
    with pytest.raises(RuntimeError, match="GPU"):        # no CPU fallback
        conv(x, ei)


GAT_GOLDENS = ["gat_real64", "gat_reswitched", "gat_ober", "gat_mixed", "gat_tanh_l2"]


def gat_golden(name):
    """case_<name>.npz (tests/golden/make_gat_goldens.py: the reference's GAT_DSSE + gsp_wls_edge + backward, in float64)."""
    import numpy as np
    z = np.load(os.path.join(GOLDEN, f"case_{name}.npz"), allow_pickle=False)
    t = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in "fi"}
    params = {k[len("param/"):]: v for k, v in t.items() if k.startswith("param/")}
    grads = {k[len("grad/"):]: v for k, v in t.items() if k.startswith("grad/")}
    return t, params, grads, [str(k) for k in z["keys"]], int(z["num_layers"]), str(z["nonlin"])


@pytest.mark.parametrize("name", GAT_GOLDENS)
def test_oracle_reproduces_the_reference_goldens(oracle, name):
    t, params, grads, _, num_layers, nonlin = gat_golden(name)
    x, ei, ea = t["x"], t["edge_index"], t["edge_attr"]
    sd = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = go.gat_dsse(x[:, :8], ei, ea[:, :6], sd, num_layers, nonlin)
    assert (out - t["out"]).abs().max().item() <= 1e-10 * t["out"].abs().max().item()
    reg = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
    loss = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=t["x_mean"], x_std=t["x_std"],
                               edge_mean=t["edge_mean"], edge_std=t["edge_std"], edge_index=ei, reg_coefs=reg, num_samples=None,
                               node_param=x[:, 8:], edge_param=ea[:, 6:])
    # (the model agrees to 1e-10.  The generator runs with float64 as torch's default dtype, so the reference's
    # sqrt(torch.tensor(3)) in get_pflow (data.py:378) is a float64 there, where oracle/dss2_oracle.py pins the float32 that the
    # usual default gives: the loss differs by ~1e-7 relative, and that carries into every gradient)
    assert abs(loss.item() - t["loss"].item()) <= 1e-6 * abs(t["loss"].item())
    loss.backward()
    for k, g in grads.items():
        assert (sd[k].grad - g).abs().max().item() <= 1e-5 * max(g.abs().max().item(), 1e-30), k


@pytest.mark.parametrize("name", GAT_GOLDENS)
def test_reference_state_dict_loads_strictly(pkg, name):
    _, params, _, keys, num_layers, nonlin = gat_golden(name)
    m = pkg.GAT_DSSE(8, 32, 2, num_layers, 6, nonlin=nonlin)
    assert list(m.state_dict()) == keys == go.state_dict_keys(num_layers)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(params[k].shape) for k in keys}
    m.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)


def test_bias_false_has_no_biases(pkg):
    """PyG builds lin_l / lin_r with bias=bias: GATv2Conv(bias=False) has no bias parameter anywhere."""
    conv = pkg.GATv2Conv(8, 8, edge_dim=6, bias=False)
    assert list(conv.state_dict()) == ["att", "lin_l.weight", "lin_r.weight", "lin_edge.weight"]
