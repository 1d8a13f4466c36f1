"""CPU: the gnn_dsse oracle against answers derived by hand (tests/golden/gnn_known_answers.json) and the reference goldens
(tests/golden/case_gnn_*.npz), strict loads of the goldens' state_dicts in their key order, gnn_dsse's construction (the reference's networks.py:11-69
attributes and state_dict keys through PyG's Sequential naming), the options the kernels refuse, the driver wiring and the
ctypes mirrors of the new structs."""
import json
import os

import pytest
import torch

import gnn_oracle as gor
from conftest import GOLDEN, ROOT

REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}

# 3 nodes: 0 -> 1 twice (a duplicate), 1 -> 2, and a self loop 2 -> 2
EI = torch.tensor([[0, 0, 1, 2], [1, 1, 2, 2]])
H = torch.tensor([[2.0], [3.0], [5.0]], dtype=torch.float64)
GNN_GOLDENS = gor.GOLDENS
gnn_golden = gor.load_golden


def _known():
    with open(os.path.join(GOLDEN, "gnn_known_answers.json")) as fh:
        return json.load(fh)["cases"]


def _t(v):
    return torch.tensor(v, dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(_known()))
def test_oracle_reproduces_the_known_answers(name):
    c = _known()[name]
    ei, h = torch.tensor(c["edge_index"]), _t(c["h"])
    n = h.size(0)
    if c["op"] == "P":
        out = gor.Structure(ei, n, True, c["add_self_loops"]).P(h)
    elif c["op"] == "gcn2":
        out = gor.gcn2(h, _t(c["x0"]), gor.Structure(ei, n), c["alpha"], _t(c["weight1"]))
    elif c["op"] == "fa":
        out = gor.fa(h, _t(c["x0"]), gor.Structure(ei, n), c["eps"], _t(c["att_l"]), _t(c["att_r"]))
    elif c["op"] == "tag":
        out = gor.tag(h, gor.Structure(ei, n, True, False), [_t(w) for w in c["lins"]], _t(c["bias"]))
    else:
        x = h.clone().requires_grad_(True)
        gor.gcn2(x, x, gor.Structure(ei, n), c["alpha"], _t(c["weight1"])).sum().backward()
        assert (x.grad - _t(c["dx"])).abs().max().item() < 1e-14
        return
    assert (out - _t(c["out"])).abs().max().item() < 1e-14


def test_known_answers_cover_the_issue_cases():
    ops = {c["op"] for c in _known().values()}
    assert {"P", "gcn2", "fa", "tag", "gcn2_dx"} <= ops
    assert any(c["op"] == "P" and c["add_self_loops"] for c in _known().values())


@pytest.mark.parametrize("name", GNN_GOLDENS)
def test_golden_files_are_small(name):
    assert os.path.getsize(os.path.join(GOLDEN, f"case_{name}.npz")) <= 100 * 1024


@pytest.mark.parametrize("name", GNN_GOLDENS)
def test_oracle_reproduces_the_reference_goldens(oracle, name):
    t, params, grads, keys, kw = gnn_golden(name)
    ref = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    x, ei, ea = t["x"].double(), t["edge_index"], t["edge_attr"].double()
    xr = x[:, :8].clone().requires_grad_(True)
    out = gor.GnnDSSE(ref, kw["num_layers"], kw["model"], main_param=kw["main_param"], K=kw["K"], nonlin=kw["nonlin"],
                      add_self_loops=kw["add_self_loops"])(xr, ei)
    assert (out - t["out"]).abs().max().item() <= 1e-10 * max(1.0, t["out"].abs().max().item())
    st = tuple(t[k].double() for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
    loss = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                               edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    loss.backward()
    # (1e-6 on the loss, 1e-5 on the gradients: the generator runs with float64 as torch's default dtype, where
    # oracle/dss2_oracle.py pins the float32 sqrt(3) of the usual default in get_pflow, as in tests/test_gine_cpu.py)
    assert abs(loss.item() - t["loss"].item()) <= 1e-6 * abs(t["loss"].item())
    assert sorted(grads) == sorted(keys)
    for k, g in grads.items():
        assert (ref[k].grad - g).abs().max().item() <= 1e-5 * max(g.abs().max().item(), 1e-30), k
    if "dx" in t:
        assert (xr.grad - t["dx"]).abs().max().item() <= 1e-5 * t["dx"].abs().max().item()


@pytest.mark.parametrize("name", GNN_GOLDENS)
def test_reference_state_dict_loads_strictly_in_key_order(pkg, name):
    _, params, _, keys, kw = gnn_golden(name)
    m = pkg.gnn_dsse(8, 32, 2, **kw)
    assert list(m.state_dict()) == keys
    m.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
    assert [k for k, _ in m.named_parameters()] == [k for k in keys]


def test_cached_oracle_keeps_the_first_structure():
    sd = {"model.module_0.weight1": torch.eye(1, dtype=torch.float64), "model.module_2.weight": torch.eye(1, dtype=torch.float64),
          "model.module_2.bias": torch.zeros(1, dtype=torch.float64), "model.module_3.weight": torch.eye(1, dtype=torch.float64),
          "model.module_3.bias": torch.zeros(1, dtype=torch.float64)}
    m = gor.GnnDSSE(sd, 2, "gcn2", nonlin="tanh")
    o1 = m(H, EI)
    assert torch.equal(m(H, EI[:, :1]), o1)
    with pytest.raises(IndexError):
        m(H[:2], EI[:, :1])


def test_reference_attributes_and_keys(pkg):
    m = pkg.gnn_dsse(8, 32, 2, 8)
    for k, v in dict(channels=8, main_param=0.1, dim_out=2, K=3, dropout=0., bias=True, theta=None, num_layers=8, shared_weights=True,
                     cached=True, normalize=True, add_self_loops=True).items():
        assert getattr(m, k) == v, k
    assert isinstance(m.nonlin, torch.nn.LeakyReLU)
    keys = list(m.state_dict())
    assert keys == [f"model.module_{2 * l}.weight1" for l in range(7)] + ["model.module_14.weight", "model.module_14.bias",
                                                                         "model.module_15.weight", "model.module_15.bias"]
    m = pkg.gnn_dsse(8, 32, 2, 3, model="gcn2", shared_weights=False)
    assert list(m.state_dict())[:2] == ["model.module_0.weight1", "model.module_0.weight2"]
    m = pkg.gnn_dsse(8, 32, 2, 3, model="fagcn")
    assert list(m.state_dict())[:2] == ["model.module_0.att_l.weight", "model.module_0.att_r.weight"]
    assert m.model.module_0.att_l.weight.shape == (1, 8)
    m = pkg.gnn_dsse(8, 32, 2, 3, model="tagcn", K=2)
    assert list(m.state_dict())[:4] == ["model.module_0.bias", "model.module_0.lins.0.weight", "model.module_0.lins.1.weight",
                                        "model.module_0.lins.2.weight"]
    m = pkg.gnn_dsse(8, 32, 2, 3, model="tagcn", K=3, bias=False)
    assert "model.module_0.bias" not in m.state_dict()
    assert list(pkg.gnn_dsse(8, 32, 2, 1).state_dict()) == ["model.module_0.weight", "model.module_0.bias", "model.module_1.weight",
                                                           "model.module_1.bias"]
    for nl, cls in (("relu", torch.nn.ReLU), ("tanh", torch.nn.Tanh)):
        assert isinstance(pkg.gnn_dsse(8, 32, 2, 3, nonlin=nl).nonlin, cls)
    assert m.model.module_1 is m.model.module_3 is m.nonlin


def test_strict_load_of_a_reference_shaped_state_dict(pkg):
    for kind in ("gcn2", "fagcn", "tagcn"):
        a, b = pkg.gnn_dsse(8, 32, 2, 8, K=2, model=kind), pkg.gnn_dsse(8, 32, 2, 8, K=2, model=kind)
        b.load_state_dict(a.state_dict(), strict=True)
        assert list(a.state_dict()) == list(b.state_dict())


def test_refusals(pkg):
    with pytest.raises(ValueError):
        pkg.gnn_dsse(8, 32, 2, 3, theta=0.5)
    with pytest.raises(ValueError):
        pkg.gnn_dsse(8, 32, 2, 3, model="fagcn", dropout=0.2)
    with pytest.raises(ValueError):
        pkg.gnn_dsse(8, 32, 2, 3, model="fagcn", normalize=False)
    with pytest.raises(ValueError):
        pkg.gnn_dsse(33, 32, 2, 3)
    with pytest.raises(ValueError):
        pkg.gnn_dsse(8, 33, 2, 3)
    with pytest.raises(ValueError):
        pkg.gnn_dsse(8, 32, 2, 3, model="tagcn", K=5)
    with pytest.raises(ValueError):
        pkg.gnn_dsse(8, 32, 2, 3, model="cheb")
    with pytest.raises(Exception):
        pkg.gnn_dsse(8, 32, 2, 3, nonlin="elu")
    with pytest.raises(ValueError):
        pkg.GCN2Conv(8, 0.1, theta=0.5, layer=1)
    m = pkg.gnn_dsse(8, 32, 2, 3)
    x = torch.randn(3, 8)
    with pytest.raises(ValueError):          # CPU tensors: no CPU path
        m(x, EI)
    with pytest.raises(TypeError):           # the reference's two-argument forward
        m(x, EI, torch.zeros(4, 6))
    with pytest.raises(ValueError):
        pkg.TAGConv(8, 8, K=2, normalize=False)(x, EI)
    with pytest.raises(ValueError):
        pkg.FAConv(8)(x, x, EI, return_attention_weights=True)
    with pytest.raises(ValueError):
        pkg.GCN2Conv(8, 0.1)(x, x, EI, edge_weight=torch.ones(4))


def test_runner_builds_the_driver_line_and_the_cli_accepts_it(pkg):
    for kind in ("gcn2", "fagcn", "tagcn"):
        m = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind)
        assert isinstance(m, pkg.gnn_dsse) and m.num_layers == 8 and m.K == 2 and m.cached is False and m.channels == 8
        assert m.model.module_14.out_features == 32 and m.model.module_15.out_features == 2
    src = open(os.path.join(ROOT, pkg.__name__, "runner.py")).read()
    assert '"gnn_dsse"]' in src and '"--gnn-model"' in src


def test_struct_layouts_match_the_header_sizes(pkg):
    """DSS2_GNN_MAX_K (tests/test_abi_cpu.py holds the mirrors of the new structs to the header)."""
    assert pkg._lib.GNN_MAX_K == 4
