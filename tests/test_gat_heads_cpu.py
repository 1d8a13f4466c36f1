"""CPU: multi-head GATv2Conv / GAT_DSSE construction (state_dict shapes, the refusals, the runner's concat rule) and the fp64
multi-head restatement tests/gat_heads_oracle.py held to the single-head one of tests/gat_oracle.py, which the known answers and
the reference goldens pin."""
import pytest
import torch

import gat_heads_oracle as gho
import gat_oracle as go


def _graph(n=9, seed=0, ed=6):
    """A small graph with an isolated target (node n - 1 has no incoming edge), a self loop and a duplicate edge."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (3 * n,), generator=g)
    tgt = torch.randint(0, n - 1, (3 * n,), generator=g)
    ei = torch.stack([torch.cat([src, torch.tensor([2, 4])]), torch.cat([tgt, torch.tensor([2, 5])])])
    ei = torch.cat([ei, ei[:, :1]], 1)
    ea = torch.randn(ei.size(1), ed, generator=g, dtype=torch.float64) if ed else None
    return ei, ea


def test_state_dict_shapes_of_a_four_head_mean_model(pkg):
    m = pkg.GAT_DSSE(8, 32, 2, 3, 6, heads=4, concat=False)
    sd = m.state_dict()
    assert list(sd) == go.state_dict_keys(3)
    ref = gho.random_state_dict(3, 4)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert tuple(sd["model.module_0.att"].shape) == (1, 4, 8)
    assert tuple(sd["model.module_0.bias"].shape) == (8,)
    assert tuple(sd["model.module_0.lin_l.weight"].shape) == (32, 8)
    assert tuple(sd["model.module_0.lin_r.bias"].shape) == (32,)
    assert tuple(sd["model.module_0.lin_edge.weight"].shape) == (32, 6)
    m.load_state_dict({k: v.float() for k, v in ref.items()}, strict=True)
    assert torch.equal(m.state_dict()["model.module_2.att"], ref["model.module_2.att"].float())
    assert (m.heads, m.concat, m.model.module_0.heads, m.model.module_0.concat) == (4, False, 4, False)


def test_conv_shapes_for_both_concat_modes(pkg):
    cat = pkg.GATv2Conv(8, 8, heads=2, concat=True)
    assert tuple(cat.bias.shape) == (16,) and tuple(cat.att.shape) == (1, 2, 8) and tuple(cat.lin_l.weight.shape) == (16, 8)
    mean = pkg.GATv2Conv(8, 8, heads=2, concat=False, edge_dim=3)
    assert tuple(mean.bias.shape) == (8,) and tuple(mean.lin_r.weight.shape) == (16, 8) and tuple(mean.lin_edge.weight.shape) == (16, 3)
    one = pkg.GATv2Conv(8, 8, concat=False)       # nothing changes at one head
    assert tuple(one.bias.shape) == (8,) and tuple(one.att.shape) == (1, 1, 8)
    a = (6.0 / (2 + 8)) ** 0.5                     # glorot over the last two dimensions of att, as PyG
    assert cat.att.abs().max().item() <= a and torch.count_nonzero(cat.bias) == 0


def test_refusals(pkg):
    with pytest.raises(ValueError, match="heads") as ex:
        pkg.GAT_DSSE(8, 32, 2, 3, 6, heads=2)
    assert "concat" in str(ex.value)
    with pytest.raises(ValueError, match="concat"):
        pkg.GAT_DSSE(8, 32, 2, 8, 6, heads=4, concat=True)
    assert pkg.GAT_DSSE(8, 32, 2, 1, 6, heads=2).heads == 2          # no conv: nothing to concatenate
    with pytest.raises(ValueError, match="heads"):
        pkg.GATv2Conv(8, 8, heads=5)                                 # 5 * 8 lanes
    with pytest.raises(ValueError, match="heads"):
        pkg.GATv2Conv(8, 5, heads=5)                                 # 5 * 8 lanes: Cp = 8
    assert pkg.GATv2Conv(8, 5, heads=4).heads == 4                   # Cp = 8: exactly 32 lanes
    assert pkg.GATv2Conv(32, 1, heads=32, concat=False).heads == 32
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="heads"):
            pkg.GATv2Conv(8, 8, heads=bad)
    with pytest.raises(ValueError, match="dropout"):                 # attention dropout stays refused
        pkg.GATv2Conv(8, 8, heads=2, dropout=0.1)


def test_a_stack_must_share_heads_and_concat(pkg):
    mk = lambda **kw: pkg.GATv2Conv(8, 8, edge_dim=6, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="heads"):
        pkg.gat._Spec([mk(heads=2, concat=False), mk(heads=1)], None, "none", 45)
    with pytest.raises(ValueError, match="concat"):
        pkg.gat._Spec([mk(heads=2, concat=False), pkg.GATv2Conv(8, 4, heads=2, concat=True, edge_dim=6)], None, "none", 45)
    with pytest.raises(ValueError, match="concat"):                  # the head Linears after concatenated heads
        pkg.gat._Spec([pkg.GATv2Conv(8, 4, heads=2)], [torch.nn.Linear(8, 32), torch.nn.Linear(32, 2)], "leaky_relu", 45)


@pytest.mark.parametrize("cin,c,heads,concat,group", [(8, 8, 1, True, 8), (8, 8, 2, False, 16), (8, 8, 4, True, 32), (5, 5, 3, True, 32),
                                                      (3, 3, 2, False, 8), (8, 2, 4, True, 8), (20, 2, 2, True, 32)])
def test_spec_lane_group_and_slab_columns(pkg, cin, c, heads, concat, group):
    conv = pkg.GATv2Conv(cin, c, heads=heads, concat=concat, edge_dim=6)
    spec = pkg.gat._Spec([conv], None, "none", 45)
    assert spec.group == group and spec.x_cols == cin
    assert spec.total == sum(p.numel() for p in conv.parameters())   # one slab column per parameter element, in parameter order
    assert [p.numel() for p in conv._slots()] == [heads * c, heads * c if concat else c, heads * c * cin, heads * c, heads * c * cin,
                                                  heads * c, heads * c * 6]


def test_runner_builds_several_heads_as_their_mean(pkg):
    m = pkg.runner.build_model("GAT_DSSE", {**pkg.runner.HYPER, "heads": 4})
    assert isinstance(m, pkg.GAT_DSSE) and m.heads == 4 and m.concat is False and m.num_layers == 8
    assert tuple(m.model.module_0.att.shape) == (1, 4, 8) and tuple(m.model.module_0.bias.shape) == (8,)
    one = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER)
    assert one.heads == 1 and one.concat is True


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("loops", [True, False])
def test_oracle_at_one_head_is_the_single_head_oracle(concat, loops):
    ei, ea = _graph()
    x = torch.randn(9, 5, dtype=torch.float64)
    p = gho.random_conv_params(5, 7, 1, concat=concat, seed=3)
    a = gho.gatv2_heads(x, ei, ea, p, 1, concat, add_self_loops=loops)
    b = go.gatv2(x, ei, ea, p, add_self_loops=loops)
    assert torch.equal(a, b) or (a - b).abs().max().item() < 1e-14


@pytest.mark.parametrize("heads,c,ed,bias", [(2, 8, 6, True), (3, 5, None, True), (4, 2, 3, False)])
@pytest.mark.parametrize("concat", [True, False])
def test_oracle_is_the_heads_side_by_side_or_averaged(heads, c, ed, bias, concat):
    """PyG's definition: a multi-head conv is its heads' single-head convs, concatenated (each with its bias block) or
    averaged with the bias added once."""
    ei, ea = _graph(ed=ed)
    x = torch.randn(9, 6, dtype=torch.float64)
    p = gho.random_conv_params(6, c, heads, concat=concat, ed=ed, bias=bias, seed=heads)
    out = gho.gatv2_heads(x, ei, ea, p, heads, concat)
    parts = [go.gatv2(x, ei, ea, gho.head_params(p, h, heads, concat)) for h in range(heads)]
    if concat:
        want = torch.cat(parts, 1)
    else:
        want = torch.stack(parts).mean(0) + (p["bias"] if bias else 0.0)
    assert tuple(out.shape) == (9, heads * c if concat else c)
    assert (out - want).abs().max().item() < 1e-13
    # the isolated target without self loops: an empty softmax, the bias alone
    bare = gho.gatv2_heads(x, ei, ea, p, heads, concat, add_self_loops=False)[-1]
    assert torch.equal(bare, p["bias"] if bias else torch.zeros_like(bare))


def test_model_oracle_at_one_head_is_the_single_head_model_oracle():
    ei, ea = _graph(n=12)
    x = torch.randn(12, 8, dtype=torch.float64)
    sd = go.random_state_dict(3, seed=4)
    a = gho.gat_dsse_heads(x, ei, ea, sd, 3, 1, "tanh")
    b = go.gat_dsse(x, ei, ea, sd, 3, "tanh")
    assert (a - b).abs().max().item() < 1e-14


def _golden():
    """case_gat_heads4_mean.npz (tests/golden/make_gat_heads_goldens.py: the reference's GAT_DSSE(heads=4, concat=False,
    num_layers=3) + gsp_wls_edge + backward, in float64)."""
    import os

    import numpy as np
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, "case_gat_heads4_mean.npz"), allow_pickle=False)
    t = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in "fi"}
    params = {k[len("param/"):]: v for k, v in t.items() if k.startswith("param/")}
    grads = {k[len("grad/"):]: v for k, v in t.items() if k.startswith("grad/")}
    return t, params, grads, [str(k) for k in z["keys"]], int(z["num_layers"]), str(z["nonlin"]), int(z["heads"])


def test_oracle_reproduces_the_reference_multi_head_golden(oracle):
    """The same bounds as tests/test_gat_cpu.py holds the single-head restatement to (and for the same reason: the generator's
    float64 default dtype changes one constant of the reference's loss by 1e-7)."""
    t, params, grads, _, num_layers, nonlin, heads = _golden()
    x, ei, ea = t["x"], t["edge_index"], t["edge_attr"]
    sd = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = gho.gat_dsse_heads(x[:, :8], ei, ea[:, :6], sd, num_layers, heads, nonlin)
    assert (out - t["out"]).abs().max().item() <= 1e-10 * t["out"].abs().max().item()
    reg = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
    loss = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=t["x_mean"], x_std=t["x_std"],
                               edge_mean=t["edge_mean"], edge_std=t["edge_std"], edge_index=ei, reg_coefs=reg, num_samples=None,
                               node_param=x[:, 8:], edge_param=ea[:, 6:])
    assert abs(loss.item() - t["loss"].item()) <= 1e-6 * abs(t["loss"].item())
    loss.backward()
    assert sorted(grads) == sorted(sd)
    for k, g in grads.items():
        assert (sd[k].grad - g).abs().max().item() <= 1e-5 * max(g.abs().max().item(), 1e-30), k


def test_reference_multi_head_state_dict_loads_strictly(pkg):
    _, params, _, keys, num_layers, nonlin, heads = _golden()
    m = pkg.GAT_DSSE(8, 32, 2, num_layers, 6, heads=heads, concat=False, nonlin=nonlin)
    assert list(m.state_dict()) == keys == go.state_dict_keys(num_layers)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(params[k].shape) for k in keys}
    m.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
