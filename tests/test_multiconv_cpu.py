"""CPU: the MultiConvNet / ChebConv oracle (tests/cheb_oracle.py) against the reference goldens (tests/golden/case_multiconv_*.npz),
a hand-derived ChebConv answer, the models' construction (the reference's networks.py:737-835 attributes and state_dict keys), strict
loads of the goldens' state_dicts, the options the kernels refuse and the ctypes mirrors of the new structs."""
import os
import types

import pytest
import torch

import cheb_oracle as cor
from conftest import load_pkg


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", cor.GOLDENS)
def test_oracle_reproduces_the_reference_golden(name):
    """out, every parameter gradient and dx to 1e-9 relative, in fp64."""
    t, params, grads, keys, args = cor.load_golden(name)
    sd = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    x = t["x"].clone().requires_grad_(True)
    out = cor.multiconv(sd, x, t["edge_index"], t["edge_attr"])
    assert _rel(out.detach(), t["out"]) < 1e-9
    out.backward(t["gout"])
    for k in keys:
        got = sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])      # (K = 1: edge_trans is not reached)
        assert got.shape == grads[k].shape
        err = float((got - grads[k]).abs().max()) if float(grads[k].abs().max()) == 0 else _rel(got, grads[k])
        assert err < 1e-9, (k, err)
    if "dx" in t:
        assert _rel(x.grad[:, 4:12], t["dx"]) < 1e-9
    assert float(x.grad[:, :4].abs().max()) == 0 and float(x.grad[:, 12:].abs().max()) == 0


def test_oracle_chebconv_by_hand():
    """A path 0 - 1 - 2 (both directions), weights 1 and 3, one channel, x = (1, 2, 4), lins = (1, 10, 100).
    deg = (1, 4, 3); entries -1, -3, 1, 4, 3 -> lambda_max = 8; what = -1/4, -3/4; d = (-3/4, 0, -1/4).
    T_1 = A x = (-3/4 - 2/4, -1/4 - 12/4, -1 - 6/4) = (-5/4, -13/4, -5/2);
    A T_1 = (15/16 + 13/16, 5/16 + 30/16, 10/16 + 39/16) = (28/16, 35/16, 49/16); T_2 = 2 A T_1 - x = (5/2, 19/8, 17/8)."""
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    w = torch.tensor([1.0, 1.0, 3.0, 3.0], dtype=torch.float64)
    x = torch.tensor([[1.0], [2.0], [4.0]], dtype=torch.float64)
    lins = [torch.tensor([[v]], dtype=torch.float64) for v in (1.0, 10.0, 100.0)]
    out = cor.cheb_conv(x, ei, w, lins, torch.tensor([0.5], dtype=torch.float64))
    want = torch.tensor([[1 - 12.5 + 250 + 0.5], [2 - 32.5 + 237.5 + 0.5], [4 - 25 + 212.5 + 0.5]], dtype=torch.float64)
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
    # a given lambda_max is used as it is; a self loop changes nothing
    ei2, w2 = torch.cat([ei, torch.tensor([[2], [2]])], dim=1), torch.cat([w, torch.tensor([7.0], dtype=torch.float64)])
    assert torch.equal(cor.cheb_conv(x, ei2, w2, lins, lambda_max=8.0), cor.cheb_conv(x, ei, w, lins))


@pytest.mark.parametrize("name", cor.GOLDENS)
def test_construction_and_strict_load(name):
    pkg = load_pkg()
    t, params, grads, keys, args = cor.load_golden(name)
    torch.manual_seed(0)
    net = pkg.MultiConvNet(*args)
    assert list(net.state_dict()) == keys
    net.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
    featn, feate, dim_out, dim_hid, n_layers, K, p = args
    assert (net.dim_featn, net.dim_feate, net.dim_out, net.dim_hid, net.n_gnn_layers, net.K, net.dropout_rate) == (featn, 2, dim_out, dim_hid, n_layers, K, p)
    assert len(net.convs) == max(n_layers, 2)
    first = net.convs[0]
    assert (first.num_convs, first.in_channels, first.out_channels) == (2, featn, dim_out if n_layers == 1 else dim_hid)
    assert isinstance(first.convs[0], pkg.ChebConv) and len(first.convs[0].lins) == K
    assert net.convs[-1].in_channels == dim_hid and net.convs[-1].out_channels == dim_out


def test_exports_and_initialisation():
    pkg = load_pkg()
    assert pkg.networks.MultiConvNet is pkg.MultiConvNet is pkg.cheb.MultiConvNet
    assert pkg.networks.WrappedMultiConv is pkg.WrappedMultiConv and pkg.networks.ChebConv is pkg.ChebConv
    torch.manual_seed(3)
    cv = pkg.ChebConv(5, 7, 3)
    assert list(cv.state_dict()) == ["bias", "lins.0.weight", "lins.1.weight", "lins.2.weight"]
    assert float(cv.bias.abs().max()) == 0 and cv.lins[0].weight.shape == (7, 5)
    a = (6.0 / 12) ** 0.5
    assert all(float(l.weight.abs().max()) <= a for l in cv.lins)
    assert list(pkg.ChebConv(5, 7, 2, bias=False).state_dict()) == ["lins.0.weight", "lins.1.weight"]
    src = open(os.path.join(os.path.dirname(pkg.cheb.__file__), "cheb.py")).read()
    assert "oracle" not in src


def test_refusals():
    pkg = load_pkg()
    for norm in ("sym", "rw"):
        with pytest.raises(ValueError):
            pkg.ChebConv(4, 4, 2, normalization=norm)
    for bad in ((33, 4, 2), (4, 33, 2), (4, 4, 0), (4, 4, 5)):
        with pytest.raises(ValueError):
            pkg.ChebConv(*bad)
    with pytest.raises(ValueError):
        pkg.WrappedMultiConv(5, 4, 4, 2)
    with pytest.raises(ValueError):
        pkg.MultiConvNet(8, 5, 2, 33, 3, 2, 0.0)
    with pytest.raises(ValueError):
        pkg.MultiConvNet(8, 5, 2, 8, 1, 2, 0.0)          # n_gnn_layers = 1 chains only with dim_out == dim_hid
    pkg.MultiConvNet(8, 5, 8, 8, 1, 2, 0.0)
    with pytest.raises(AssertionError):
        pkg.MultiConvNet(8, 6, 2, 8, 2, 2, 0.0)          # the reference asserts dim_feate == 5
    cv = pkg.ChebConv(4, 4, 2)
    x, ei = torch.zeros(3, 4), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError):                      # batch with a per-graph lambda_max
        cv(x, ei, batch=torch.zeros(3, dtype=torch.int64), lambda_max=torch.tensor([2.0, 2.0]))
    with pytest.raises(ValueError):
        cv(x, ei, lambda_max=torch.tensor([2.0, 2.0]))


def test_cpu_tensors_raise():
    pkg = load_pkg()
    x, ei = torch.zeros(3, 4), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError):
        pkg.ChebConv(4, 4, 2)(x, ei)
    with pytest.raises(RuntimeError):
        pkg.WrappedMultiConv(2, 4, 4, 2)(x, [ei, ei], [torch.ones(2), torch.ones(2)])
    net = pkg.MultiConvNet(8, 5, 2, 8, 2, 2, 0.0)
    data = types.SimpleNamespace(x=torch.zeros(3, 20), edge_index=ei, edge_attr=torch.zeros(2, 5))
    with pytest.raises(RuntimeError):
        net(data)


def test_struct_layouts_match_the_header_sizes():
    """The DSS2_CHEB_MAX_* values and the exported entries (tests/test_abi_cpu.py holds the mirrors to the header)."""
    L = load_pkg()._lib
    assert (L.CHEB_MAX_K, L.CHEB_MAX_CONVS) == (4, 4)
    for name in ("dss2_cheb_forward", "dss2_cheb_backward", "dss2_cheb_edge_forward", "dss2_cheb_edge_backward"):
        assert name in L.EXPORTED_SYMBOLS
