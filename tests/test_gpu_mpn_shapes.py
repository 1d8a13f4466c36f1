"""The MPN path (MPN, SkipMPN, PFN, SkipPFN) against the fp64 oracle model on the graphs of tests/mpn_shape_cases.py: ELL widths 1 .. 8 and
CSR staging at 9, every tile height as the primary tiling, full tiles with the widest row in their last row, ragged packing, nodes
without a branch, a neighbour listed twice.

Every case runs the package's model with the oracle model's weights and backward(gout), once without and once with x.requires_grad
(the two take different routes: the chains' edge phases need a backward without an input gradient).  Bounds are the path's flat ones:
rel_err(out) < 1e-5, rel_err < 1e-4 for dx and every parameter gradient, with no 8 / N term (tests/test_mpn_shape_cases_cpu.py shows
every case fit for that: 4 x the fp32 oracle's error lies under them).  The topology on the device and the route the forward stored must be the
ones pinned on the CPU, so that each case is known to run the kernels it is there for."""
import contextlib
import importlib

import pytest
import torch

import mpn_shape_cases as mc
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c.name for c in mc.CASES]


def _stored_route(fn):
    """(the whole-stack kernels ran, the BlockRoutes the forward stored or None) of a model output's autograd node."""
    name = type(fn).__name__
    if name.startswith("_FusedStackFn"):
        return True, None
    if name.startswith("_PFNFn"):
        return False, [meta.route for meta in fn.meta[2]]
    assert name.startswith("_MPNFn"), name
    return False, [fn.meta[2].route]


@contextlib.contextmanager
def _switched_off(module, flag):
    """``module.flag = False``, restored on the way out."""
    keep = getattr(module, flag)
    setattr(module, flag, False)
    try:
        yield
    finally:
        setattr(module, flag, keep)


def _run(case, need_dx):
    """One forward and backward(gout) of the package's model: dict(out, dx, grads, topo, stack, routes)."""
    b = mc.batch(case.name)
    model = mc.build_model(case).to(DEV)
    x = b["x"].float().to(DEV).requires_grad_(need_dx)
    ei, ea = b["edge_index"].to(DEV), b["edge_attr"].float().to(DEV)
    out = model(x, ei, ea)
    stack, routes = _stored_route(out.grad_fn)
    out.backward(b["gout"].float().to(DEV))
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad, grads={k: p.grad for k, p in model.named_parameters()},
                topo=mc.pkg().topology.get_topology(ei, x.size(0)), stack=stack, routes=routes)


def _errors(tag, got, want, need_dx):
    """Prints every error beside its bound; returns the failures."""
    errs = [("out", rel_err(got["out"], want["out"]), mc.OUT_BOUND)]
    if need_dx:
        errs.append(("dx", rel_err(got["dx"], want["dx"]), mc.GRAD_BOUND))
    assert set(got["grads"]) == set(want["grads"])
    errs += [(k, rel_err(got["grads"][k], g), mc.GRAD_BOUND) for k, g in want["grads"].items()]
    for k, e, bound in errs:
        print(f"[mpn shapes] {tag}: {k} {e:.2e} (bound {bound:.0e})")
    return [(k, e, bound) for k, e, bound in errs if not e < bound]


@pytest.mark.parametrize("need_dx", [False, True], ids=["no_dx", "dx"])
@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_mpn_path_on_shapes_the_grids_never_produce(case, need_dx):
    got = _run(case, need_dx)
    topo = got["topo"]
    assert not topo.global_only
    assert (topo.nrb, topo.ntiles, topo.ell, topo.ellT) == mc.STRUCTURE[case.name][:4]
    assert topo.stats()["max_segment"] == mc.STRUCTURE[case.name][4]
    _, rows, wg, edge = mc.route_literal(case, need_dx, block_routes=got["routes"], topo=topo)
    want_route = mc.ROUTE[case.name][need_dx]
    print(f"[mpn shapes] {case.name} need_dx={need_dx}: stack {got['stack']}, wgrad {wg}, edge families {edge}")
    for bi, row in enumerate(rows):
        print(f"    block {bi}: " + ", ".join(f"{f}={v}" for f, v in zip(mc.ROUTE_FIELDS, row)))
    assert (got["stack"], rows, wg, edge) == want_route
    bad = _errors(f"{case.name} need_dx={need_dx}", got, mc.reference(case.name), need_dx)
    assert not bad, bad


@pytest.mark.parametrize("name", ["c2_ell8_head_edge", "full64_ell5"])
def test_fused_edge_phases_agree_with_the_separate_launches(name):
    """flags.CHAIN_EDGE = False takes the edge MLP out of both chains (its own launches, the grids' tested route at widths 3 and 4):
    the fused phases of these widths must agree with it within the same bounds."""
    case, P = mc.BY_NAME[name], mc.pkg()
    fused = _run(case, False)
    assert fused["routes"][0].bwd_edge and fused["routes"][0].edge == mc.ROUTE[name][False][1][0][mc.ROUTE_FIELDS.index("edge")]
    with _switched_off(P.flags, "CHAIN_EDGE"):
        apart = _run(case, False)
    assert not apart["routes"][0].edge and not apart["routes"][0].bwd_edge
    assert apart["routes"][0]._replace(edge=fused["routes"][0].edge, bwd_edge=True) == fused["routes"][0]      # nothing else moved
    bad = _errors(f"{name} CHAIN_EDGE off, against the oracle", apart, mc.reference(name), False)
    bad += _errors(f"{name} fused against CHAIN_EDGE off", fused, {k: apart[k] for k in ("out", "grads")}, False)
    assert not bad, bad


@pytest.mark.parametrize("need_dx", [False, True], ids=["no_dx", "dx"])
@pytest.mark.parametrize("name", ["pairs_ell1", "stack_full64_ell4"])
def test_block_route_of_the_whole_stack_cases(name, need_dx):
    """The two cases the whole-stack kernels take, with those switched off (stack.STACK_KERNEL = False): the blocks run the per-block route
    pinned beside the stack answer -- bf16x6 chains of hid 32 at ELL width 1, and on full 64-row tiles with a node without a branch."""
    case = mc.BY_NAME[name]
    with _switched_off(importlib.import_module(mc.PKG_NAME + ".stack"), "STACK_KERNEL"):
        got = _run(case, need_dx)
    assert not got["stack"]
    _, rows, _, _ = mc.route_literal(case, need_dx, block_routes=got["routes"], topo=got["topo"])
    assert rows == mc.ROUTE[name][need_dx][1]
    bad = _errors(f"{name} need_dx={need_dx}, stack kernels off", got, mc.reference(name), need_dx)
    assert not bad, bad
