"""The MPN path against the fp64 oracle model at the hidden widths, head widths, K and depths of tests/mpn_width_cases.py: dim_hid off
the 32 grid (a partly filled last column group, K padded beyond the real width), every chain family with its row split and wave counts,
dim_out 1 .. 11, K 1 .. 3, chains longer than flags.CHAIN_MAX, and one SkipPFN stack at a width the whole-stack kernels decline.

Every case runs like tests/test_gpu_mpn_shapes.py runs its own: the package's model with the oracle model's weights, one forward and
backward(gout), without and with x.requires_grad; the device topology and the stored routes, the weight-gradient and edge plans and the
chain records must be the ones pinned on the CPU; out is held to 1e-5, dx and every parameter gradient to 1e-4, flat (tests/
test_mpn_width_cases_cpu.py shows every case fit for that).  Besides:

  last column group   every parameter gradient with a hid-sized axis, on columns 32 * (hid // 32) .. of that axis alone, normalised by
                      that slice's own fp64 maximum, to the same bound: a kernel wrong only in the partial group cannot hide behind a
                      larger entry elsewhere
  pad columns         every case with hid % 32 != 0 or a padded K runs a second time after NaN was left in freed device memory: finite and
                      bit-identical to the first run
  formats             four widths again under each flag that takes a 16-bit chain or weight-gradient form away; the stored route moves in
                      the pinned fields only
  split chains        the 9- and 10-layer chains with CHAIN_MAX = 3 against the oracle and against the default run
  heads apart         every case with a fused head with flags.CHAIN_HEAD and flags.CHAIN_HEAD_FWD off

Every error is printed beside its bound; the worst error / bound per tensor kind is printed as the module finishes."""
# Measured on an MI355X when these tests were written (all 74 pass; every second run bit-identical), worst error / bound over every
# comparison with the oracle in this module:
#   out                0.066   t32_w200 (bf16x6 chain, 8 waves, hid 200)
#   dx                 0.008   t32_w200
#   conv weight        0.032   t96_d11, convs.1.lins.1.weight (ten chained f16x3 layers)
#   head weight        0.007   w260_nochain, convs.2.lins.0.weight
#   edge-MLP weight    0.036   t96_d11, edge_aggr.edge_aggr.0.bias
#   last-group slice   0.016   w136_w8, convs.3.lins.2.weight[axis 1, 128:]
# No case missed a bound and no kernel or selection had to change.  One case is not what its first description said: dim_hid 260 does
# not run the fused block layer by layer but leaves it for the per-layer autograd nodes (wc.GENERAL_PATH); it stays, as that path three layers deep
# with a last column group of four.
import functools
import math

import pytest
import torch

import mpn_shape_cases as mc
import mpn_width_cases as wc
from test_gpu_mpn_shapes import DEV, _stored_route

pytestmark = pytest.mark.gpu
IDS = [c.name for c in wc.ALL_CASES]
KINDS = ("out", "dx", "conv weight", "head weight", "edge-MLP weight", "last-group slice")
WORST = {}      # tensor kind -> (error / bound, where), over everything this module compared with the oracle


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    yield
    for kind in KINDS:
        if kind in WORST:
            print(f"\n[mpn widths] worst error / bound, {kind}: {WORST[kind][0]:.3f} ({WORST[kind][1]})", end="")
    print()


def _run(case, need_dx):
    """One forward and backward(gout) of the package's model, as tests/test_gpu_mpn_shapes.py runs its cases: dict(out, dx, grads, topo,
    stack, routes).  A case of wc.GENERAL_PATH stores no route (routes None): its output must come from the per-layer nodes."""
    b = mc.batch(case)
    model = mc.build_model(case).to(DEV)
    x = b["x"].float().to(DEV).requires_grad_(need_dx)
    ei, ea = b["edge_index"].to(DEV), b["edge_attr"].float().to(DEV)
    out = model(x, ei, ea)
    if case.name in wc.GENERAL_PATH:
        assert type(out.grad_fn).__name__.startswith("_TAGConvFn"), type(out.grad_fn).__name__
        stack, routes = False, None
    else:
        stack, routes = _stored_route(out.grad_fn)
    out.backward(b["gout"].float().to(DEV))
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad, grads={k: p.grad for k, p in model.named_parameters()},
                topo=mc.pkg().topology.get_topology(ei, x.size(0)), stack=stack, routes=routes)


def _err(got, want):
    """max |got - want| / max |want| in fp64 (conftest.rel_err, for tensors on any device)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def _check(tag, case, got, want, need_dx, oracle=True):
    """Holds ``got`` to the flat bounds against ``want`` (the oracle's fp64 run, or another run of the package), whole tensors and the last
    column group of every hid-sized axis on its own.  Prints every error beside its bound; returns the failures."""
    rows = [("out", "out", _err(got["out"], want["out"]), mc.OUT_BOUND)]
    if need_dx:
        rows.append(("dx", "dx", _err(got["dx"], want["dx"]), mc.GRAD_BOUND))
    assert set(got["grads"]) == set(want["grads"])
    for k, g in want["grads"].items():
        rows.append((wc.kind_of(case, k), k, _err(got["grads"][k], g), mc.GRAD_BOUND))
        for (label, s_want), (_, s_got) in zip(wc.hid_slices(case, k, g), wc.hid_slices(case, k, got["grads"][k])):
            rows.append(("last-group slice", label, _err(s_got, s_want), mc.GRAD_BOUND))
    for kind, k, e, bound in rows:
        print(f"[mpn widths] {tag}: {k} {e:.2e} (bound {bound:.0e})")
        if oracle and not (WORST.get(kind, (-1.0,))[0] >= e / bound):      # (a NaN replaces anything)
            WORST[kind] = (e / bound, f"{tag}: {k}")
    return [(k, e, bound) for _, k, e, bound in rows if not e < bound]


def _assert_structure(case, topo):
    want = mc.STRUCTURE[wc.BASE[case.name]]
    assert not topo.global_only
    assert (topo.nrb, topo.ntiles, topo.ell, topo.ellT) == want[:4]
    assert topo.stats()["max_segment"] == want[4]


def _leave_nan_in_freed_memory():
    """Fills what the caching allocator will hand out next with NaN: the cache is emptied, then one 20 MB block of the large pool, 8 MB
    of the small pool and a few small tensors of each size class (they go into the holes that tensors still alive leave in their segments)
    are filled and freed; the next run's activations, slabs and weight packs are carved out of them."""
    def nan(n):
        return torch.full((n,), math.nan, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    blocks = [nan(n) for n in (1 << 9, 1 << 12, 1 << 15) for _ in range(8)] + [nan(1 << 17) for _ in range(16)] + [nan(5 << 20)]
    torch.cuda.synchronize()
    del blocks
    # the allocator does hand the large block out again, as it was left (the only cached block of its size: an exact fit)
    assert torch.isnan(torch.empty(5 << 20, dtype=torch.float32, device=DEV)).all()


@functools.lru_cache(maxsize=None)
def _default_run(name):
    """The default route of a case without an input gradient, run once for the reruns to compare with."""
    return _run(wc.BY_NAME[name], False)


def _print_route(tag, stack, rows, wg, edge, chains):
    print(f"[mpn widths] {tag}: stack {stack}, wgrad {wg}, edge families {edge}")
    for bi, (row, (pf, pb)) in enumerate(zip(rows, chains)):
        print(f"    block {bi}: " + ", ".join(f"{f}={v}" for f, v in zip(mc.ROUTE_FIELDS, row)))
        print(f"    block {bi}: chain record forward {pf}, transposed {pb}")


@pytest.mark.parametrize("need_dx", [False, True], ids=["no_dx", "dx"])
@pytest.mark.parametrize("case", wc.ALL_CASES, ids=IDS)
def test_mpn_path_at_widths_heads_and_depths_no_other_test_runs(case, need_dx):
    tag = f"{case.name} need_dx={need_dx}"
    got = _run(case, need_dx)
    _assert_structure(case, got["topo"])
    _, rows, wg, edge, chains = wc.route_literal(case, need_dx, block_routes=got["routes"], topo=got["topo"])
    _print_route(tag, got["stack"], rows, wg, edge, chains)
    assert (got["stack"], rows, wg, edge, chains) == wc.ROUTE[case.name][need_dx]
    bad = _check(tag, case, got, mc.reference(case), need_dx)
    if wc.pad_sensitive(case):
        _leave_nan_in_freed_memory()
        again = _run(case, need_dx)
        assert again["routes"] == got["routes"]
        pairs = [("out", got["out"], again["out"])] + ([("dx", got["dx"], again["dx"])] if need_dx else [])
        pairs += [(k, g, again["grads"][k]) for k, g in got["grads"].items()]
        for k, a, b in pairs:
            if not torch.isfinite(b).all():
                bad.append((f"{k} after NaN in freed memory", math.nan, 0.0))
            elif not torch.equal(a, b):
                bad.append((f"{k} differs between two runs", _err(b, a), 0.0))
        print(f"[mpn widths] {tag}: second run after NaN in freed memory compared, {len(pairs)} tensors")
    assert not bad, bad


@pytest.mark.parametrize("variant", list(wc.VARIANT_FLAGS))
@pytest.mark.parametrize("name", wc.VARIANT_CASES)
def test_formats_of_one_width_agree(name, variant):
    """Each flag takes one 16-bit form away (flags.py): CHAIN_F16 -> bf16x6 chains, CHAIN_BF16 -> the fp32 chain (row split 2 at width 36;
    none on 192-row tiles: layer by layer), CHAIN_LAYERS -> dss2_gemm_prop per layer, WGRAD_F16 -> the bf16x6 and WGRAD_BF16 -> the fp32 weight
    gradient.  Every form meets the oracle bounds, and the stored route moves in the pinned fields only."""
    case, tag = wc.BY_NAME[name], f"{name} {variant}"
    want_moved, want_wg, want_edge = wc.VARIANTS[name][variant]
    default = _default_run(name)
    d_route = default["routes"][0]
    off = {f: False for f in wc.VARIANT_FLAGS[variant]}
    if want_wg[1] == wc.WG_NONE:
        # no weight-gradient kernel of that format for this tile height and width: the library must say so, not run something else
        assert wc.variant_literal(case, variant, default=d_route, block_route=d_route, topo=default["topo"]) == ({}, want_wg, want_edge)
        with wc.flags_set(**off), pytest.raises(RuntimeError, match="wgrad"):
            _run(case, False)
        torch.cuda.synchronize()
        return
    with wc.flags_set(**off):
        got = _run(case, False)
    _assert_structure(case, got["topo"])
    moved, wg, edge = wc.variant_literal(case, variant, default=d_route, block_route=got["routes"][0], topo=got["topo"])
    print(f"[mpn widths] {tag}: route fields moved {moved}, wgrad {wg}, edge families {edge}")
    assert (moved, wg, edge) == (want_moved, want_wg, want_edge)
    assert got["routes"][0] == d_route._replace(**want_moved)
    bad = _check(tag, case, got, mc.reference(case), False)
    assert not bad, bad


@pytest.mark.parametrize("name", wc.SPLIT_CASES)
def test_a_chain_split_into_more_launches_agrees(name):
    """flags.CHAIN_MAX = 3: ops.gemm_prop_chain runs the 9 (10) chained layers as three (four) launches per direction instead of two, each
    reading the last Y of the one before.  Same route, same bounds against the oracle, and within them of the default run."""
    case = wc.BY_NAME[name]
    default = _default_run(name)
    assert default["routes"][0].n_chain > mc.pkg().flags.CHAIN_MAX
    with wc.flags_set(CHAIN_MAX=3):
        got = _run(case, False)
    assert got["routes"] == default["routes"]
    bad = _check(f"{name} CHAIN_MAX=3, against the oracle", case, got, mc.reference(case), False)
    bad += _check(f"{name} CHAIN_MAX=3 against the default run", case, got, {k: default[k] for k in ("out", "grads")}, False, oracle=False)
    assert not bad, bad


@pytest.mark.parametrize("flag", ["CHAIN_HEAD", "CHAIN_HEAD_FWD"])
@pytest.mark.parametrize("name", wc.HEAD_CASES)
def test_heads_in_launches_of_their_own(name, flag):
    """flags.CHAIN_HEAD = False takes the head out of both chains, flags.CHAIN_HEAD_FWD = False out of the forward chain: the narrow layer
    and its weight gradient run in launches of their own, at a width off the grids.  Nothing else of the route moves."""
    case = wc.BY_NAME[name]
    default = _default_run(name)
    with wc.flags_set(**{flag: False}):
        got = _run(case, False)
    assert got["routes"][0] == default["routes"][0]._replace(**wc.heads_apart(flag))
    assert not got["routes"][0].head and got["routes"][0].bwd_head == (flag == "CHAIN_HEAD_FWD")
    bad = _check(f"{name} {flag} off", case, got, mc.reference(case), False)
    assert not bad, bad
