"""CPU: every case of tests/mpn_width_cases.py is what its table says, so that tests/test_gpu_mpn_widths.py can hold it to the plain
bounds on the GPU.

Structure: the case's graphs are its base case's, with the base's pinned STRUCTURE.  Route: route.block_route, the whole-stack query, the
weight-gradient plan, the edge plan and the chain records (dss2_gemm_prop_chain_plan, both directions) on the stand-in topology equal the
pinned literals, with and without an input gradient; so does what each flag of the format reruns moves.  Coverage: over the table, every
chain family, row split 2, 8 waves, every remainder of hid and of the padded K, the head widths, K and depths the table claims.
Conditioning: 4 x the error of the oracle model in fp32 against the same model in fp64 lies under the GPU bound (1e-5 for the output, 1e-4
for dx and every parameter gradient), also on the last column group alone, normalised by its own maximum; that slice is within a factor
100 of its tensor's maximum, so the slice check of the GPU test is no weaker than the whole-tensor one by more than that."""
import pytest
import torch

import mpn_shape_cases as mc
import mpn_width_cases as wc
from conftest import rel_err

IDS = [c.name for c in wc.ALL_CASES]


@pytest.mark.parametrize("case", wc.ALL_CASES, ids=IDS)
def test_structure_is_the_base_cases(case):
    base = mc.BY_NAME[wc.BASE[case.name]]
    assert mc.graph_key(case) == mc.graph_key(base) and case.full == base.full
    got = mc.structure(case)
    print(f"[mpn widths] {case.name}: graphs of {base.name}, (nrb, ntiles, ell, ellT, max_segment, min degree) = {got}; {case.purpose}")
    assert got == mc.STRUCTURE[base.name]
    b, bb = mc.batch(case), mc.batch(base)
    assert b["x"] is bb["x"] and b["edge_index"] is bb["edge_index"] and b["edge_attr"] is bb["edge_attr"]      # the same graphs and features
    assert b["gout"].shape == (sum(case.counts), case.args[2]) and b["gout"].dtype == torch.float64
    assert mc.topology_oracle(case) is mc.topology_oracle(base)


@pytest.mark.parametrize("need_dx", [False, True], ids=["no_dx", "dx"])
@pytest.mark.parametrize("case", wc.ALL_CASES, ids=IDS)
def test_route_is_the_pinned_one(case, need_dx):
    got = wc.route_literal(case, need_dx)
    stack, rows, wg, edge, chains = got
    print(f"[mpn widths] {case.name} need_dx={need_dx}: stack {stack}, wgrad (tile rows, kernel) {wg}, edge families {edge}")
    for bi, (row, (pf, pb)) in enumerate(zip(rows, chains)):
        print(f"    block {bi}: " + ", ".join(f"{f}={v}" for f, v in zip(mc.ROUTE_FIELDS, row)))
        print(f"    block {bi}: chain record forward {pf}, transposed {pb}")
    assert got == wc.ROUTE[case.name][need_dx]


@pytest.mark.parametrize("variant", list(wc.VARIANT_FLAGS))
@pytest.mark.parametrize("name", wc.VARIANT_CASES)
def test_format_reruns_move_what_is_pinned(name, variant):
    got = wc.variant_literal(wc.BY_NAME[name], variant)
    print(f"[mpn widths] {name} {variant}: route fields moved {got[0]}, wgrad {got[1]}, edge families {got[2]}")
    assert got == wc.VARIANTS[name][variant]
    FL = mc.pkg().flags
    assert all(getattr(FL, f) is True for f in wc.VARIANT_FLAGS[variant])      # (restored)


@pytest.mark.parametrize("flag", ["CHAIN_HEAD", "CHAIN_HEAD_FWD"])
@pytest.mark.parametrize("name", wc.HEAD_CASES)
def test_head_flags_clear_the_head_fields_only(name, flag):
    P, case = mc.pkg(), wc.BY_NAME[name]
    args = (mc.blocks_of(case)[0], mc.stub_topology(case).tiling, False, False)
    default = P.route.block_route(*args)
    with wc.flags_set(**{flag: False}):
        apart = P.route.block_route(*args)
    assert default.bwd_head and apart == default._replace(**wc.heads_apart(flag))
    assert getattr(P.flags, flag) is True


def test_chain_max_lowered_keeps_the_deep_routes():
    P = mc.pkg()
    for name in wc.SPLIT_CASES:
        case = wc.BY_NAME[name]
        args = (mc.blocks_of(case)[0], mc.stub_topology(case).tiling, False, False)
        default = P.route.block_route(*args)
        with wc.flags_set(CHAIN_MAX=3):
            assert P.route.block_route(*args) == default
    assert P.flags.CHAIN_MAX == 8


def _row(name, need_dx=False, block=0):
    return dict(zip(mc.ROUTE_FIELDS, wc.ROUTE[name][need_dx][1][block]))


def _default_kernel(name, transposed=False, block=0):
    """(family, row_split, waves) of the chain a case runs by default in one direction, None without a chain."""
    r = _row(name, block=block)
    if not (r["bwd_chain"] if transposed else r["n_chain"]):
        return None
    fmts = wc.ROUTE[name][False][4][block][int(transposed)][0]
    return fmts[(2 if r["f16"] else 1) if r["use16"] else 0]


def test_the_table_covers_what_it_claims():
    names = [c.name for c in wc.CASES]
    D = {c.name: wc.dims(c) for c in wc.CASES}      # name -> (nout, hid, L, nmat)
    kernels = {n: _default_kernel(n) for n in names}
    for n in names:      # both directions run the same kernel wherever both are chained
        assert _default_kernel(n, True) == kernels[n] or kernels[n] is None
    by_family = {}
    for n, k in kernels.items():
        if k is not None:
            by_family.setdefault(k[0], []).append(n)
    # every chain family is some case's DEFAULT route
    assert by_family[wc.FP32] == ["t96_w136_fp32"]
    assert {"w36_rs2", "w44_k1", "w40_k3", "d10_split", "t32_w200"} <= set(by_family[wc.BF16X6])
    assert {"w72_head", "w100_out3", "w136_w8", "w252", "w160_out5", "c2g_w96"} <= set(by_family[wc.SP])
    assert {"t96_w44", "t96_w100_out4_k1", "t96_d11", "t192_w72_out1"} <= set(by_family[wc.SP6])
    assert {k[1] for k in kernels.values() if k} == {1, 2}                                   # row split 2
    assert {k[2] for k in kernels.values() if k} >= {2, 3, 4, 8}                             # waves, 8 among them
    assert {k[2] for n, k in kernels.items() if k and k[0] == wc.SP6} == {2, 3, 4}
    assert {D[n][1] for n in by_family[wc.BF16X6] if kernels[n][1] == 2} >= {36, 40, 44}
    # both 16-bit formats of the split-plane forms, with and without the fused heads
    assert {_row(n)["f16"] for n in by_family[wc.SP]} == {False, True} and {_row(n)["head"] for n in by_family[wc.SP]} == {False, True}
    assert {(_row(n)["bwd_head"], _row(n)["bwd_head_wgrad"]) for n in by_family[wc.SP6]} == {(False, False), (True, False), (True, True)}
    # the partly filled last column group and the padded K
    chained = [n for n in names if kernels[n] is not None]
    assert {D[n][1] % 32 for n in chained} >= {4, 8, 12}
    assert {wc.kpad16(D[n][1]) - D[n][1] for n in chained if _row(n)["use16"]} >= {4, 8, 12}
    assert {D[n][0] for n in names} >= {1, 3, 4, 5, 11}                                     # nout
    assert {D[n][3] for n in chained} == {2, 3, 4}                                          # nmat
    CHAIN_MAX = mc.pkg().flags.CHAIN_MAX
    assert CHAIN_MAX == 8
    deep = {n: _row(n)["n_chain"] for n in names if _row(n)["n_chain"] > CHAIN_MAX}
    assert deep == {"d10_split": 9, "t96_d11": 10}
    for n in deep:      # ... and the heads and the joined folded layer dropped there
        assert not _row(n)["head"] and not _row(n)["bwd_head"]
        assert not mc.pkg().route.block_route(mc.blocks_of(wc.BY_NAME[n])[0], mc.stub_topology(wc.BY_NAME[n]).tiling, False, False).bwd_join
    # no chain, for each of the two reasons chain_select has besides the tiles: above 256, hid % 4 != 0
    nochain = {n: D[n][1] for n in names if kernels[n] is None and not _row(n)["bwd_chain"]}
    assert nochain == {"w260_nochain": 260, "w70_scalar": 70}
    assert all(f == (wc.NONE, 0, 0) for n in nochain for p in wc.ROUTE[n][False][4][0] for f in p[0])
    # heads: fused for nout 1 .. 4 with the weight gradient up to 2; nout 5 still narrow, 11 not
    is_narrow = mc.pkg().ops.is_narrow
    assert is_narrow(3, 5) and not is_narrow(3, 11)
    for n in wc.HEAD_CASES:
        r = _row(n)
        assert r["bwd_head"] and r["bwd_head_wgrad"] == (D[n][0] <= 2), n
    assert {n for n in names if _row(n)["head"] or _row(n)["bwd_head"]} == set(wc.HEAD_CASES) | {"w136_w8", "t96_w44"}
    # the tile heights and the weight-gradient kernels behind the chains
    assert {mc.STRUCTURE[wc.BASE[n]][0] for n in names} == {1, 2, 3, 6}
    assert {wc.ROUTE[n][False][2] for n in names} == {(64, wc.WG_BF16_64), (64, wc.WG_FP32), (96, wc.WG_F16_TALL), (192, wc.WG_F16_TALL), (32, wc.WG_F16_32)}
    assert wc.ROUTE["w260_nochain"][False][3] == (0, 0, 0)
    # the stack: declined, the blocks chained
    assert not wc.ROUTE["stack_w40"][False][0] and not wc.ROUTE["stack_w40"][True][0]
    assert mc.ROUTE["stack_full64_ell4"][False][0]                                         # (its graphs at hid 32: taken)
    assert [r[1] for r in wc.ROUTE["stack_w40"][True][1]] == [2, 2]
    # the reruns reach what they are there for
    V = wc.VARIANTS
    assert V["w36_rs2"]["chain_bf16_off"][0]["use16"] is False and "n_chain" not in V["w36_rs2"]["chain_bf16_off"][0]      # the fp32 chain, row split 2
    assert wc.ROUTE["w36_rs2"][False][4][0][0][0][0] == (wc.FP32, 2, 4)
    assert V["t192_w72_out1"]["chain_bf16_off"][0]["n_chain"] == 0                                                            # no fp32 chain there
    assert all(V[n]["chain_layers_off"][0]["n_chain"] == 0 and not V[n]["chain_layers_off"][0]["bwd_chain"] for n in wc.VARIANT_CASES)
    assert {V[n]["wgrad_f16_off"][1][1] for n in wc.VARIANT_CASES} == {wc.WG_BF16_64, wc.WG_BF16_TALL}
    assert {V[n]["wgrad_bf16_off"][1][1] for n in wc.VARIANT_CASES} == {wc.WG_FP32, wc.WG_NONE}


def test_the_literals_match_the_package_constants():
    P = mc.pkg()
    assert (wc.NONE, wc.FP32, wc.BF16X6, wc.SP, wc.SP6) == (P._lib.CHAIN_NONE, P._lib.CHAIN_FP32, P._lib.CHAIN_BF16X6, P._lib.CHAIN_SP, P._lib.CHAIN_SP6)
    assert (wc.WG_NONE, wc.WG_BF16_TALL) == (P._lib.WGRAD_NONE, P._lib.WGRAD_BF16_TALL)
    assert set(wc.CHAIN_FIELDS) | {"gate_words", "head_modes", "head_wgrad"} <= {f for f, _ in P._lib.ChainKernel._fields_}
    for case in wc.ALL_CASES:       # the package builds each case's model with the oracle model's state_dict keys (strict load)
        m = mc.build_model(case)
        assert [k for k, _ in m.named_parameters()] == [k for k, _ in mc.oracle_model(case).named_parameters()]
        blocks = list(m.mpns) if hasattr(m, "mpns") else [m]      # the fused block, or (above 256) the per-layer nodes
        assert all(b.edge_aggr.fused_dims() == (case.name not in wc.GENERAL_PATH) for b in blocks), case.name
    assert [wc.dims(wc.BY_NAME[n])[1] for n in wc.GENERAL_PATH] == [260]


def _slice_err(got, want):
    return (got.double() - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


@pytest.mark.parametrize("case", wc.ALL_CASES, ids=IDS)
def test_case_is_well_conditioned(case):
    r64, r32 = mc.reference(case), mc.oracle_run(case, torch.float32)
    assert torch.isfinite(r64["out"]).all() and r64["out"].abs().max() > 1e-3
    errs = {"out": (rel_err(r32["out"], r64["out"]), mc.OUT_BOUND), "dx": (rel_err(r32["dx"], r64["dx"]), mc.GRAD_BOUND)}
    assert r64["dx"].abs().max() > 0
    for k, g in r64["grads"].items():
        assert g is not None and g.abs().max() > 0, k
        errs[k] = (rel_err(r32["grads"][k], g), mc.GRAD_BOUND)
        for (label, s64), (_, s32) in zip(wc.hid_slices(case, k, g), wc.hid_slices(case, k, r32["grads"][k])):
            errs[label] = (_slice_err(s32, s64), mc.GRAD_BOUND)
    worst = max((k for k in errs if k != "out"), key=lambda k: errs[k][0])
    print(f"[mpn widths] {case.name}: fp32 out {errs['out'][0]:.2e} (bound {mc.OUT_BOUND:.0e}), worst gradient {worst} {errs[worst][0]:.2e} "
          f"(bound {mc.GRAD_BOUND:.0e})")
    for k, (e, bound) in errs.items():
        assert 4 * e < bound, (case.name, k, e, bound)


@pytest.mark.parametrize("case", wc.ALL_CASES, ids=IDS)
def test_the_last_column_group_is_not_degenerate(case):
    hid = wc.dims(case)[1]
    c0 = wc.last_group(hid)
    r64 = mc.reference(case)
    if c0 is None:
        assert all(not wc.hid_slices(case, k, g) for k, g in r64["grads"].items())
        return
    assert 0 < hid - c0 < 32
    seen, smallest = 0, (None, float("inf"))
    for k, g in r64["grads"].items():
        slices = wc.hid_slices(case, k, g)
        assert len(slices) == sum(1 for n in g.shape if n == hid)
        for label, s in slices:
            assert s.numel() == g.numel() // hid * (hid - c0)
            ratio = s.abs().max().item() / g.abs().max().item()
            smallest = min(smallest, (label, ratio), key=lambda t: t[1])
            assert ratio > 1e-2, (case.name, label, ratio)
            seen += 1
    # every tensor with a hid-sized axis: both edge-MLP Linears (weight, bias; the second's weight on both axes), every hid -> hid conv
    # (bias, K + 1 weights on both axes) and the head's weights -- per block
    nout, _, L, nmat = wc.dims(case)
    blocks = len(mc.blocks_of(case))
    assert seen == blocks * (1 + 1 + 2 + 1 + (L - 1) * (1 + 2 * nmat) + nmat)
    print(f"[mpn widths] {case.name}: columns {c0} .. {hid - 1}, {seen} slices, the smallest against its tensor's maximum: {smallest[0]} {smallest[1]:.2f}")


def test_pad_sensitive_cases_are_the_ones_off_the_grids():
    assert {c.name for c in wc.ALL_CASES if not wc.pad_sensitive(c)} == {"w160_out5", "out11_wide_head", "d10_split", "t96_d11", "c2g_w96"}
    assert wc.kpad16(36) == 48 and wc.kpad16(252) == 256 and wc.kpad16(96) == 96 and wc.last_group(100) == 96 and wc.last_group(96) is None
