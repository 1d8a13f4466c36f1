"""CPU: every case of tests/mpn_shape_cases.py is what its table says, so that tests/test_gpu_mpn_shapes.py can hold it to the plain
bounds on the GPU.

Structure: the topology oracle's (nrb, ntiles, ell, ellT, max_segment, min degree) equals the pinned literal.  Route: route.block_route,
the whole-stack query, the weight-gradient plan and the edge plan on a stand-in topology built from the oracle's arrays equal the pinned
literals, with and without an input gradient, and every case's route says what the case is there for.  Conditioning: 4 x the error of the
oracle model in fp32 against the same model in fp64 lies under the GPU bound (1e-5 for the output, 1e-4 for dx and every parameter
gradient); a case that misses gets another seed, never a wider bound.  Placement: the capped nodes sit where the table says, read off
the edge list and tile_start."""
import pytest
import torch

import mpn_shape_cases as mc
from conftest import rel_err

IDS = [c.name for c in mc.CASES]


@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_structure_is_the_pinned_one(case):
    got = mc.structure(case.name)
    print(f"[mpn shapes] {case.name}: (nrb, ntiles, ell, ellT, max_segment, min degree) = {got}; {case.purpose}")
    assert got == mc.STRUCTURE[case.name]
    b = mc.batch(case.name)
    assert b["x"].size(0) == sum(case.counts) and b["x"].dtype == torch.float64
    # one direction per branch: the reference's first-edge rule calls the batch directed, the model doubles it
    o = mc.topology_oracle(case.name)
    assert o.directed and o.E2 == 2 * b["edge_index"].size(1)
    # every graph is one connected segment of the tiling (a one-node graph too)
    assert [int(v) for v in o.bounds] == list(b["start"]) + [sum(case.counts)]


@pytest.mark.parametrize("need_dx", [False, True], ids=["no_dx", "dx"])
@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_route_is_the_pinned_one(case, need_dx):
    got = mc.route_literal(case, need_dx)
    stack, rows, wg, edge = got
    print(f"[mpn shapes] {case.name} need_dx={need_dx}: stack {stack}, wgrad (tile rows, kernel) {wg}, edge families {edge}")
    for bi, row in enumerate(rows):
        print(f"    block {bi}: " + ", ".join(f"{f}={v}" for f, v in zip(mc.ROUTE_FIELDS, row)))
    assert got == mc.ROUTE[case.name][need_dx]


def _row(name, need_dx, block=0):
    return dict(zip(mc.ROUTE_FIELDS, mc.ROUTE[name][need_dx][1][block]))


def test_the_pinned_routes_say_what_the_cases_are_there_for():
    R, S = mc.ROUTE, mc.STRUCTURE
    fused = dict(f16=True, n_chain=3, use16=True, gw=128, head=True, edge=True, bwd_chain=True, bwd_head=True, bwd_head_wgrad=True,
                 bwd_edge=True, glob=False)
    assert _row("full64_ell5", False) == fused and S["full64_ell5"][:4] == (2, 3, 5, 5)
    assert _row("parallel_ell8", False) == fused
    r = _row("c2_ell8_head_edge", False)        # the pairing no grid produces
    assert (r["head"], r["edge"], r["bwd_edge"]) == (True, False, True) and S["c2_ell8_head_edge"][:4] == (2, 23, 8, 8)
    for name in ("full64_ell5", "c2_ell8_head_edge", "parallel_ell8"):      # an input gradient takes the edge phases out of both chains
        r = _row(name, True)
        assert not r["edge"] and not r["bwd_edge"] and r["head"] and r["bwd_head"]
    for name, nrb, gw in (("n65_ell6", 3, 256), ("full96_ell8", 3, 256), ("full192_ell8", 6, 384)):     # the tall chains
        r = _row(name, False)
        assert S[name][0] == nrb and (r["n_chain"], r["f16"], r["gw"], r["head"], r["bwd_head"]) == (3, True, gw, False, True)
    assert S["ragged_ell7"][5] == 0 and mc.stub_topology("ragged_ell7").tiling.max_tile_rows == 0
    assert S["full128_ell6"][0] == 4 and _row("full128_ell6", False)["n_chain"] == 0 and not _row("full128_ell6", False)["bwd_chain"]
    r = _row("nrb1_ell8", False)
    assert S["nrb1_ell8"][0] == 1 and (r["n_chain"], r["use16"], r["f16"], r["gw"]) == (3, True, False, 0)
    assert R["nrb1_ell8"][False][2] == (32, mc.WG_F16_32)
    assert S["pairs_ell1"][2:4] == (1, 1)
    assert S["csr9"][2:4] == (0, 0) and R["csr9"][True][3] == (mc.E_CSR,) * 3 and not _row("csr9", False)["glob"]
    assert mc.degrees("csr9").max() == 9
    assert 4 < S["parallel_ell8"][2] <= 8
    # the whole-stack kernels: taken at ELL 4, declined at 5
    assert R["stack_full64_ell4"][False][0] and R["stack_full64_ell4"][True][0] and S["stack_full64_ell4"][5] == 0
    assert not R["stack_ell5"][False][0] and not R["stack_ell5"][True][0] and S["stack_ell5"][2] == 5
    assert not R["pfn_ell8_96"][False][0] and S["pfn_ell8_96"][0] == 3
    assert {S[c.name][0] for c in mc.CASES} == {1, 2, 3, 4, 6}          # every tile height is some case's primary tiling
    assert {S[c.name][2] for c in mc.CASES} == {0, 1, 4, 5, 6, 7, 8}    # ELL widths (0: CSR staging); 3 and 4 are the grids'


@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_case_is_well_conditioned(case):
    r64, r32 = mc.reference(case.name), mc.oracle_run(case, torch.float32)
    assert torch.isfinite(r64["out"]).all() and r64["out"].abs().max() > 1e-3
    errs = {"out": (rel_err(r32["out"], r64["out"]), mc.OUT_BOUND), "dx": (rel_err(r32["dx"], r64["dx"]), mc.GRAD_BOUND)}
    for k, g in r64["grads"].items():
        assert g is not None and g.abs().max() > 0, k
        errs[k] = (rel_err(r32["grads"][k], g), mc.GRAD_BOUND)
    worst = max((k for k in errs if k != "out"), key=lambda k: errs[k][0])
    print(f"[mpn shapes] {case.name}: fp32 out {errs['out'][0]:.2e} (bound {mc.OUT_BOUND:.0e}), worst gradient {worst} {errs[worst][0]:.2e} "
          f"(bound {mc.GRAD_BOUND:.0e})")
    for k, (e, bound) in errs.items():
        assert 4 * e < bound, (case.name, k, e, bound)


@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_capped_nodes_sit_where_the_table_says(case):
    b = mc.batch(case.name)
    ei, o = b["edge_index"], mc.topology_oracle(case.name)
    ts, tm = o.tile_start.tolist(), 32 * o.nrb
    deg = mc.degrees(case.name)
    nbrs = lambda v: set(ei[1, ei[0] == v].tolist()) | set(ei[0, ei[1] == v].tolist())      # noqa: E731
    last_rows, mid = [], 0
    for k, (n, hub, start) in enumerate(zip(case.counts, b["hubs"], b["start"])):
        distinct = len(nbrs(hub))
        assert distinct == min(case.cap, n - 1), (k, distinct)            # exactly the cap (a branch listed twice is one neighbour)
        assert deg[start:start + n].max() <= case.cap * (2 if case.dup3 else 1)
        tile = max(t for t in range(o.ntiles) if ts[t] <= hub)
        row = hub - ts[tile]
        if k in case.tail:
            assert hub == start + n - 1 and start in nbrs(hub)
            if row == tm - 1:                                             # the graph fills its tile: last row, with row 0 a neighbour
                assert start == ts[tile]
                last_rows.append(row)
        elif 0 < row < ts[tile + 1] - ts[tile] - 1:
            mid += 1
    if case.full:
        assert last_rows and set(last_rows) == {tm - 1} and tm - 1 in (31, 63, 95, 127, 191)
        assert mid >= 1
    if not case.dup3:
        assert int(deg.max()) == min(case.cap, max(case.counts) - 1)
    # a branch is stored once, in one direction (parallel_ell8: or twice in the same direction)
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    assert not set(pairs) & {(b_, a_) for a_, b_ in pairs}
    assert (len(pairs) > len(set(pairs))) == case.dup3


def test_the_cases_that_fill_a_tile_cover_every_last_row():
    rows = {32 * mc.STRUCTURE[c.name][0] - 1 for c in mc.CASES if c.full}
    assert rows == {63, 95, 127, 191}      # (no graph can fill a 32-row tile of a case that also needs ELL 8 on 15 nodes: nrb 1 is covered unfilled)


def test_the_stand_in_topology_matches_the_package_constants():
    P = mc.pkg()
    assert P.topology._ELL_MAX == 8 and tuple(P.topology._NRB_CHOICES) == (2, 4, 3, 1, 6)
    assert (mc.WG_FP32, mc.WG_BF16_64, mc.WG_F16_32, mc.WG_F16_TALL, mc.WG_F16_TALL_PAIR) == \
        (P._lib.WGRAD_FP32, P._lib.WGRAD_BF16_64, P._lib.WGRAD_F16_32, P._lib.WGRAD_F16_TALL, P._lib.WGRAD_F16_TALL_PAIR)
    assert (mc.E_CSR, mc.E_VALU, mc.E_VALU_HALF, mc.E_BF16X6) == (P._lib.EDGE_CSR, P._lib.EDGE_VALU, P._lib.EDGE_VALU_HALF, P._lib.EDGE_BF16X6)
    for case in mc.CASES:       # the package builds each case's model with the oracle model's state_dict keys (strict load)
        m = mc.build_model(case)
        assert [k for k, _ in m.named_parameters()] == [k for k, _ in mc.oracle_model(case).named_parameters()]


@pytest.mark.parametrize("case", [c for c in mc.CASES if c.full], ids=[c.name for c in mc.CASES if c.full])
def test_a_dropped_last_slot_of_the_last_row_would_show(case):
    """What the placement is for: the oracle model without the LAST ELL entry of a tile's last row (the capped node's in-edge of the
    highest directed id) moves the output by more than 100 x the GPU bound, so a kernel that drops that slot or that row cannot pass."""
    b = mc.batch(case.name)
    o = mc.topology_oracle(case.name)
    ts, tm = o.tile_start.tolist(), 32 * o.nrb
    hub = next(h for k, h in enumerate(b["hubs"]) if k in case.tail and (h + 1) in ts and (h + 1 - tm) in ts)
    ei2, ea2 = mc.dss2_oracle.undirect_graph(b["edge_index"], b["edge_attr"])
    drop = int((ei2[1] == hub).nonzero().max())
    slot = int(o.rowptr[hub + 1] - o.rowptr[hub]) - 1
    assert slot == o.ell - 1 or case.dup3           # the widest row of the batch (parallel_ell8: 4 neighbours, some twice; another row is wider)
    assert int(o.ell_ent_tiles[ts.index(hub + 1) - 1, slot, tm - 1, 1]) == o.ent[o.rowptr[hub + 1] - 1]       # the row's last slot is in use ...
    assert int(o.perm[o.rowptr[hub + 1] - 1]) == drop                                                               # ... by that entry
    keep = torch.ones(ei2.size(1), dtype=torch.bool)
    keep[drop] = False
    ei3, ea3 = ei2[:, keep], ea2[keep]
    assert not mc.dss2_oracle.is_directed(ei3)      # taken as it is, not doubled again
    with torch.no_grad():
        out = mc.oracle_model(case)(b["x"], ei3, ea3)
    moved = rel_err(out, mc.reference(case.name)["out"])
    print(f"[mpn shapes] {case.name}: without the last slot of row {hub} the output moves by {moved:.2e}")
    assert moved > 100 * mc.OUT_BOUND
