"""CPU: every case of tests/lanegroup_cases.py is fit to be held to the plain floors on the GPU.

Conditioning: 4 x the error of the fp32 restatement against the fp64 one, for the output, every parameter gradient and the input
gradient, lies under that quantity's bound (1e-5; max(1e-4, 8 / N), and 1e-4 at the small ends), so tests/test_gpu_lanegroup_shapes.py never needs a widened
bound.  Kink margin: with ReLU / LeakyReLU no input of the model's nonlinearity lies within 1e-5 of zero in fp64.  (The gates
inside a conv, GINE's message ReLU and GATv2's score LeakyReLU, open per edge and channel; one that falls the other way moves a
gradient by one edge's share, which is what the 8 / N of the floor and the fp32 run above cover.)  A case that misses either
condition gets another seed in lanegroup_cases.SEEDS, never a wider bound.  Geometry: the slab-cap cases really are capped, with
unequal trip counts, and the small ends have the rows and trips their names say.  The restatement equals the oracle modules' own
model wiring bit for bit, and the package builds each case's model with the table's state_dict keys."""
import os
import re

import pytest
import torch

import lanegroup_cases as lc
from conftest import PKG_NAME, ROOT, rel_err


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_case_is_well_conditioned_and_away_from_kinks(case):
    r64, r32 = lc.oracle_run(case, torch.float64, with_pre=True), lc.oracle_run(case, torch.float32)
    n = lc.structure(case.struct)[1]
    tol = lc.grad_bound(case, n)
    assert torch.isfinite(r64["out"]).all() and r64["out"].abs().max() > 1e-3
    errs = {"out": (rel_err(r32["out"], r64["out"]), lc.OUT_FLOOR), "dx": (rel_err(r32["dx"], r64["dx"]), tol)}
    for k, g in r64["grads"].items():
        if g is None:        # a parameter the model does not use (the shared nn of a GINE model without convs)
            assert r32["grads"][k] is None
            continue
        errs[k] = (rel_err(r32["grads"][k], g), tol)
    worst = max(errs, key=lambda k: errs[k][0] / errs[k][1])
    print(f"[lanegroup cases] {case.id}: fp32 out {errs['out'][0]:.2e}, worst {worst} {errs[worst][0]:.2e} (floor {errs[worst][1]:.2e})")
    for k, (e, floor) in errs.items():
        assert 4 * e < floor, (case.id, k, e, floor)
    if case.nonlin in ("relu", "leaky_relu") and r64["pre"]:
        margin = min(z.abs().min().item() for z in r64["pre"])
        assert margin > lc.KINK_MARGIN, (case.id, margin)


@pytest.mark.parametrize("case", [c for c in lc.CASES if c.struct in ("mixed16", "n33")], ids=lambda c: c.id)
def test_restatement_equals_the_oracles_own_wiring_and_the_model_takes_the_keys(case):
    x, ei, ea = lc.inputs(case)
    sd = lc.state_dict(case)
    want = lc.existing_oracle(case, sd, x, ei, ea)
    if want is not None:
        ref = lc.gine_oracle.unique_params(sd) if case.family == "gine" else sd
        assert torch.equal(lc.restate(case, ref, x, ei, ea), want)
    m = lc.build_model(case)        # strict load: the table's keys are the model's
    spec = lc.spec_of(case, m)
    assert spec.group == case.group and spec.x_cols == case.in_width
    named = [k for k, _ in m.named_parameters()]
    assert sorted(named) == sorted(k for k, v in lc.leaves(case, sd, torch.float64).items() if v.requires_grad)


def test_the_table_covers_what_it_claims():
    fams = set(lc.FAMILIES)
    for dims in lc.WIDTHS:
        assert {c.family for c in lc.WIDTH_CASES if c.dims == dims and not c.chain} == fams, dims
    for g in (8, 16, 32):       # every kernel instantiation: a width case with convs and a head, and a slab-cap case
        for fam in lc.FAMILIES:
            assert any(c.family == fam and c.group == g and c.num_layers > 1 for c in lc.WIDTH_CASES), (fam, g)
        for kernel in (("gat",), ("gine",), lc.GNN_KINDS):
            assert any(c.family in kernel and c.group == g and c.num_layers > 1 for c in lc.CAP_CASES), (kernel, g)
        assert any(c.struct == "cap_hub" and c.group == g for c in lc.CAP_CASES), g
    assert {c.nonlin for c in lc.WIDTH_CASES} == set(lc.NONLINS)
    assert {c.num_layers for c in lc.WIDTH_CASES} >= {1, 2, 5}
    assert any(c.num_layers == 1 and c.group == 32 for c in lc.WIDTH_CASES)
    assert {c.edge_dim for c in lc.WIDTH_CASES if c.family == "gat"} == {None, 3, 6, 16}
    assert {c.edge_dim for c in lc.WIDTH_CASES if c.family == "gine"} == {None, 6, 16}
    opt = lambda fam, **kv: [c for c in lc.WIDTH_CASES if c.family == fam and c.num_layers > 1 and all(c.opt.get(k) == v for k, v in kv.items())]  # noqa: E731
    assert any(c.dims[0] == 32 for c in opt("gcn2", shared_weights=False))
    assert any(c.dims[0] == 32 for c in opt("tagcn", K=4)) and any(c.dims[0] == 32 for c in opt("tagcn", K=0))
    assert any(c.dims[0] == 12 for c in opt("tagcn", bias=False))
    assert any(c.dims[0] == 17 for c in opt("fagcn", main_param=0.0, add_self_loops=False))
    assert any(c.chain == (5, 12, 20, 7) and c.dims == (7, 9, 4) for c in lc.WIDTH_CASES)


@pytest.mark.parametrize("case", lc.CAP_CASES, ids=lambda c: c.id)
def test_slab_cap_cases_are_capped_with_unequal_trips(case):
    n = lc.structure(case.struct)[1]
    spec = lc.spec_of(case, lc.build_model(case))
    assert spec.n_slabs == lc.pkg().lanegroup._MAX_SLABS == lc.MAX_SLABS == 256
    assert n > lc.MAX_SLABS * (lc.NT // spec.group) and spec.group == case.group
    t = lc.trips(n, spec.group, spec.n_slabs)
    assert min(t) >= 2 and len(set(t)) > 1, (min(t), max(t))
    assert (min(t), max(t)) == {8: (2, 3), 16: (4, 5), 32: (8, 9)}[spec.group]


def test_small_ends_have_the_rows_and_trips_their_names_say():
    by = {(c.struct, c.family): c for c in lc.SMALL_CASES}
    geo = {}
    for (struct, fam), case in by.items():
        spec = lc.spec_of(case, lc.build_model(case))
        n = lc.structure(struct)[1]
        geo.setdefault(struct, set()).add((n, spec.group, spec.n_slabs, tuple(lc.trips(n, spec.group, spec.n_slabs))))
    assert geo["n1"] == {(1, 8, 1, (1,))} and lc.structure("n1")[0].size(1) == 0
    assert geo["n3"] == {(3, 16, 1, (1,))}                          # one partial lane-group row, one slab
    assert geo["n33"] == {(33, 8, 2, (1, 1))}                       # two slabs, the second with one node
    assert geo["n2049"] == {(2049, 32, 256, (2,) + (1,) * 255)}     # one node in the second trip of workgroup 0 only


def test_the_table_knows_the_kernels_workgroup_size_and_slab_cap():
    with open(os.path.join(ROOT, PKG_NAME, "csrc", "dss2_lanegroup.hpp")) as fh:
        nt = re.search(r"constexpr int [^;]*\bNT = (\d+)", fh.read())
    assert nt and int(nt.group(1)) == lc.NT
    assert lc.pkg().lanegroup._MAX_SLABS == lc.MAX_SLABS
