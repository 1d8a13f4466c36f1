"""GPU: estimator.wls_bad_data_banded and estimator.wls_robust_banded -- bad-data detection and the Huber form on the banded kernel
(csrc/dss2_wls_bad_data.hip's wls_bad_data_banded_kernel with csrc/dss2_wls_banded_invert.hpp's selected inverse;
csrc/dss2_wls_banded.hpp's kernel on dss2_wls_robust_args) -- against the fp64 oracles of tests/wls_bad_data_oracle.py and
tests/wls_robust_oracle.py on the batches of tests/wls_banded_cases.py.

Every bound, and every list of graphs whose removals are compared, comes from tests/test_wls_banded_bad_data_cpu.py, which measures them
in the oracles alone (never from the kernel), at tol = 0 and 8 iterations per solve:
  bus_sens, edge_sens   cpu.bounds(name)[0]: 2e-7 absolute on n257, n320, ober70, star41, path12 (tests/test_gpu_wls_bad_data.py's floor);
                        1.2e-6 .. 3.0e-6 on radial300 (8 x the fp64 routes' own spread, which moves with the host BLAS: 1.5e-7 .. 3.7e-7)
  rN, removed_rn        the S bound at the floor, sens / (2 s_min), in units of max(rN, 1), where the oracle's S >= 2 s_min: 1e-3 at
                        s_min = 1e-4 (5.9e-3 on radial300), a tenth of it at the default s_min; measurements with S inside
                        [s_min / 2, 2 s_min] are left out (at most 10 %: 3.4 %, 2.1 %, 1.9 % on the three; the CPU file asserts it)
  state_std             cpu.bounds(name)[1]: 3.44e-9, on radial300 1.1e-7 .. 1.6e-7
  dof, suspect, iterations, status   equal;  chi2_limit 1e-12 relative
  state                 wls_large_cases.state_bound(the oracle's spread over summation orders): 5e-7
  Huber                 state 5e-7, q 1e-9, cost 1e-6 relative (tests/test_gpu_wls_robust.py's floors; 8 x the oracle's spread stays below)
Removals are compared on the graphs the CPU file lists as CLEAR (every removal leads its runner-up by 1 % in the oracle): all with one
error; with three, n257 graph 0, n320 both, radial300 graph 1.  Against wls_bad_data_large on sizes both forms serve: twice the bounds.

What must hold to the bit: with max_removals = 0 the five solve fields against wls_estimate_banded; gamma = inf against
wls_estimate_banded; two runs; max_groups = 1 against the default; a graph alone against the same graph inside a batch; a hipGraph
replay and a launch-plan replay against the eager call with a given `order`, also after the static inputs were overwritten; the graphs
beside one that does not fit its declared band.  Every test prints its errors beside the bounds (-s).
"""
import ctypes as C
import functools
import importlib
import math

import pytest
import torch

import test_wls_bad_data_large_cpu as cpu_large
import test_wls_banded_bad_data_cpu as cpu
import wls_bad_data_oracle as bo
import wls_banded_cases as bc
import wls_cases as wc
import wls_large_cases as lc
import wls_robust_oracle as ro
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXED = cpu.FIXED
SOLVE_FIELDS = ("state", "objective", "iterations", "status", "last_step")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


def _to_device(b):
    return {k: (tuple(s.to(DEV) for s in v) if k == "stats" else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _device(name):
    return _to_device(bc.batch(name))


def _order(pkg, b, **kw):
    return pkg.estimator.band_order(b["edge_index"], b["nodes_per_graph"], num_nodes=b["x"].size(0), **kw)


def _run(pkg, b, entry="wls_bad_data_banded", **kw):
    return getattr(pkg.estimator, entry)(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def _compare_measurements(res, ref, s_min):
    """Worst errors of S and rN (the latter in units of max(rN, 1), where the oracle's S >= 2 s_min) against the oracle."""
    S = torch.cat([res.bus_sens.cpu().reshape(-1), res.edge_sens.cpu().reshape(-1)])
    rn = torch.cat([res.bus_rn.cpu().reshape(-1), res.edge_rn.cpu().reshape(-1)])
    S0 = torch.cat([ref["bus_sens"].reshape(-1), ref["edge_sens"].reshape(-1)])
    rn0 = torch.cat([ref["bus_rn"].reshape(-1), ref["edge_rn"].reshape(-1)])
    kept, low = S0 >= 2 * s_min, S0 < s_min / 2
    assert bool((rn[low] == 0).all()) and bool((rn0[low] == 0).all())
    assert torch.equal(S == 0, S0 == 0)             # inactive measurements: exactly 0 on both sides
    assert int((~kept & ~low).sum()) <= 0.1 * int((S0 != 0).sum())
    return (S - S0).abs().max().item(), ((rn - rn0).abs() / rn0.clamp_min(1.0))[kept].max().item(), int((~kept & ~low).sum())


def _clean_parity(tag, pkg, name, res, plain):
    """A max_removals = 0 result against the oracle of the clean data and, to the bit, against the plain banded solve."""
    hb, ref = bc.batch(name), cpu.clean(name)
    for f in SOLVE_FIELDS:
        assert torch.equal(getattr(res, f), getattr(plain, f)), (name, f)
    sens, std = cpu.bounds(name)
    rn_b = cpu.rn_bound(name, cpu.S_MIN_CMP)
    e_s, e_rn, left_out = _compare_measurements(res, ref, cpu.S_MIN_CMP)
    e_std = (res.state_std.cpu() - ref["state_std"]).abs().max().item()
    e_lim = ((res.chi2_limit.cpu() - ref["chi2_limit"]).abs() / ref["chi2_limit"]).max().item()
    G = hb["x"].shape[0] // hb["nodes_per_graph"]
    print(f"[banded bad-data {tag}] {name}: S {e_s:.2e}/{sens:.2e} rN {e_rn:.2e}/{rn_b:.2e} state_std {e_std:.2e}/{std:.2e} chi2_limit {e_lim:.1e}/1e-12 "
          f"dof {res.dof.tolist()} suspect {res.suspect.tolist()} left out {left_out}")
    assert res.bus_rn.shape == (hb["x"].shape[0], 4) and res.edge_sens.shape == (hb["edge_attr"].shape[0], 2) and res.removed.shape == (G, 1)
    assert res.bus_rn.dtype == res.bus_sens.dtype == res.state_std.dtype == torch.float64 and res.state.dtype == torch.float32
    assert torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.n_removed == 0).all()) and bool((res.removed == -1).all())
    assert e_s <= sens and e_rn <= rn_b and e_std <= std and e_lim <= 1e-12
    b = _device(name)
    assert bool((res.state_std[:, 1][b["x"][:, 9] != 0] == 0).all())


# ---- 1. clean data

@pytest.mark.parametrize("name", cpu.BEYOND)
def test_clean_data_match_the_oracle_and_the_solve_is_wls_estimate_banded(pkg, name):
    b = _device(name)
    assert b["nodes_per_graph"] > pkg.estimator.max_nodes_per_graph_large()
    _clean_parity("clean", pkg, name, _run(pkg, b, s_min=cpu.S_MIN_CMP, **FIXED), _run(pkg, b, "wls_estimate_banded", **FIXED))


# ---- 2. gross errors

def _removals(pkg, name, count, order=None):
    hb, targets = cpu.corrupted(name, count)
    ref = cpu.removal_oracle(name, count)
    kw = {} if order is None else dict(order=order)
    res = _run(pkg, _to_device(hb), **cpu.REMOVALS[count], **kw)
    n = hb["nodes_per_graph"]
    ok = torch.tensor([g in cpu.CLEAR[(name, count)] for g in range(len(ref["decisions"]))])
    rows = ok.repeat_interleave(n)
    bound_st = lc.state_bound(cpu.removal_state_spread(name, count)[ok].max().item())
    rn_b = cpu.rn_bound(name, 1e-3)                  # (the default s_min)
    e_st = (res.state.cpu().double() - ref["state"])[rows].abs().max().item()
    e_rem = ((res.removed_rn.cpu() - ref["removed_rn"]).abs() / ref["removed_rn"].clamp_min(1.0))[ok].max().item()
    print(f"[banded bad-data {count} error(s)] {name}: targets {targets} removed {res.removed.tolist()} n_removed {res.n_removed.tolist()} compared {ok.tolist()}: "
          f"removed_rn {e_rem:.2e}/{rn_b:.2e} state {e_st:.2e}/{bound_st:.2e} iterations {res.iterations.tolist()} suspect {res.suspect.tolist()}")
    assert torch.equal(res.removed.cpu()[ok], ref["removed"][ok]) and torch.equal(res.n_removed.cpu()[ok], ref["n_removed"][ok])
    assert torch.equal(res.iterations.cpu()[ok], ref["iterations"][ok]) and torch.equal(res.status.cpu()[ok], ref["status"][ok])
    assert e_rem <= rn_b and e_st <= bound_st
    # the graphs left out ran too: no failure, a finite state
    assert bool((res.status != 2).all()) and bool(torch.isfinite(res.state).all()) and bool(torch.isfinite(res.objective).all())
    N = hb["x"].shape[0]
    for g in torch.nonzero(ok).flatten().tolist():           # a removed measurement is inactive in the final solve -- at the CALLER's id
        for t in res.removed[g, :int(res.n_removed[g])].tolist():
            got = res.bus_sens.reshape(-1)[t] if t < 4 * N else res.edge_sens.reshape(-1)[t - 4 * N]
            assert float(got) == 0.0
    return res, ref


@pytest.mark.parametrize("name", cpu.BEYOND)
def test_one_gross_error_per_graph_is_removed(pkg, name):
    _removals(pkg, name, 1)


@pytest.mark.parametrize("name", cpu.BEYOND)
def test_three_gross_errors_per_graph_are_removed_in_the_oracles_order(pkg, name):
    _removals(pkg, name, 3)


def test_removed_ids_are_the_callers_under_a_non_identity_order(pkg):
    hb, _ = cpu.corrupted(cpu.RELABELLED)
    order = _order(pkg, _to_device(hb))
    res, ref = _removals(pkg, cpu.RELABELLED, 1, order=order)
    N = hb["x"].shape[0]
    ids = res.removed[:, 0].tolist()
    kernels = [4 * int(order.inverse[i // 4]) + i % 4 for i in ids]
    print(f"[banded bad-data labels] removed {ids} (the caller's ids); the kernel's own ids of the same measurements {kernels}")
    assert all(0 <= i < 4 * N for i in ids) and all(i != k for i, k in zip(ids, kernels))
    assert not torch.equal(order.perm.long().cpu(), torch.arange(N))


# ---- 3. band edges

def test_band_edges(pkg):
    """One 70-bus graph with the band forced to the minimum, around one and two blocks, and dense as a band; the star; the path."""
    b = _device("ober70")
    least = _order(pkg, b).half_bandwidth
    assert least < 15
    for hb in (least, 15, 16, 17, 31, 32, 33, 2 * 70 - 1):
        o = _order(pkg, b, half_bandwidth=hb)
        _clean_parity(f"edges hb={hb}", pkg, "ober70", _run(pkg, b, s_min=cpu.S_MIN_CMP, order=o, **FIXED),
                      _run(pkg, b, "wls_estimate_banded", order=o, **FIXED))
    for name, hb in (("star41", 81), ("path12", 5)):
        b = _device(name)
        assert _order(pkg, b).half_bandwidth == hb
        _clean_parity("edges", pkg, name, _run(pkg, b, s_min=cpu.S_MIN_CMP, **FIXED), _run(pkg, b, "wls_estimate_banded", **FIXED))


# ---- 4. against the dense form on sizes both serve

@pytest.mark.parametrize("name", ["ober70", "n100", "ober179"])
def test_against_the_dense_form(pkg, name):
    sens, std = cpu.bounds(name) if name == "ober70" else cpu_large.bounds(name)
    rn_b = sens / (2.0 * cpu.S_MIN_CMP)
    b = _device(name)
    kw = dict(s_min=cpu.S_MIN_CMP, **FIXED)
    band, dense = _run(pkg, b, **kw), _run(pkg, b, "wls_bad_data_large", **kw)
    st_b = bc.bound(name, FIXED["max_iter"], 0.0)
    e_st = (band.state.double() - dense.state.double()).abs().max().item()
    e_s = max((band.bus_sens - dense.bus_sens).abs().max().item(), (band.edge_sens - dense.edge_sens).abs().max().item())
    e_std = (band.state_std - dense.state_std).abs().max().item()
    S0 = torch.cat([dense.bus_sens.reshape(-1), dense.edge_sens.reshape(-1)])
    rn, rn0 = torch.cat([band.bus_rn.reshape(-1), band.edge_rn.reshape(-1)]), torch.cat([dense.bus_rn.reshape(-1), dense.edge_rn.reshape(-1)])
    e_rn = ((rn - rn0).abs() / rn0.clamp_min(1.0))[S0 >= 2 * cpu.S_MIN_CMP].max().item()
    print(f"[banded bad-data both forms] {name}: state {e_st:.2e}/{2 * st_b:.1e} S {e_s:.2e}/{2 * sens:.2e} rN {e_rn:.2e}/{2 * rn_b:.2e} state_std {e_std:.2e}/{2 * std:.2e}")
    assert torch.equal(band.iterations, dense.iterations) and torch.equal(band.status, dense.status)
    assert torch.equal(band.dof, dense.dof) and torch.equal(band.suspect, dense.suspect) and torch.equal(band.chi2_limit, dense.chi2_limit)
    assert e_st <= 2 * st_b and e_s <= 2 * sens and e_rn <= 2 * rn_b and e_std <= 2 * std
    # decisions: one gross error per graph, on the graphs whose decision is clear in the oracle
    if name == "ober70":
        hb = bc.batch(name)
        targets = bo.largest_sensitivity_targets(*cpu.args(hb))
        x2, ea2 = bo.add_gross_errors(hb["x"], hb["edge_attr"], hb["stats"], targets)
        bad = dict(hb, x=x2, edge_attr=ea2)
        ref = bo.bad_data(*cpu.args(bad), **cpu.REMOVALS[1])
        ok = torch.tensor([bool(d) and lead >= cpu.MIN_LEAD for d, lead in zip(cpu.decided(ref), cpu.leads(ref))])
    else:
        bad = cpu_large.corrupted(name)[0]
        ref = cpu_large.removal_oracle(name)
        ok = torch.tensor([bool(d) and (name, g) not in cpu_large.ONE_ERROR_LEFT_OUT for g, d in enumerate(cpu_large.decided(ref))])
    db = _to_device(bad)
    band, dense = _run(pkg, db, **cpu.REMOVALS[1]), _run(pkg, db, "wls_bad_data_large", **cpu.REMOVALS[1])
    print(f"[banded bad-data both forms] {name}: removed {band.removed.tolist()} dense {dense.removed.tolist()} oracle {ref['removed'].tolist()} compared {ok.tolist()}")
    assert bool(ok.any())
    assert torch.equal(band.removed.cpu()[ok], dense.removed.cpu()[ok]) and torch.equal(band.removed.cpu()[ok], ref["removed"][ok])
    assert torch.equal(band.n_removed.cpu()[ok], dense.n_removed.cpu()[ok]) and torch.equal(band.iterations.cpu()[ok], dense.iterations.cpu()[ok])


# ---- 5. reproducibility

def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


def test_runs_group_counts_and_batch_positions_agree_bitwise(pkg):
    hb = cpu.corrupted("n257")[0]
    b = _to_device(hb)
    kw = dict(threshold=4.0, max_removals=2, max_iter=6, tol=1e-6)
    res = _run(pkg, b, **kw)
    assert bool((res.n_removed == 1).all()) and bool((res.status == 0).all())
    assert _equal(_run(pkg, b, **kw), res)
    assert _equal(_run(pkg, b, max_groups=1, **kw), res)
    # graph 1 alone: its rows, its edges' rows and its per-graph outputs; its ids shifted by the graph's place
    n, E = 257, hb["edge_attr"].shape[0]
    first_edge = int((hb["edge_index"][0] < n).sum())
    alone = _to_device(dict(hb, x=hb["x"][n:], y=hb["y"][n:], edge_index=hb["edge_index"][:, first_edge:] - n, edge_attr=hb["edge_attr"][first_edge:]))
    out = _run(pkg, alone, **kw)
    for f in ("state", "bus_rn", "bus_sens", "state_std"):
        assert torch.equal(getattr(out, f), getattr(res, f)[n:]), f
    for f in ("edge_rn", "edge_sens"):
        assert torch.equal(getattr(out, f), getattr(res, f)[first_edge:]), f
    for f in ("objective", "iterations", "status", "last_step", "dof", "chi2_limit", "suspect", "removed_rn", "n_removed"):
        assert torch.equal(getattr(out, f)[0], getattr(res, f)[1]), f
    ids, ids_alone = res.removed[1].cpu(), out.removed[0].cpu()
    shifted = torch.where(ids < 0, ids, torch.where(ids < 4 * 2 * n, ids - 4 * n, ids - 4 * 2 * n - 2 * first_edge + 4 * n))
    assert torch.equal(ids_alone, shifted.to(ids_alone.dtype)) and int(ids_alone[0]) >= 0


@pytest.mark.parametrize("entry,kw", [("wls_bad_data_banded", dict(threshold=4.0, max_removals=2, max_iter=6, tol=1e-6)),
                                      ("wls_robust_banded", dict(gamma=3.0, max_iter=6, tol=1e-6))])
def test_replays_with_a_given_order_agree_bitwise(pkg, entry, kw):
    b, other = _to_device(cpu.corrupted("n257")[0]), _device("n257")
    order = _order(pkg, b)
    kw = dict(kw, order=order)
    eager, eager_other = _run(pkg, b, entry, **kw), _run(pkg, other, entry, **kw)
    assert not torch.equal(eager.state, eager_other.state)
    if entry == "wls_bad_data_banded":
        assert bool((eager.n_removed == 1).all()) and bool((eager_other.n_removed == 0).all())
    else:
        assert bool((eager.n_downweighted >= 1).all())
    # hipGraph
    static = _static_copy(b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(pkg, static, entry, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _run(pkg, static, entry, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(out, eager)
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(out, eager_other)
    # launch plan: the gathers around the solve are launches of the library, and replay with it
    static = _static_copy(b)
    with torch.no_grad():
        rec = pkg.graphs.PlannedStep(lambda: _run(pkg, static, entry, **kw))
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager)
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager_other)


# ---- 6. the guard and the refusals

def test_refusals_and_the_band_guard(pkg):
    est, lib = pkg.estimator, pkg._lib
    L = lib.lib()
    b = _device("n257")
    cap = est.band_max_half_bandwidth(257, bad_data=True)
    with pytest.raises(NotImplementedError, match=f"hb of at most {cap} states, got hb = {cap + 1}"):
        _run(pkg, b, order=_order(pkg, b, half_bandwidth=cap + 1))
    with pytest.raises(ValueError, match="order was made for"):
        _run(pkg, _device("n320"), order=_order(pkg, b))
    # a band one block too small for ONE graph of three (tests/test_gpu_wls_banded.py's batch): the star in the caller's numbering needs
    # Wb = 5; hb = 64 declares 4.  That graph: bd_refuse's outputs and its init; the chains beside it: the correct call's bits.
    g = _device("guard41")
    good = _order(pkg, g, identity=True)
    assert good.half_bandwidth == 81
    init = torch.stack([torch.linspace(0.98, 1.02, 123, device=DEV), torch.linspace(-0.01, 0.01, 123, device=DEV)], 1)
    init[g["x"][:, 9] != 0, 1] = 0.0
    kw = dict(max_iter=6, tol=1e-6, init=init, threshold=4.0, max_removals=2)
    want = _run(pkg, g, order=good, **kw)
    assert bool((want.status != 2).all())
    need = est.band_workspace_bytes(41, 64, 3)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    est._WORKSPACES[(g["x"].device, need)] = ws
    short = _run(pkg, g, order=good._replace(half_bandwidth=64), **kw)
    torch.cuda.synchronize()
    del est._WORKSPACES[(g["x"].device, need)]
    assert bool((ws[need // 3:2 * need // 3] == 0xA5).all()) and bool((ws[need:] == 0xA5).all())
    assert not bool((ws[:need // 3] == 0xA5).all()) and not bool((ws[2 * need // 3:need] == 0xA5).all())
    print(f"[banded bad-data guard] status {short.status.tolist()} iterations {short.iterations.tolist()} dof {short.dof.tolist()} removed {short.removed.tolist()} "
          f"against {want.status.tolist()} {want.iterations.tolist()} {want.dof.tolist()}")
    assert int(short.status[1]) == 2 and int(short.iterations[1]) == 0 and float(short.last_step[1]) == 0.0
    assert torch.equal(short.state[41:82], init[41:82]) and bool((short.objective[1] == 0).all())
    assert short.removed[1].tolist() == [-1, -1] and short.removed_rn[1].tolist() == [0.0, 0.0]
    assert int(short.n_removed[1]) == 0 and int(short.dof[1]) == 0 and int(short.suspect[1]) == 0 and math.isinf(float(short.chi2_limit[1]))
    for t in (short.bus_rn, short.bus_sens, short.state_std):
        assert bool((t[41:82] == 0).all())
    rows = {0: slice(0, 41), 2: slice(82, 123)}
    erows = {k: (g["edge_index"][0] >= 41 * k) & (g["edge_index"][0] < 41 * k + 41) for k in (0, 2)}
    for k in (0, 2):
        for f in ("state", "bus_rn", "bus_sens", "state_std"):
            assert torch.equal(getattr(short, f)[rows[k]], getattr(want, f)[rows[k]]), (f, k)
        for f in ("edge_rn", "edge_sens"):
            assert torch.equal(getattr(short, f)[erows[k]], getattr(want, f)[erows[k]]), (f, k)
        for f in ("objective", "iterations", "status", "last_step", "dof", "chi2_limit", "suspect", "removed", "removed_rn", "n_removed"):
            assert torch.equal(getattr(short, f)[k], getattr(want, f)[k]), (f, k)
    # through the ABI: rc 2 and a message, before any launch
    stream = lib.stream_ptr(torch.device(DEV))
    a = lib.WlsBadDataArgs()
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    a.solve.n_nodes, a.solve.n_edges, a.solve.nodes_per_graph, a.solve.max_iter, a.solve.tol = 514, 512, 257, 5, 1e-6
    a.threshold, a.s_min, a.z_p, a.max_removals = 3.0, 1e-3, 1.64, 1
    a.workspace, a.workspace_bytes, a.solve.half_bandwidth = buf.data_ptr(), 0, -1
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"half_bandwidth" in L.dss2_last_error() and b"banded" in L.dss2_last_error()
    a.solve.half_bandwidth = cap + 1
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and f"half-bandwidth of {cap + 1}".encode() in L.dss2_last_error()
    a.solve.half_bandwidth = 19
    need = est.band_workspace_bytes(257, 19, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and f"need {need}".encode() in L.dss2_last_error()
    a.workspace = ws.data_ptr() + 8
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"aligned" in L.dss2_last_error()
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"null argument" in L.dss2_last_error()      # (the Python formula is the C side's; the tensors are missing)
    ptr = torch.tensor([0, 257, 514], device=DEV)
    a.solve.graph_ptr, a.solve.n_graphs = ptr.data_ptr(), 2
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"graph_ptr" in L.dss2_last_error()
    r = lib.WlsRobustArgs()
    r.solve.n_nodes, r.solve.n_edges, r.solve.nodes_per_graph, r.solve.max_iter, r.solve.tol = 514, 512, 257, 5, 1e-6
    r.gamma, r.solve.half_bandwidth = 3.0, -1
    assert L.dss2_wls_robust_large(C.byref(r), stream) == 2 and b"half_bandwidth" in L.dss2_last_error()
    r.solve.half_bandwidth = 19
    assert L.dss2_wls_robust_large(C.byref(r), stream) == 2 and b"workspace is null" in L.dss2_last_error()
    r.workspace, r.workspace_bytes = ws.data_ptr(), need - 1
    assert L.dss2_wls_robust_large(C.byref(r), stream) == 2 and f"need {need}".encode() in L.dss2_last_error()
    r.solve.graph_ptr, r.solve.n_graphs = ptr.data_ptr(), 2
    assert L.dss2_wls_robust_large(C.byref(r), stream) == 2 and b"graph_ptr" in L.dss2_last_error()
    torch.cuda.synchronize()


# ---- 7. the Huber form

@pytest.mark.parametrize("name", ["n257", "radial300"])
def test_huber_matches_the_oracle(pkg, name):
    hb, _ = cpu.corrupted(name)
    ref = cpu.huber_oracle(name)
    sb, qb = cpu.huber_bounds(name)
    res = _run(pkg, _to_device(hb), "wls_robust_banded", max_iter=cpu.HUBER_ITERS, tol=0.0, gamma=ro.GAMMA)
    st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    ob = ((res.objective.cpu() - ref["objective"]).abs() / ref["objective"].abs()).max().item()
    qe = max((res.bus_q.cpu() - ref["bus_q"]).abs().max().item(), (res.edge_q.cpu() - ref["edge_q"]).abs().max().item())
    print(f"[banded huber parity] {name}: state {st:.2e}/{sb:.1e} q {qe:.2e}/{qb:.1e} cost {ob:.2e}/{cpu.HUBER_OBJ_BOUND:.0e} "
          f"down-weighted {res.n_downweighted.tolist()} oracle {ref['n_downweighted'].tolist()}")
    assert isinstance(res, pkg.estimator.WLSRobustResult) and res.bus_q.shape == (hb["x"].shape[0], 4) and res.bus_q.dtype == torch.float64
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert st <= sb and qe <= qb and ob <= cpu.HUBER_OBJ_BOUND
    assert sum(ro.near_threshold(ref)) == 0                   # (nothing is left out of the next comparison)
    assert ro.downweighted_ids(dict(bus_q=res.bus_q.cpu(), edge_q=res.edge_q.cpu())) == ro.downweighted_ids(ref)
    assert torch.equal(res.n_downweighted.cpu(), ref["n_downweighted"])


@pytest.mark.parametrize("name", ["n257", "radial300"])
def test_gamma_inf_is_the_plain_banded_solve_to_the_bit(pkg, name):
    b = _to_device(cpu.corrupted(name)[0])
    for kw in (dict(max_iter=1, tol=0.0), dict(max_iter=8, tol=0.0), dict(max_iter=20, tol=1e-6)):
        plain = _run(pkg, b, "wls_estimate_banded", **kw)
        for plain_iters in (0, 1):
            res = _run(pkg, b, "wls_robust_banded", gamma=float("inf"), plain_iters=plain_iters, **kw)
            for f in SOLVE_FIELDS:
                assert torch.equal(getattr(res, f), getattr(plain, f)), (name, kw, f)
            assert bool((res.bus_q == 1.0).all()) and bool((res.edge_q == 1.0).all()) and bool((res.n_downweighted == 0).all())


def test_huber_against_the_dense_form_on_ober179(pkg):
    b = _to_device(ro.corrupted("ober179")[0])
    kw = dict(max_iter=14, tol=0.0, gamma=ro.GAMMA)            # (the fixed trip count tests/test_gpu_wls_robust.py holds ober179 to)
    band, dense = _run(pkg, b, "wls_robust_banded", **kw), _run(pkg, b, "wls_robust", large=True, **kw)
    sb, qb = 5e-7, 1e-9                                        # tests/test_gpu_wls_robust.py's floors, which hold ober179 from three iterations on
    st = (band.state.double() - dense.state.double()).abs().max().item()
    qe = max((band.bus_q - dense.bus_q).abs().max().item(), (band.edge_q - dense.edge_q).abs().max().item())
    ob = ((band.objective - dense.objective).abs() / dense.objective.abs()).max().item()
    print(f"[banded huber both forms] ober179: state {st:.2e}/{2 * sb:.1e} q {qe:.2e}/{2 * qb:.1e} cost {ob:.2e}/{2e-6:.0e} down-weighted {band.n_downweighted.tolist()}")
    assert torch.equal(band.iterations, dense.iterations) and torch.equal(band.status, dense.status)
    assert torch.equal(band.n_downweighted, dense.n_downweighted)
    assert st <= 2 * sb and qe <= 2 * qb and ob <= 2e-6


# ---- 8. the runner

def test_evaluate_wls_routes_the_gross_error_forms_above_256_buses(pkg):
    b = _to_device(cpu.corrupted("radial300")[0])
    loader = [{k: v for k, v in b.items() if k != "stats"}]
    bad, robust = dict(threshold=4.0, max_removals=3), dict(gamma=3.0)
    for kw in (dict(bad_data=dict(bad, large="auto")), dict(robust=robust)):
        with pytest.raises(NotImplementedError, match="buses per graph, got 300"):
            pkg.runner.evaluate_wls(loader, b["stats"], 300, max_iter=8, tol=0.0, **kw)
    got = pkg.runner.evaluate_wls(loader, b["stats"], 300, max_iter=8, tol=0.0, banded="auto", bad_data=dict(bad, large="auto"))
    print(f"[banded bad-data evaluate] removed {got['wls_removed']} suspect {got['wls_suspect']} not converged {got['wls_not_converged']} rmse_v {got['rmse_v']:.4g}")
    assert set(got) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged", "wls_suspect", "wls_removed"}
    assert got["wls_removed"] == 2 and all(math.isfinite(got[k]) for k in pkg.data.EVAL_METRICS)
    assert pkg.runner.evaluate_wls(loader, b["stats"], 300, max_iter=8, tol=0.0, banded=True, bad_data=bad) == got
    rob = pkg.runner.evaluate_wls(loader, b["stats"], 300, max_iter=8, tol=0.0, banded="auto", robust=robust)
    print(f"[banded huber evaluate] down-weighted {rob['wls_downweighted']} not converged {rob['wls_not_converged']} rmse_v {rob['rmse_v']:.4g}")
    assert set(rob) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged", "wls_downweighted"}
    assert rob["wls_downweighted"] >= 2 and all(math.isfinite(rob[k]) for k in pkg.data.EVAL_METRICS)
