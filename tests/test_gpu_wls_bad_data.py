"""GPU: estimator.wls_bad_data / csrc/dss2_wls_bad_data.hip against the fp64 oracle of tests/wls_bad_data_oracle.py (sensitivities from a
QR, not the kernel's inverse of the gain matrix) on the batches of tests/wls_cases.py: 3 to 7 graphs of 2 to 70 buses.

Bounds (from two fp64 routes on the CPU, tests/test_wls_bad_data_cpu.py; never from the kernel), at tol = 0 and 8 iterations per solve:
  bus_sens, edge_sens   2e-7 absolute (8 x the 2.0e-8 the two routes differ by)
  rN, removed_rn        1e-4 max(rN, 1) where the oracle's S >= 2 s_min -- the S bound at the floor, 2e-7 / (2 * 1e-3); measurements with
                        S inside [s_min / 2, 2 s_min] are left out (at most 10 % of the active ones), below s_min / 2 both sides give 0
  dof, suspect          equal;  chi2_limit 1e-12 relative to the same formula in fp64
  state_std             3.44e-9 absolute = 8 x 4.3e-10, the worst difference between the two fp64 routes (4.24e-10, n33, the measurements
                        entering the gain matrix in a random order)
  state                 5e-7 absolute, as for wls_estimate
A removal is compared where the oracle's winner leads its runner-up, and every arg-max of the graph is away from the threshold, by at
least 1e-3 relative; the graphs left out are at most 10 %.  With max_removals = 0 the solve's five outputs are wls_estimate's to the bit.
Every test prints its errors beside the bounds (run with -s).
"""
import ctypes as C
import functools
import importlib

import pytest
import torch

import wls_bad_data_oracle as bo
import wls_cases as wc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENS_BOUND, RN_BOUND, STATE_BOUND, STD_BOUND, S_MIN, LEAD = 2e-7, 1e-4, 5e-7, 8 * 4.3e-10, 1e-3, 1e-3
FIXED = dict(max_iter=8, tol=0.0)
SOLVE_FIELDS = ("state", "objective", "iterations", "status", "last_step")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


@functools.lru_cache(maxsize=None)
def _host(name):
    return wc.any_batch(name)


def _to_device(b):
    return {k: (tuple(s.to(DEV) for s in v) if k == "stats" else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _device(name):
    return _to_device(_host(name))


@functools.lru_cache(maxsize=None)
def _corrupted(name):
    """One gross error of +25 sigma per graph, at the measurement of largest S with a non-zero Jacobian row: (host batch, targets)."""
    b = _host(name)
    targets = bo.largest_sensitivity_targets(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"])
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], targets)
    return dict(b, x=x2, edge_attr=ea2), targets


@functools.lru_cache(maxsize=None)
def _two_errors():
    """cigre14 with two gross errors on graph 2 (the two largest S; in the oracle both decisions lead by more than 10 %)."""
    b = _host("cigre14")
    args = (b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"])
    ids = [bo.largest_sensitivity_targets(*args, rank=r)[2] for r in (0, 1)]
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], ids)
    return dict(b, x=x2, edge_attr=ea2), ids


def _oracle_of(b, **kw):
    return bo.bad_data(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"], **kw)


@functools.lru_cache(maxsize=None)
def _oracle(name, case):
    if case == "clean":
        return _oracle_of(_host(name), **FIXED)
    if case == "one":
        return _oracle_of(_corrupted(name)[0], threshold=4.0, max_removals=3, **FIXED)
    return _oracle_of(_two_errors()[0], threshold=4.0, max_removals=int(case), **FIXED)


def _run(pkg, b, **kw):
    return pkg.estimator.wls_bad_data(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _estimate(pkg, b, **kw):
    return pkg.estimator.wls_estimate(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def _decided(ref, threshold):
    """[G] bool: every arg-max of the graph is at least LEAD away from the threshold, every removal leads its runner-up by LEAD."""
    out = []
    for dec in ref["decisions"]:
        ok = True
        for _, best, second in dec:
            ok = ok and abs(best - threshold) >= LEAD * threshold and (best <= threshold or best - second >= LEAD * best)
        out.append(ok)
    return torch.tensor(out)


def _compare_measurements(res, ref, rows=None, erows=None):
    """Worst errors of S and rN (the latter in units of max(rN, 1)) against the oracle, the counts of compared / left-out measurements."""
    S = torch.cat([res.bus_sens.cpu()[rows].reshape(-1), res.edge_sens.cpu()[erows].reshape(-1)])
    rn = torch.cat([res.bus_rn.cpu()[rows].reshape(-1), res.edge_rn.cpu()[erows].reshape(-1)])
    S0 = torch.cat([ref["bus_sens"][rows].reshape(-1), ref["edge_sens"][erows].reshape(-1)])
    rn0 = torch.cat([ref["bus_rn"][rows].reshape(-1), ref["edge_rn"][erows].reshape(-1)])
    kept, low = S0 >= 2 * S_MIN, S0 < S_MIN / 2
    assert bool((rn[low] == 0).all()) and bool((rn0[low] == 0).all())
    e_s = (S - S0).abs().max().item()
    e_rn = ((rn - rn0).abs() / rn0.clamp_min(1.0))[kept].max().item()
    return e_s, e_rn, int((~kept & ~low).sum())


ALL = slice(None)


@pytest.mark.parametrize("max_iter", [1, 8])
@pytest.mark.parametrize("name", wc.ALL_BATCHES)
def test_without_removals_the_solve_is_wls_estimate_to_the_bit(pkg, name, max_iter):
    b = _device(name)
    for tol in (0.0, 1e-6):
        res, ref = _run(pkg, b, max_iter=max_iter, tol=tol), _estimate(pkg, b, max_iter=max_iter, tol=tol)
        for f in SOLVE_FIELDS:
            assert torch.equal(getattr(res, f), getattr(ref, f)), (name, max_iter, tol, f)
    init = _host(name)["y"].double().clone()
    init[:, 0] += 0.01
    init = init.float().to(DEV)
    res, ref = _run(pkg, b, init=init, max_iter=max_iter, tol=1e-6), _estimate(pkg, b, init=init, max_iter=max_iter, tol=1e-6)
    for f in SOLVE_FIELDS:
        assert torch.equal(getattr(res, f), getattr(ref, f)), (name, max_iter, "warm", f)
    assert bool((res.n_removed == 0).all()) and bool((res.removed == -1).all()) and res.removed.shape == (b["num_graphs"], 1)


def test_parity_at_fixed_trip_counts(pkg):
    near = active = 0
    for name in wc.ALL_BATCHES:
        ref, b = _oracle(name, "clean"), _host(name)
        res = _run(pkg, _device(name), **FIXED)
        e_s, e_rn, left_out = _compare_measurements(res, ref, ALL, ALL)
        e_std = (res.state_std.cpu() - ref["state_std"]).abs().max().item()
        e_lim = ((res.chi2_limit.cpu() - ref["chi2_limit"]).abs() / ref["chi2_limit"]).max().item()
        e_st = (res.state.cpu().double() - ref["state"]).abs().max().item()
        n = b["nodes_per_graph"]
        G = b["num_graphs"]
        trace = res.bus_sens.reshape(G, -1).sum(1).index_add(0, _device(name)["edge_index"][0] // n, res.edge_sens.sum(1)).cpu()
        e_tr = (trace - res.dof.cpu().double()).abs().max().item()
        near, active = near + left_out, active + int((ref["bus_sens"] != 0).sum()) + int((ref["edge_sens"] != 0).sum())
        print(f"[bad-data parity] {name}: S {e_s:.2e}/{SENS_BOUND:.0e} rN {e_rn:.2e}/{RN_BOUND:.0e} state_std {e_std:.2e}/{STD_BOUND:.2e} chi2_limit {e_lim:.1e}/1e-12 "
              f"state {e_st:.2e}/{STATE_BOUND:.0e} sum S - dof {e_tr:.1e}/1e-6 dof {res.dof.tolist()} suspect {res.suspect.tolist()} left out {left_out}")
        assert res.bus_rn.dtype == torch.float64 and res.bus_rn.shape == (b["x"].shape[0], 4) and res.edge_sens.shape == (b["edge_attr"].shape[0], 2)
        assert res.dof.dtype == torch.int32 and res.suspect.dtype == torch.int32 and res.state_std.shape == (b["x"].shape[0], 2)
        assert torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
        assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
        assert e_s <= SENS_BOUND and e_rn <= RN_BOUND and e_std <= STD_BOUND and e_lim <= 1e-12 and e_st <= STATE_BOUND and e_tr <= 1e-6
        assert bool((res.state_std[:, 1][_device(name)["x"][:, 9] != 0] == 0).all())
        # inactive measurements: exactly 0 on both sides
        assert torch.equal(res.bus_sens.cpu() == 0, ref["bus_sens"] == 0) and torch.equal(res.edge_sens.cpu() == 0, ref["edge_sens"] == 0)
    print(f"[bad-data parity] {near} of {active} active measurements have S within a factor 2 of s_min and are left out of the rN comparison")
    assert near <= 0.1 * active


@pytest.mark.parametrize("name", wc.ALL_BATCHES)
def test_clean_data_lose_nothing(pkg, name):
    b = _device(name)
    res, plain = _run(pkg, b, threshold=4.0, max_removals=3, **FIXED), _run(pkg, b, **FIXED)
    print(f"[bad-data clean] {name}: largest rN {max(res.bus_rn.max().item(), res.edge_rn.max().item()):.3f} n_removed {res.n_removed.tolist()}")
    assert bool((res.n_removed == 0).all()) and bool((res.removed == -1).all()) and res.removed.shape == (b["num_graphs"], 3)
    assert bool((res.removed_rn == 0).all())
    assert torch.equal(res.state, plain.state) and torch.equal(res.objective, plain.objective) and torch.equal(res.bus_rn, plain.bus_rn)


def test_one_gross_error_per_graph_is_removed(pkg):
    graphs = left_out = 0
    for name in wc.ALL_BATCHES:
        hb, targets = _corrupted(name)
        ref = _oracle(name, "one")
        res = _run(pkg, _to_device(hb), threshold=4.0, max_removals=3, **FIXED)
        ok = _decided(ref, 4.0)
        graphs, left_out = graphs + ok.numel(), left_out + int((~ok).sum())
        n = hb["nodes_per_graph"]
        rows = ok.repeat_interleave(n)
        erows = ok[hb["edge_index"][0] // n]
        e_st = (res.state.cpu().double() - ref["state"])[rows].abs().max().item()
        e_rem = ((res.removed_rn.cpu() - ref["removed_rn"]).abs() / ref["removed_rn"].clamp_min(1.0))[ok].max().item()
        e_s, e_rn, _ = _compare_measurements(res, ref, rows, erows)
        print(f"[bad-data one error] {name}: targets {targets} removed {res.removed[:, 0].tolist()} rN {['%.2f' % v for v in res.removed_rn[:, 0].tolist()]} "
              f"n_removed {res.n_removed.tolist()} decided {ok.tolist()}: removed_rn {e_rem:.2e}/{RN_BOUND:.0e} state {e_st:.2e}/{STATE_BOUND:.0e} "
              f"after the removal S {e_s:.2e}/{SENS_BOUND:.0e} rN {e_rn:.2e}/{RN_BOUND:.0e} suspect {res.suspect.tolist()}")
        assert ref["removed"][:, 0].tolist() == targets and ref["n_removed"].tolist() == [1] * len(targets)
        assert torch.equal(res.removed.cpu()[ok], ref["removed"][ok]) and torch.equal(res.n_removed.cpu()[ok], ref["n_removed"][ok])
        assert torch.equal(res.iterations.cpu()[ok], ref["iterations"][ok]) and torch.equal(res.dof.cpu()[ok], ref["dof"][ok])
        assert torch.equal(res.suspect.cpu()[ok], ref["suspect"][ok])
        assert e_rem <= RN_BOUND and e_st <= STATE_BOUND and e_s <= SENS_BOUND and e_rn <= RN_BOUND
        # the removed measurement is inactive in the final solve
        for g in torch.nonzero(ok).flatten().tolist():
            t = targets[g]
            N = hb["x"].shape[0]
            got = res.bus_sens.reshape(-1)[t] if t < 4 * N else res.edge_sens.reshape(-1)[t - 4 * N]
            assert float(got) == 0.0
    print(f"[bad-data one error] {left_out} of {graphs} graphs decide within 1e-3 and are left out")
    assert graphs == 27 and left_out <= 0.1 * graphs


def test_two_errors_the_cap_and_what_stays_suspect(pkg):
    hb, ids = _two_errors()
    b = _to_device(hb)
    both, one = _oracle("cigre14", "2"), _oracle("cigre14", "1")
    assert bool(_decided(both, 4.0).all()) and sorted(both["removed"][2].tolist()) == sorted(ids) and both["n_removed"].tolist() == [0, 0, 2, 0, 0]
    res = _run(pkg, b, threshold=4.0, max_removals=2, **FIXED)
    e_rem = ((res.removed_rn.cpu() - both["removed_rn"]).abs() / both["removed_rn"].clamp_min(1.0)).max().item()
    e_st = (res.state.cpu().double() - both["state"]).abs().max().item()
    print(f"[bad-data two errors] injected {ids} removed {res.removed[2].tolist()} (oracle {both['removed'][2].tolist()}) rN {res.removed_rn[2].tolist()} "
          f"removed_rn {e_rem:.2e}/{RN_BOUND:.0e} state {e_st:.2e}/{STATE_BOUND:.0e} iterations {res.iterations.tolist()} suspect {res.suspect.tolist()}")
    assert torch.equal(res.removed.cpu(), both["removed"]) and torch.equal(res.n_removed.cpu(), both["n_removed"])
    assert torch.equal(res.iterations.cpu(), both["iterations"]) and torch.equal(res.suspect.cpu(), both["suspect"]) and int(res.suspect[2]) == 0
    assert e_rem <= RN_BOUND and e_st <= STATE_BOUND
    capped = _run(pkg, b, threshold=4.0, max_removals=1, **FIXED)
    print(f"[bad-data cap] removed {capped.removed[:, 0].tolist()} n_removed {capped.n_removed.tolist()} suspect {capped.suspect.tolist()} largest rN left {capped.bus_rn[30:45].max().item():.2f}")
    assert capped.n_removed.tolist() == [0, 0, 1, 0, 0] and capped.removed.shape == (5, 1) and int(capped.removed[2, 0]) == int(both["removed"][2, 0])
    assert int(capped.suspect[2]) == 1 and torch.equal(capped.suspect.cpu(), one["suspect"]) and torch.equal(capped.iterations.cpu(), one["iterations"])
    assert max(capped.bus_rn[30:45].max().item(), 0.0) > 4.0


def test_a_graph_without_measurements_fails_alone(pkg):
    hb, _ = _corrupted("cigre14")
    b = _to_device(hb)
    n, ei = 15, b["edge_index"]
    xm, eam = b["x"].clone(), b["edge_attr"].clone()
    xm[2 * n:3 * n, :8] = 0.0
    edges2 = (ei[0] >= 2 * n) & (ei[0] < 3 * n)
    eam[edges2, :4] = 0.0
    kw = dict(threshold=4.0, max_removals=2, max_iter=12, tol=1e-6)
    ref, res = _run(pkg, b, **kw), _run(pkg, dict(b, x=xm, edge_attr=eam), **kw)
    print(f"[bad-data masked] status {res.status.tolist()} n_removed {res.n_removed.tolist()} dof {res.dof.tolist()} suspect {res.suspect.tolist()}")
    assert res.status.tolist() == [0, 0, 2, 0, 0] and res.n_removed.tolist() == [1, 1, 0, 1, 1] and int(res.iterations[2]) == 0
    assert int(res.suspect[2]) == 0 and float(res.chi2_limit[2]) == float("inf") and int(res.dof[2]) < 0 and bool((res.removed[2] == -1).all())
    assert torch.equal(res.state[2 * n:3 * n], torch.tensor([1.0, 0.0], device=DEV).expand(n, 2))
    for t in (res.bus_rn[2 * n:3 * n], res.bus_sens[2 * n:3 * n], res.state_std[2 * n:3 * n], res.edge_rn[edges2], res.edge_sens[edges2]):
        assert bool((t == 0).all())
    others = torch.tensor([True, True, False, True, True], device=DEV)
    rows, erows = others.repeat_interleave(n), ~edges2
    for f in res._fields:
        got, want = getattr(res, f), getattr(ref, f)
        sel = rows if f in ("state", "bus_rn", "bus_sens", "state_std") else (erows if f in ("edge_rn", "edge_sens") else others)
        assert torch.equal(got[sel], want[sel]), f
    assert bool(torch.isfinite(res.objective).all())


def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


@pytest.mark.parametrize("name", ["cigre14", "ober_sub"])
def test_runs_copies_group_caps_and_replays_agree_bitwise(pkg, name):
    hb, _ = _corrupted(name)
    b, other = _to_device(hb), _device(name)
    kw = dict(threshold=4.0, max_removals=2, max_iter=6, tol=1e-6)
    eager = _run(pkg, b, **kw)
    assert bool((eager.n_removed == 1).all())
    assert _equal(_run(pkg, b, **kw), eager)
    for groups in (1, 7):
        assert _equal(_run(pkg, b, max_groups=groups, **kw), eager)
    eager_other = _run(pkg, other, **kw)
    assert not torch.equal(eager_other.state, eager.state) and bool((eager_other.n_removed == 0).all())
    # copies of the batch in one batch: every copy's rows equal the first's (ids shifted by the copy's offset)
    if name == "cigre14":
        big = pkg.synthetic.tile_real_batch(hb, 3)
        dev = dict(_to_device({k: v for k, v in big.items() if k != "stats"}), stats=b["stats"])
        res = _run(pkg, dev, **kw)
        N, E, G = hb["x"].shape[0], hb["edge_attr"].shape[0], hb["num_graphs"]
        for f in res._fields:
            if f == "removed":
                continue
            v = getattr(res, f).reshape(3, -1)
            assert torch.equal(v, v[:1].expand_as(v)), f
            assert torch.equal(v[0], getattr(eager, f).reshape(-1)), f
        bus = eager.removed < 4 * N
        for k in range(3):
            want = torch.where(bus, eager.removed + 4 * N * k, eager.removed + 4 * N * 2 + 2 * E * k)
            assert torch.equal(res.removed[k * G:(k + 1) * G], torch.where(eager.removed < 0, eager.removed, want))
    # hipGraph
    static = _static_copy(b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(pkg, static, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _run(pkg, static, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(out, eager)
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(out, eager_other)
    # launch plan
    static = _static_copy(b)
    with torch.no_grad():
        rec = pkg.graphs.PlannedStep(lambda: _run(pkg, static, **kw))
    assert rec.n_launches == 1
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager)
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager_other)


def test_refusals(pkg):
    b, h = _device("cigre14"), _host("cigre14")
    big = pkg.synthetic.make_batch(["ober179"], 1, seed=0)
    with pytest.raises(NotImplementedError, match=str(pkg.estimator.max_nodes_per_graph())):
        pkg.estimator.wls_bad_data(big["x"].to(DEV), big["edge_index"].to(DEV), big["edge_attr"].to(DEV), *[s.to(DEV) for s in big["stats"]], 179)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.estimator.wls_bad_data(h["x"], h["edge_index"], h["edge_attr"], *h["stats"], 15)
    for kw, what in ((dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(max_removals=-1), "max_removals"),
                     (dict(max_removals=65), "max_removals"), (dict(max_removals=1.5), "max_removals"), (dict(confidence=0.0), "confidence"),
                     (dict(confidence=1.0), "confidence"), (dict(s_min=0.0), "s_min"), (dict(s_min=1.0), "s_min"), (dict(max_iter=0), "max_iter"),
                     (dict(tol=-1.0), "tol"), (dict(nodes_per_graph=14), "nodes_per_graph"), (dict(init=torch.ones(75, 3, device=DEV)), "init must be")):
        with pytest.raises(ValueError, match=what):
            _run(pkg, dict(b, nodes_per_graph=kw.pop("nodes_per_graph", 15)), **kw)
    # through the ABI: rc 2 and a message, before any launch
    L, lib = pkg._lib.lib(), pkg._lib
    stream = lib.stream_ptr(torch.device(DEV))
    assert L.dss2_wls_bad_data(None, stream) == 2 and b"null" in L.dss2_last_error()
    a = lib.WlsBadDataArgs()
    a.solve.n_nodes, a.solve.n_edges, a.solve.nodes_per_graph, a.solve.max_iter, a.solve.tol = 179, 178, 179, 5, 1e-6
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"LDS" in L.dss2_last_error()
    a.solve.n_nodes, a.solve.nodes_per_graph = 31, 15
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"multiple" in L.dss2_last_error()
    # a complete argument block whose ids do not fit int32, then one with a threshold of 0: refused before anything is read
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    a = lib.WlsBadDataArgs()
    s = a.solve
    for f in ("x", "edge_attr", "x_mean", "x_std", "edge_mean", "edge_std", "efrom", "eto", "inc_rowptr", "inc_ent", "state", "objective",
              "iterations", "status", "last_step", "vminmax"):
        setattr(s, f, buf.data_ptr())
    for f in ("dof", "chi2_limit", "suspect", "removed", "removed_rn", "n_removed", "bus_rn", "bus_sens", "edge_rn", "edge_sens", "state_std"):
        setattr(a, f, buf.data_ptr())
    s.ldx, s.ldea, s.nodes_per_graph, s.max_iter, s.tol = 11, 13, 15, 5, 1e-6
    a.threshold, a.s_min, a.z_p, a.max_removals = 3.0, 1e-3, 1.64, 1
    s.n_nodes, s.n_edges = 15 * (2 ** 29 // 15), 2 ** 29
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"int32" in L.dss2_last_error()
    s.n_nodes, s.n_edges, a.threshold = 15, 14, 0.0
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"threshold" in L.dss2_last_error()
    a.threshold, a.max_removals = 3.0, 65
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"max_removals" in L.dss2_last_error()
    torch.cuda.synchronize()


def test_evaluate_wls_removes_what_was_injected(pkg):
    stats_h = _host("cigre14")["stats"]
    stats = _device("cigre14")["stats"]
    loader, injected = [], 0
    for seed in (21, 22):
        hb = dict(pkg.synthetic.make_batch(["cigre14"], 4, seed=seed, stats=stats_h), nodes_per_graph=15)
        targets = bo.largest_sensitivity_targets(hb["x"], hb["edge_index"], hb["edge_attr"], stats_h, 15)
        x2, ea2 = bo.add_gross_errors(hb["x"], hb["edge_attr"], stats_h, targets)
        injected += len(targets)
        loader.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in dict(hb, x=x2, edge_attr=ea2).items() if k != "stats"})
    plain = pkg.runner.evaluate_wls(loader, stats, 15)
    got = pkg.runner.evaluate_wls(loader, stats, 15, bad_data=dict(threshold=4.0, max_removals=3))
    print(f"[bad-data evaluate] removed {got['wls_removed']} of {injected} injected, suspect {got['wls_suspect']}, rmse_v {got['rmse_v']:.4g} against {plain['rmse_v']:.4g} without")
    assert set(plain) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged"}
    assert set(got) == set(plain) | {"wls_suspect", "wls_removed"}
    assert got["wls_removed"] == injected and got["wls_not_converged"] == 0
    assert got["rmse_v"] <= plain["rmse_v"]
    # synthetic.corrupt_measurements: random active measurements; every graph is flagged or cleaned, and nothing fails
    noisy, ids = pkg.synthetic.corrupt_measurements(dict(_device("cigre14")), per_graph=1, sigmas=25.0, seed=1)
    res = _run(pkg, noisy, threshold=4.0, max_removals=3)
    print(f"[bad-data evaluate] corrupt_measurements ids {ids[:, 0].tolist()} removed {res.removed[:, 0].tolist()} suspect {res.suspect.tolist()}")
    assert ids.shape == (5, 1) and bool((res.status == 0).all())
