"""CPU: what tests/test_gpu_wls_banded_bad_data.py relies on, without a GPU -- estimator.wls_bad_data_banded and wls_robust_banded
(csrc/dss2_wls_bad_data.hip's banded kernel, csrc/dss2_wls_banded_invert.hpp, csrc/dss2_wls_banded.hpp) on the batches of
tests/wls_banded_cases.py.

(a) csrc/dss2_wls_banded_invert.hpp's selected inverse restated in numpy ON ITS STORAGE LAYOUT (the band rows; the panel Yp in the Pt
    block of LDS, row-major, a row's place counted from the panel's first row; Ld, invd and T), fed from test_wls_banded_cpu.banded_solve's L,
    against np.linalg.inv(G) at every stored position of the lower band: relative to sqrt(Sigma_ii Sigma_jj) within 100 cond(G) eps, the
    form of the factorisation's own bound there.  Everything the kernel may not read -- the b row, the padding rows, the columns left of
    0, what lies above the diagonal, the panel before it is written -- starts as NaN, every value read is asserted finite, and what was
    NaN and is not a stored lower-band position is NaN afterwards.  Slack angles: 1 on the diagonal, exactly 0 beside it.
    ober70 at hb = minimum, 15, 16, 17, 31, 32, 33 and 139 (dense as a band); path12 at minimum, 16, 23; star41 at 81 (dense); n257 at
    minimum, 32, 33.  4 ceil(ns / 16) + 1 barriers.
(b) the positions bd_bus asks Sigma for -- (bus, bus), (bus, neighbour), (neighbour, neighbour of the same bus), both states of each --
    enumerated from the relabelled edge list of every batch the GPU file runs: each lies in the stored band of band_order's hb.
(c) the fixtures of the GPU tests on n257, n320 and radial300 (two graphs each), measured in the fp64 oracle alone by the procedure of
    tests/test_wls_bad_data_large_cpu.py and printed (-s): the share of S within a factor 2 of s_min = 1e-4 (at most 10 %); the spread of
    the three fp64 routes to S and state_std, x 8, floors 2e-7 and 3.44e-9 -> bounds(name), rn_bound(name, s_min); gross errors of
    +25 sigma at the measurements of largest S (ranks 0, and 0, 1, 2): a graph is CLEAR when every arg-max is 1e-3 away from the
    threshold (decided) and every removal leads its runner-up by at least 1 %; at most one graph per batch is not, asserted.
(d) the host side: the LDS formula with the bad-data block against a hand count at n = 257, hb = 19, monotone in n and hb, the cap, the
    refusals that need no GPU, the struct's new field.
"""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

import wls_bad_data_oracle as bo
import wls_banded_cases as bc
import wls_edge_cases as we
import wls_large_cases as lc
import wls_oracle as wo
import wls_robust_oracle as ro
from conftest import load_pkg
from test_wls_bad_data_large_cpu import FIXED, LEAD, REMOVAL_KW, S_MIN_CMP, SENS_BOUND, STD_BOUND, decided
from test_wls_banded_cpu import NB, TILE, _normal_equations, banded_solve

BEYOND = ("n257", "n320", "radial300")
MIN_LEAD = 1e-2                      # the oracle's top two rN at every removal of a compared graph
RELABELLED = "relabelled257"         # n257 in a caller's random numbering: the batch whose removed ids differ between the two numberings


@pytest.fixture(scope="module")
def est():
    return load_pkg().estimator


# ---- (a) the selected inverse

def band_selinv(L, hb):
    """The stored lower band of Sigma = (L L^T)^-1 by wb_selinv's steps on wb_selinv's arrays.  Returns (Sigma [ns, ns] with NaN at what is
    not a stored lower-band position, stored [ns, ns] bool, barriers)."""
    ns = L.shape[0]
    Wb = -(-hb // NB)
    W, shift, nbr = NB * (Wb + 1), NB * Wb, -(-ns // NB)
    A = np.full(nbr * NB * W + NB * nbr, np.nan)

    def at(r):
        return r * W + shift - r // NB * NB

    def left(r):
        return max(0, r // NB * NB - shift)

    stored = np.zeros(A.shape, dtype=bool)
    for r in range(ns):
        assert not L[r, :left(r)].any(), "the factor leaves the declared band"
        A[at(r) + left(r):at(r) + r + 1] = L[r, left(r):r + 1]
        stored[at(r) + left(r):at(r) + r + 1] = True
    S = NB * Wb + TILE

    def read(off, n=1):
        v = A[off:off + n]
        assert stored[off:off + n].all() and np.isfinite(v).all(), "a read outside the stored lower band, or of a NaN"
        return v.copy() if n > 1 else float(v[0])

    def solve(x, Ld, invd):                         # y L_JJ = x, columns from the last
        for k in range(NB - 1, -1, -1):
            x[k] *= invd[k]
            x[:k] -= x[k] * Ld[k, :k]
        return x

    barriers = 1
    for j0 in range((ns - 1) // NB * NB, -1, -NB):
        w = min(NB, ns - j0)
        first = j0 + w
        end = min(ns, first + shift)
        npan = end - first
        assert npan == 0 or w == NB
        Yp = np.full(NB * S, np.nan)                # (the Pt block of LDS; nothing of an earlier panel may be needed)
        assert NB * npan <= NB * S
        Ld = np.eye(NB)
        for q in range(w):
            Ld[q, :q + 1] = read(at(j0 + q) + j0, q + 1)
        invd = 1.0 / np.diag(Ld)
        for i in range(first, end):
            Yp[NB * (i - first):NB * (i - first) + NB] = solve(read(at(i) + j0, NB), Ld, invd)
        T = np.stack([solve(np.eye(NB)[q].copy(), Ld, invd) for q in range(NB)])
        out = np.zeros((npan, NB))
        for i in range(first, end):
            acc = np.zeros(NB)
            for k in range(first, end):
                s = read(at(max(i, k)) + min(i, k))
                y = Yp[NB * (k - first):NB * (k - first) + NB]
                assert np.isfinite(y).all(), "the panel is read where it was not written"
                acc += s * y
            out[i - first] = 0.0 - acc
        for i in range(first, end):
            A[at(i) + j0:at(i) + j0 + NB] = out[i - first]
        for a in range(w):
            for b in range(a + 1):
                s = 0.0
                for m in range(NB):
                    s += T[m, a] * T[m, b]
                for k in range(first, end):
                    s -= Yp[NB * (k - first) + a] * read(at(k) + j0 + b)
                A[at(j0 + a) + j0 + b] = s
        barriers += 4
    assert np.isnan(A[~stored]).all(), "something outside the stored lower band was written"
    Sg = np.full((ns, ns), np.nan)
    inband = np.zeros((ns, ns), dtype=bool)
    for r in range(ns):
        Sg[r, left(r):r + 1] = A[at(r) + left(r):at(r) + r + 1]
        inband[r, left(r):r + 1] = True
    assert np.isfinite(Sg[inband]).all()
    return Sg, inband, barriers


@pytest.mark.parametrize("name,hbs", [("ober70", (None, 15, 16, 17, 31, 32, 33, 139)), ("path12", (None, 16, 23)), ("star41", (81,)),
                                      ("n257", (None, 32, 33))])
def test_selected_inverse_restated_on_the_kernels_layout(est, name, hbs):
    G, b, hb_min = _normal_equations(name, est)
    ns = len(b)
    ref = np.linalg.inv(G)
    cond = np.linalg.cond(G)
    d = np.sqrt(np.diag(ref))
    scale = d[:, None] * d[None, :]
    bound = 100.0 * cond * np.finfo(float).eps
    slack = [s for s in range(ns) if G[s, s] == 1.0 and np.count_nonzero(G[s]) == 1]
    assert slack and all(s % 2 == 1 for s in slack)
    for hb in hbs:
        hb = hb_min if hb is None else hb
        assert hb >= hb_min
        L, _, _, ok = banded_solve(G, b, hb)
        assert ok
        Sg, inband, barriers = band_selinv(L, hb)
        err = (np.abs(Sg - ref) / scale)[inband].max()
        dense = bool(inband[np.tril_indices(ns)].all())
        print(f"[banded selinv] {name} ns={ns} hb={hb} (Wb {-(-hb // NB)}{', the whole lower triangle' if dense else ''}): "
              f"{err:.1e} / {bound:.1e} (100 cond eps, cond {cond:.1e}), {barriers} barriers")
        assert err <= bound
        assert barriers == 4 * ((ns + NB - 1) // NB) + 1
        assert dense or hb < ns - 1                  # dense as a band: the whole lower triangle of the inverse
        for s in slack:
            row, col = Sg[s][inband[s]], Sg[:, s][inband[:, s]]
            assert Sg[s, s] == 1.0 and np.count_nonzero(row) == 1 and np.count_nonzero(col) == 1


# ---- (b) the positions bd_bus asks for

def bd_bus_positions(edge_index, n, G):
    """Per graph the (p, q) state pairs, local, that bd_bus reads Sigma at: from the incidence of the relabelled edge list."""
    ei = edge_index.cpu().numpy()
    out = []
    for g in range(G):
        nb = [set() for _ in range(n)]
        for f, t in ei.T.tolist():
            if g * n <= f < (g + 1) * n and g * n <= t < (g + 1) * n:
                nb[f - g * n].add(t - g * n)          # (a self-loop is its own neighbour, as ws_slot has it)
                nb[t - g * n].add(f - g * n)
        pairs = set()
        for li in range(n):
            group = [li] + sorted(nb[li])
            for a in group:
                for b in group:
                    for sa in (0, 1):
                        for sb in (0, 1):
                            pairs.add((2 * a + sa, 2 * b + sb))
        out.append(pairs)
    return out


@pytest.mark.parametrize("name", ["ober70", "path12", "star41", "n257", "n320", "radial300", RELABELLED, "n100", "ober179"])
def test_bd_bus_stays_inside_the_stored_band(est, name):
    b = bc.batch(name)
    n, N = b["nodes_per_graph"], b["x"].size(0)
    o = est.band_order(b["edge_index"], n, num_nodes=N)
    shift = est.band_blocks(o.half_bandwidth) * NB
    total = worst = 0
    for pairs in bd_bus_positions(o.edge_index, n, N // n):
        for p, q in pairs:
            hi, lo = max(p, q), min(p, q)
            total += 1
            worst = max(worst, hi - lo)
            assert lo >= hi // NB * NB - shift, (name, p, q, o.half_bandwidth)
    print(f"[banded bd_bus positions] {name}: {total} pairs, the widest {worst} states apart, hb {o.half_bandwidth} (stored from {shift} left of a block row)")
    assert worst <= o.half_bandwidth


# ---- (c) the fixtures of the GPU tests

def args(b):
    return b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"]


@functools.lru_cache(maxsize=None)
def clean(name):
    """The oracle on the data as they are, at the comparisons' s_min."""
    return bo.bad_data(*args(bc.batch(name)), s_min=S_MIN_CMP, **FIXED)


# Which measurements carry the gross errors, and how large they are.  The measurement of largest S is the default elsewhere; here the ranks are
# chosen, in the oracle alone, so that the removals are clear: on these trees the top ranks include TWINS -- two injections whose
# normalized residuals agree to 1e-5 whichever of them carries the error (n257 graph 1 at ranks 0, 2 and 4) -- and no implementation can
# be asked which twin it removes.  Three errors get three sizes, so that their own rN are 25 % apart.
ONE_RANK = {"n257": 1, "n320": 2, "radial300": 3, RELABELLED: 1}
THREE_RANKS = {"n257": (1, 3, 4), "n320": (2, 1, 5), "radial300": (3, 1, 5)}
SIGMAS = {1: (25.0,), 3: (30.0, 22.0, 16.0)}
REMOVALS = {1: dict(threshold=4.0, max_removals=3, **FIXED), 3: dict(threshold=4.0, max_removals=5, **FIXED)}
# the graphs whose removals the GPU file compares (asserted below: exactly the clear ones; at most one graph of a batch is not)
CLEAR = {("n257", 1): [0, 1], ("n320", 1): [0, 1], ("radial300", 1): [0, 1], (RELABELLED, 1): [0, 1],
         ("n257", 3): [0], ("n320", 3): [0, 1], ("radial300", 3): [1]}
assert REMOVALS[1] == REMOVAL_KW[(0,)] and REMOVALS[3] == REMOVAL_KW[(0, 1, 2)]      # (tests/test_wls_bad_data_large_cpu.py's settings)


def ranks_of(name, count):
    return (ONE_RANK[name],) if count == 1 else THREE_RANKS[name]


@functools.lru_cache(maxsize=None)
def corrupted(name, count=1):
    """Gross errors at the measurements of the chosen ranks of S, one per rank and graph: (host batch, targets per rank)."""
    b = bc.batch(name)
    x2, ea2, targets = b["x"], b["edge_attr"], []
    for rank, sigmas in zip(ranks_of(name, count), SIGMAS[count]):
        targets.append(bo.largest_sensitivity_targets(*args(b), rank=rank))
        x2, ea2 = bo.add_gross_errors(x2, ea2, b["stats"], targets[-1], sigmas)
    return dict(b, x=x2, edge_attr=ea2), targets


@functools.lru_cache(maxsize=None)
def removal_oracle(name, count=1, perm_seed=None):
    return bo.bad_data(*args(corrupted(name, count)[0]), perm_seed=perm_seed, **REMOVALS[count])


def leads(ref):
    """Per graph the smallest relative lead of a REMOVED measurement over its runner-up (inf where nothing was removed)."""
    out = []
    for g, dec in enumerate(ref["decisions"]):
        taken = dec[:int(ref["n_removed"][g])]
        out.append(min([(best - second) / best for _, best, second in taken], default=float("inf")))
    return out


def clear(name, count=1):
    """Per graph: every decision of the oracle is test_wls_bad_data_large_cpu.decided's and every removal leads by MIN_LEAD."""
    ref = removal_oracle(name, count)
    return [bool(d) and lead >= MIN_LEAD for d, lead in zip(decided(ref), leads(ref))]


@functools.lru_cache(maxsize=None)
def removal_state_spread(name, count=1):
    """Per graph: the worst, over perm_seed 1 and 2, of |fp32(final state) - final state with G summed in a permuted order|."""
    ref = removal_oracle(name, count)
    n = bc.batch(name)["nodes_per_graph"]
    worst = torch.zeros(len(ref["decisions"]), dtype=torch.float64)
    for seed in (1, 2):
        other = removal_oracle(name, count, seed)
        worst = torch.maximum(worst, (ref["state"].float().double() - other["state"]).abs().reshape(-1, 2 * n).max(1).values)
    return worst


@functools.lru_cache(maxsize=None)
def route_spread(name):
    """(S, state_std): the worst absolute difference between the QR route and the normal equations, the latter in the measurements' own
    order and in two permuted ones, at the oracle's state of the clean data."""
    b = bc.batch(name)
    n = b["nodes_per_graph"]
    state = clean(name)["state"]
    e_s = e_std = 0.0
    for g, gr in enumerate(wo.graphs_of(*args(b))):
        u = state[g * n:(g + 1) * n].reshape(-1)
        S, std = bo.sens_qr(gr, u)
        gen = torch.Generator().manual_seed(5 + g)
        for perm in (None, torch.randperm(gr.z.shape[0], generator=gen), torch.randperm(gr.z.shape[0], generator=gen)):
            S2, std2 = bo.sens_normal(gr, u, perm)
            e_s, e_std = max(e_s, float((S - S2).abs().max())), max(e_std, float((std - std2).abs().max()))
    return e_s, e_std


def bounds(name):
    """(S bound, state_std bound): the tree figures of tests/test_gpu_wls_bad_data.py as floors, or 8 x the fp64 routes' own spread where
    that is larger.  Never from the kernel."""
    e_s, e_std = route_spread(name)
    return max(SENS_BOUND, 8.0 * e_s), max(STD_BOUND, 8.0 * e_std)


def rn_bound(name, s_min):
    """The S bound at the floor: in units of max(rN, 1), where the oracle's S >= 2 s_min."""
    return bounds(name)[0] / (2.0 * s_min)


@pytest.mark.parametrize("name", BEYOND + ("ober70", "star41", "path12"))
def test_few_sensitivities_fall_close_to_s_min(name):
    res = clean(name)
    S = torch.cat([res["bus_sens"].reshape(-1), res["edge_sens"].reshape(-1)])
    active = sum(int((gr.w > 0).sum()) for gr in wo.graphs_of(*args(bc.batch(name))))
    near = int(((S >= S_MIN_CMP / 2) & (S <= 2 * S_MIN_CMP)).sum())
    print(f"[banded bad-data s_min] {name}: {near} of {active} active measurements ({100.0 * near / active:.1f} %) have S within a factor 2 of {S_MIN_CMP:.0e}")
    assert near <= 0.1 * active
    assert bool((res["status"] == 1).all()) and bool((res["iterations"] == FIXED["max_iter"]).all()) and bool((res["n_removed"] == 0).all())


@pytest.mark.parametrize("name", BEYOND + ("ober70", "star41", "path12"))
def test_fp64_routes_spread_gives_the_bounds(name):
    e_s, e_std = route_spread(name)
    sens, std = bounds(name)
    print(f"[banded bad-data routes] {name}: S {e_s:.2e} state_std {e_std:.2e} between the fp64 routes -> bounds {sens:.2e}, {std:.2e}; "
          f"rN bound at s_min = {S_MIN_CMP:.0e}: {rn_bound(name, S_MIN_CMP):.2e}, at 1e-3: {rn_bound(name, 1e-3):.2e}")
    assert sens == max(SENS_BOUND, 8.0 * e_s) and std == max(STD_BOUND, 8.0 * e_std)
    assert e_s <= 1e-5 and e_std <= 1e-6            # (an order of magnitude above ober179's would be another problem)


@pytest.mark.parametrize("name,count", sorted(CLEAR))
def test_which_graphs_remove_clearly(name, count):
    hb, targets = corrupted(name, count)
    ref = removal_oracle(name, count)
    ok = clear(name, count)
    print(f"[banded bad-data {count} error(s)] {name}: ranks {ranks_of(name, count)} targets {targets} removed {ref['removed'].tolist()} "
          f"rN {[['%.2f' % v for v in row] for row in ref['removed_rn'].tolist()]} leads {['%.1e' % v for v in leads(ref)]} clear {ok} "
          f"state spread {['%.1e' % v for v in removal_state_spread(name, count).tolist()]}")
    assert [g for g, c in enumerate(ok) if c] == CLEAR[(name, count)]
    assert sum(not c for c in ok) <= 1, "at most one graph of a batch may be left out"
    for g in CLEAR[(name, count)]:
        assert int(ref["n_removed"][g]) == count and leads(ref)[g] >= MIN_LEAD
        # the errors come out in the order of their sizes: rank by rank
        assert ref["removed"][g].tolist() == [t[g] for t in targets] + [-1] * (ref["removed"].shape[1] - count)


def test_a_removed_bus_id_differs_between_the_two_numberings(est):
    """relabelled257: the oracle removes a BUS measurement whose bus the band order moves -- a kernel that reported its own id would fail."""
    hb, _ = corrupted(RELABELLED)
    o = est.band_order(hb["edge_index"], 257, num_nodes=514)
    ref = removal_oracle(RELABELLED)
    N = hb["x"].shape[0]
    moved = [int(i) for g, i in enumerate(ref["removed"][:, 0].tolist()) if clear(RELABELLED)[g] and 0 <= i < 4 * N and int(o.inverse[i // 4]) != i // 4]
    print(f"[banded bad-data labels] removed {ref['removed'][:, 0].tolist()}: bus ids whose row moves under the band order {moved}")
    assert moved


# ---- (c') the Huber form's fixtures: tests/test_gpu_wls_robust.py's bounds, from the oracle's own spread over summation orders

HUBER_ITERS, HUBER_SEEDS = 8, (1, 2, 3, 4)
HUBER_STATE_FLOOR, HUBER_Q_FLOOR, HUBER_OBJ_BOUND = 5e-7, 1e-9, 1e-6      # tests/test_gpu_wls_robust.py's


@functools.lru_cache(maxsize=None)
def huber_oracle(name, perm_seed=None, gamma=ro.GAMMA):
    """wls_robust_oracle.solve_huber on corrupted(name) (one error of 25 sigma per graph), HUBER_ITERS iterations, tol = 0."""
    return ro.solve_huber(*args(corrupted(name)[0]), max_iter=HUBER_ITERS, tol=0.0, perm_seed=perm_seed, gamma=gamma)


@functools.lru_cache(maxsize=None)
def huber_bounds(name):
    """(state, q): max(the floor, 8 x the worst difference between the oracle and itself with G summed in four permuted orders)."""
    ref = huber_oracle(name)
    e_st = e_q = 0.0
    for seed in HUBER_SEEDS:
        other = huber_oracle(name, seed)
        e_st = max(e_st, (ref["state"].float().double() - other["state"]).abs().max().item())
        e_q = max(e_q, (ref["bus_q"] - other["bus_q"]).abs().max().item(), (ref["edge_q"] - other["edge_q"]).abs().max().item())
    return max(HUBER_STATE_FLOOR, 8.0 * e_st), max(HUBER_Q_FLOOR, 8.0 * e_q)


@pytest.mark.parametrize("name", ["n257", "radial300"])
def test_huber_fixtures(name):
    ref = huber_oracle(name)
    sb, qb = huber_bounds(name)
    near = ro.near_threshold(ref)
    print(f"[banded huber fixtures] {name}: state bound {sb:.2e} q bound {qb:.2e}; down-weighted {ref['n_downweighted'].tolist()} "
          f"within 1e-6 gamma of gamma {near}; cost {ref['objective'].sum(1).tolist()}")
    assert sum(near) == 0                           # (nothing has to be left out of the comparison of the sets {q < 1})
    assert bool((ref["n_downweighted"] >= 1).all()) and bool((ref["status"] == 1).all())
    assert sb <= 1e-5 and qb <= 1e-5


# ---- (d) the host side

def test_size_formulas_with_the_bad_data_block(est):
    L = load_pkg()._lib
    assert L.WLS_BAND_BAD_DATA_BYTES == 4 * 8 + 4 * 4 + 4 * 4 + 64 * 4 == 320       # red_v, red_i, red_c, rem
    # by hand, n = 257, hb = 19 (Wb = 2): the panel 16 x 40, Ld 256, invd 16, u and du 2 x 514 doubles; 16 bytes of control words; 257
    # slack flags in 272 bytes; then the bad-data block
    assert est.band_lds_bytes(257, 19, bad_data=True) == (16 * 40 + 256 + 16 + 4 * 257) * 8 + 16 + 272 + 320 == 16128
    assert est.band_lds_bytes(257, 19, True) == est.band_lds_bytes(257, 19) + 320 and est.band_lds_bytes(257, 19, False) == est.band_lds_bytes(257, 19)
    f = lambda n, hb: est.band_lds_bytes(n, hb, bad_data=True)
    for n in (1, 70, 257, 1000):
        vals = [f(n, hb) for hb in range(1, 300)]
        assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[0] < vals[-1]
    for hb in (1, 19, 69, 241):
        vals = [f(n, hb) for n in range(1, 1200)]
        assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[0] < vals[-1]
    for n in (257, 300, 1000, 4000):
        cap = est.band_max_half_bandwidth(n, bad_data=True)
        assert cap % 16 == 0 and f(n, cap) <= L.WLS_BAND_LDS_BYTES < f(n, cap + 1)
        assert cap <= est.band_max_half_bandwidth(n)
    assert est.band_max_half_bandwidth(300, True) >= 69 and est.band_max_half_bandwidth(1000, True) >= 241
    assert est.band_max_half_bandwidth(10 ** 5, True) == 0


def test_struct_mirror_and_python_side_without_a_gpu(est, monkeypatch):
    pkg = load_pkg()
    lib = pkg._lib
    cls = lib.WlsBadDataArgs
    assert ("bus_label", ctypes.c_void_p) in cls._fields_ and cls().bus_label is None
    assert cls._fields_[-2:] == [("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_uint64)]
    for name, like, dropped in (("wls_bad_data_banded", est.wls_bad_data_large, ()), ("wls_robust_banded", est.wls_robust, ("large",))):
        fn = getattr(est, name)
        assert getattr(pkg, name) is fn and name in pkg.__all__
        want = [p for p in inspect.signature(like).parameters if p not in dropped] + ["order"]
        assert list(inspect.signature(fn).parameters) == want and inspect.signature(fn).parameters["order"].default is None
        for p, v in inspect.signature(like).parameters.items():
            if p not in dropped:
                assert inspect.signature(fn).parameters[p].default == v.default, (name, p)
    b = bc.batch("n257")
    for fn in (est.wls_bad_data_banded, est.wls_robust_banded):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 257)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 257, order=est.band_order(b["edge_index"], 257, num_nodes=514))
    # with the device check out of the way a host batch reaches every ValueError and then the size refusal, and nothing beyond it
    o = est.band_order(b["edge_index"], 257, num_nodes=514)
    cap, cap_bd = est.band_max_half_bandwidth(257), est.band_max_half_bandwidth(257, bad_data=True)
    call = lambda fn, order=o, **kw: fn(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 257, order=order, **kw)
    with monkeypatch.context() as m:
        m.setattr(est, "_require_gpu", lambda *tensors: None)
        with pytest.raises(NotImplementedError, match=f"wls_bad_data_banded .* hb of at most {cap_bd} states, got hb = {cap_bd + 1}"):
            call(est.wls_bad_data_banded, o._replace(half_bandwidth=cap_bd + 1))
        with pytest.raises(NotImplementedError, match=f"wls_robust_banded .* hb of at most {cap} states, got hb = {cap + 1}"):
            call(est.wls_robust_banded, o._replace(half_bandwidth=cap + 1))
        foreign = est.band_order(bc.batch("n320")["edge_index"], 320, num_nodes=640)
        for fn in (est.wls_bad_data_banded, est.wls_robust_banded):
            with pytest.raises(ValueError, match="order was made for"):
                call(fn, foreign)
        for kw in (dict(threshold=0.0), dict(max_removals=65), dict(confidence=1.0), dict(s_min=0.0)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                call(est.wls_bad_data_banded, **kw)
        for kw in (dict(gamma=0.0), dict(plain_iters=-1)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                call(est.wls_robust_banded, **kw)
    assert "needs the dense covariance" not in est.wls_estimate_banded.__doc__ and "no Huber form" not in est.__doc__


def test_evaluate_wls_still_refuses_what_the_band_cannot_serve():
    pkg = load_pkg()
    stats = lc.batch("n33")["stats"]
    for kw in (dict(bad_data=dict(threshold=3.0)), dict(robust=dict(gamma=3.0))):
        with pytest.raises(ValueError, match="banded"):
            pkg.runner.evaluate_wls([], stats, 300, banded="yes", **kw)
        assert pkg.runner.evaluate_wls([], stats, 300, banded="auto", **kw)["wls_not_converged"] == 0
    with pytest.raises(ValueError, match="two answers"):
        pkg.runner.evaluate_wls([], stats, 300, banded=True, bad_data=dict(threshold=3.0), robust=dict(gamma=3.0))
