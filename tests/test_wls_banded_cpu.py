"""CPU: the host side of the banded WLS estimator (estimator.band_order and the size formulas of estimator.wls_estimate_banded) and the
banded factorisation of csrc/dss2_wls_banded.hpp restated in numpy on its storage layout.

  (a) band_order on a path, a star with 40 leaves, cigre14_reswitched (a cycle), ober_sub, the 257-bus tree and a randomly relabelled
      copy of it: a permutation per graph; the reported hb equals a brute-force bandwidth of the relabelled 2-hop pattern (dense A^2);
      the path comes out at 2 buses; two calls agree; equal topologies share one ordering; half_bandwidth= raises hb and is refused below
      the minimum; the edge list keeps its order and orientation.
  (b) the dense fp64 oracle on the relabelled batch, un-permuted, equals the oracle on the original within the oracle's own spread over
      summation orders: relabelling changes nothing but rounding.
  (c) the Python workspace and LDS formulas against a hand count for n = 257, hb = 19, monotone in n and hb, equal to the header's
      constants; the cap.
  (d) the kernel's steps on the kernel's arrays (the band rows, the right-hand side behind them, the panel with a row's place counted
      from the panel's first row, starting as NaN) against LAPACK, at band edges: hb at the minimum, at multiples of 16 and one beside
      them, and dense as a band.
"""
import math

import numpy as np
import pytest
import torch

import abi_probe
import wls_banded_cases as bc
import wls_edge_cases as we
import wls_large_cases as lc
import wls_oracle as wo
from conftest import load_pkg

NB, TILE = 16, 8
ORDER_CASES = ["path12", "star41", "mixed8", "ober_sub", "n257", "relabelled257"]


@pytest.fixture(scope="module")
def est():
    return load_pkg().estimator


def _order(est, name, **kw):
    b = bc.batch(name)
    return est.band_order(b["edge_index"], b["nodes_per_graph"], num_nodes=b["x"].size(0), **kw)


@pytest.mark.parametrize("name", ORDER_CASES)
def test_band_order_is_a_permutation_with_the_exact_bandwidth(est, name):
    b = bc.batch(name)
    n, N = b["nodes_per_graph"], b["x"].size(0)
    o = _order(est, name)
    perm, inv = o.perm.long(), o.inverse.long()
    assert o.perm.dtype == torch.int32 and o.topology is None and o.nodes_per_graph == n
    assert torch.equal(perm.sort().values, torch.arange(N)) and torch.equal(perm[inv], torch.arange(N))
    assert torch.equal(perm // n, torch.arange(N) // n), "a bus left its graph"
    # stored order and orientation kept: edge e still joins the same two buses, from -> to
    assert o.edge_index.dtype == b["edge_index"].dtype and torch.equal(perm[o.edge_index], b["edge_index"])
    brute = bc.brute_force_half_bandwidth(o.edge_index, n, N)
    before = bc.brute_force_half_bandwidth(b["edge_index"], n, N)
    print(f"[band order] {name}: hb {o.half_bandwidth} (brute force {brute}; the caller's numbering {before}), {o.n_orderings} ordering(s) for {N // n} graphs")
    assert o.half_bandwidth == brute <= before
    again = _order(est, name)
    assert all(torch.equal(p, q) for p, q in zip(o[:3], again[:3])) and o[4:] == again[4:]
    ident = _order(est, name, identity=True)
    assert ident.half_bandwidth == before and torch.equal(ident.perm.long(), torch.arange(N)) and torch.equal(ident.edge_index, b["edge_index"])


def test_band_order_known_answers(est):
    assert _order(est, "path12").half_bandwidth == 2 * 2 + 1                 # a path: 2 buses
    assert _order(est, "star41").half_bandwidth == 2 * 40 + 1                # every bus within two branches of every other
    assert _order(est, "n257").half_bandwidth == 2 * 9 + 1                   # the issue's measurement: 9 buses
    assert _order(est, "radial300").half_bandwidth == 69
    # equal topologies share one ordering; the mixed batch has two
    assert _order(est, "n257").n_orderings == 1 and _order(est, "mixed8").n_orderings == 2 and _order(est, "relabelled257").n_orderings == 2
    o = _order(est, "n257")
    assert torch.equal(o.perm[257:].long() - 257, o.perm[:257].long())
    # one-bus graphs without a branch: hb = 1
    one = est.band_order(torch.zeros(2, 0, dtype=torch.long), 1, num_nodes=3)
    assert one.half_bandwidth == 1 and one.perm.tolist() == [0, 1, 2]


def test_half_bandwidth_can_be_raised_not_lowered(est):
    o = _order(est, "n257")
    assert _order(est, "n257", half_bandwidth=o.half_bandwidth).half_bandwidth == o.half_bandwidth
    up = _order(est, "n257", half_bandwidth=64)
    assert up.half_bandwidth == 64 and torch.equal(up.perm, o.perm)
    with pytest.raises(ValueError, match=f"below the {o.half_bandwidth} states"):
        _order(est, "n257", half_bandwidth=o.half_bandwidth - 1)
    with pytest.raises(ValueError, match="crosses graphs"):
        est.band_order(torch.tensor([[0], [5]]), 3, num_nodes=6)
    with pytest.raises(ValueError, match="whole graphs"):
        est.band_order(torch.tensor([[0], [1]]), 3, num_nodes=7)


@pytest.mark.parametrize("name", ["n257", "relabelled257", "mixed8"])
def test_relabelling_changes_nothing_but_rounding(est, name):
    b = bc.batch(name)
    o = _order(est, name)
    moved = bc.relabel(b, o.inverse.long())
    assert torch.equal(moved["edge_index"], o.edge_index)
    for max_iter in (1, 8):
        ref = bc.oracle(name, max_iter, 0.0)
        got = wo.solve(*we.args(moved), max_iter=max_iter, tol=0.0)
        back = got["state"][o.inverse.long()]
        sp = bc.spread(name, max_iter, 0.0)          # the project's measure: |fp32(oracle state) - permuted-order state|, four orders
        err = (back - ref["state"]).abs().max().item()
        obj = ((got["objective"] - ref["objective"]).abs() / ref["objective"].abs()).max().item()
        print(f"[band relabel] {name} max_iter={max_iter}: state {err:.2e} against the oracle's own spread {sp:.2e}; objective {obj:.2e}")
        assert err <= sp and obj <= bc.OBJ_BOUND
        assert torch.equal(got["iterations"], ref["iterations"]) and torch.equal(got["status"], ref["status"])


def test_size_formulas(est):
    L = load_pkg()._lib
    # (tests/test_abi_cpu.py holds the three mirrors to the header's DSS2_WLS_BAND_* values)
    assert {"WLS_BAND_BLOCK", "WLS_BAND_GROUPS", "WLS_BAND_LDS_BYTES"} <= abi_probe.header_constants()
    assert (L.WLS_BAND_BLOCK, L.WLS_BAND_GROUPS, L.WLS_BAND_LDS_BYTES) == (16, 512, 160 * 1024)
    # by hand, n = 257, hb = 19: Wb = 2; 514 states = 33 block rows of 16 rows of 48 doubles, and 33 * 16 doubles of right-hand side
    assert est.band_blocks(19) == 2 and est.band_blocks(16) == 1 and est.band_blocks(17) == 2 and est.band_blocks(1) == 1
    assert est.band_workspace_bytes(257, 19, 1) == (33 * 16 * 48 + 33 * 16) * 8 == 206976
    assert est.band_workspace_bytes(257, 19, 3) == 3 * 206976
    # LDS: the panel 16 x (32 + 8), Ld 256, invd 16, u and du 2 * 514 doubles; 16 bytes of control words; 257 slack flags in 272 bytes
    assert est.band_lds_bytes(257, 19) == (16 * 40 + 256 + 16 + 4 * 257) * 8 + 16 + 272 == 15808
    assert est.band_groups(3) == 3 and est.band_groups(3, 2) == 2 and est.band_groups(4096) == 512 and est.band_groups(4096, 600) == 512
    for f in (est.band_lds_bytes, lambda n, hb: est.band_workspace_bytes(n, hb, 1)):
        for n in (1, 70, 257, 1000):
            vals = [f(n, hb) for hb in range(1, 300)]
            assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[0] < vals[-1]
        for hb in (1, 19, 69, 241):
            vals = [f(n, hb) for n in range(1, 1200)]
            assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[0] < vals[-1]
    # the cap: the largest hb that fits, and the issue's grids are inside it
    for n in (257, 300, 1000, 4000):
        cap = est.band_max_half_bandwidth(n)
        assert cap % 16 == 0 and est.band_lds_bytes(n, cap) <= L.WLS_BAND_LDS_BYTES < est.band_lds_bytes(n, cap + 1)
    assert est.band_max_half_bandwidth(300) >= 69 and est.band_max_half_bandwidth(1000) >= 241
    assert est.band_max_half_bandwidth(10 ** 5) == 0
    b = bc.batch("n257")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_estimate_banded(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 257)
    assert load_pkg().synthetic.load_grid(load_pkg().synthetic.register_radial(1000)).n == 1000


# ---- (d) the banded factorisation of csrc/dss2_wls_banded.hpp on its storage layout

def banded_solve(G, b, hb):
    """(L [ns, ns], y, du, ok) by the kernel's steps on the kernel's arrays."""
    ns = len(b)
    Wb = -(-hb // NB)
    W, shift, nbr = NB * (Wb + 1), NB * Wb, -(-ns // NB)
    A = np.zeros(nbr * NB * W + NB * nbr)
    rhs = nbr * NB * W

    def at(r):                                      # the offset of row r's column 0
        return r * W + shift - r // NB * NB

    def left(r):
        return max(0, r // NB * NB - shift)

    for r in range(ns):
        assert not G[r, :left(r)].any(), "a non-zero outside the declared band"
        assert at(r) + left(r) >= r * W and at(r) + r < (r + 1) * W
        A[at(r) + left(r):at(r) + r + 1] = G[r, left(r):r + 1]
    A[rhs:rhs + ns] = b
    S = NB * Wb + TILE
    Pt = np.full((NB, S), np.nan)
    ok = True
    for j0 in range(0, ns, NB):
        w = min(NB, ns - j0)
        first = j0 + w
        end = min(ns, first + shift)
        row = lambda i: rhs if i == end else at(i)
        D = np.zeros((NB, NB))
        for i in range(w):
            D[i, :i + 1] = A[at(j0 + i) + j0:at(j0 + i) + j0 + i + 1]
        for j in range(NB):
            d = D[j, j]
            good = d > 0 and math.isfinite(d)
            if j < w:
                ok = ok and good
            s = math.sqrt(d) if good else 1.0
            D[j + 1:, j] /= s
            D[j, j] = s
            for k in range(j + 1, NB):
                D[k:, k] -= D[k:, j] * D[k, j]
        Ld = np.zeros((NB, NB))
        for i in range(w):
            Ld[i, :i + 1] = D[i, :i + 1]
            A[at(j0 + i) + j0:at(j0 + i) + j0 + i + 1] = D[i, :i + 1]
        invd = 1.0 / np.diag(D)
        Pt[:] = np.nan                              # (nothing of an earlier panel may be needed)
        for i in range(first, end + 1):
            x = A[row(i) + j0:row(i) + j0 + NB].copy()
            for j in range(NB):
                x[j] *= invd[j]
                x[j + 1:] -= x[j] * Ld[j + 1:, j]
            A[row(i) + j0:row(i) + j0 + NB] = x
            Pt[:, i - first] = x
        if first < ns:
            ntr = (end + 1 - first + TILE - 1) // TILE
            for ti in range(ntr):
                for tj in range(ti + 1):
                    i0, c0 = first + TILE * ti, first + TILE * tj
                    assert i0 - first + TILE <= S
                    with np.errstate(invalid="ignore"):
                        acc = Pt[:, i0 - first:i0 - first + TILE].T @ Pt[:, c0 - first:c0 - first + TILE]
                    for q in range(TILE):
                        i = i0 + q
                        for c in range(TILE):
                            if i <= end and c0 + c <= i and c0 + c < end:
                                assert i == end or c0 + c >= left(i)
                                A[row(i) + c0 + c] -= acc[q, c]
    assert np.isfinite(A).all()
    L = np.zeros((ns, ns))
    for r in range(ns):
        L[r, left(r):r + 1] = A[at(r) + left(r):at(r) + r + 1]
    y = A[rhs:rhs + ns].copy()
    du = y.copy()
    for j0 in range((ns - 1) // NB * NB, -1, -NB):
        w = min(NB, ns - j0)
        for j in range(w - 1, -1, -1):
            xj = du[j0 + j] * (1.0 / A[at(j0 + j) + j0 + j])
            du[j0 + j] = xj
            for k in range(j):
                du[j0 + k] -= A[at(j0 + j) + j0 + k] * xj
        for c in range(left(j0), j0):
            for j in range(w):
                du[c] -= A[at(j0 + j) + c] * du[j0 + j]
    return L, y, du, ok


def _normal_equations(name, est):
    b = bc.batch(name)
    o = est.band_order(b["edge_index"], b["nodes_per_graph"], num_nodes=b["x"].size(0))
    gr = wo.graphs_of(*we.args(bc.relabel(b, o.inverse.long())))[0]
    u = torch.zeros(2 * gr.n, dtype=torch.float64)
    u[0::2] = 1.0
    Gm, rhs = gr.normal_equations(u)
    return Gm.numpy(), rhs.numpy(), o.half_bandwidth


@pytest.mark.parametrize("name,hbs", [("n257", (None, 32, 33)), ("ober70", (None, 15, 16, 17, 31, 32, 33, 139)), ("star41", (None,)),
                                      ("path12", (None, 16, 23))])
def test_banded_factorisation_restated_on_the_kernels_layout(est, name, hbs):
    G, b, hb_min = _normal_equations(name, est)
    ns = len(b)
    r, c = np.nonzero(G)
    assert (r - c).max() <= hb_min, "the gain matrix of the relabelled graph leaves the band band_order reports"
    Lref = np.linalg.cholesky(G)
    ref_du = np.linalg.solve(G, b)
    cond = np.linalg.cond(G)
    for hb in hbs:
        hb = hb_min if hb is None else hb
        if hb < hb_min:
            continue
        L, y, du, ok = banded_solve(G, b, hb)
        assert ok
        scale = np.sqrt(np.diag(G))[:, None]
        err_L = (np.abs(L - Lref) / scale).max()
        resid = np.abs(L @ L.T - G).max() / np.abs(G).max()
        err_du = np.abs(du - ref_du).max() / np.abs(ref_du).max()
        back = np.abs(G @ du - b).max() / (np.abs(G).max() * np.abs(du).max() + np.abs(b).max())
        err_y = np.abs(y - np.linalg.solve(Lref, b)).max() / np.abs(y).max()
        print(f"[wls banded restatement] {name} ns={ns} hb={hb}: L {err_L:.1e} residual {resid:.1e} y {err_y:.1e} du {err_du:.1e} (cond {cond:.1e}) backward {back:.1e}")
        assert resid <= 1e-13 and back <= 1e-13
        assert err_L <= 1e-6 and err_y <= 1e-6
        assert err_du <= 100.0 * cond * np.finfo(float).eps
