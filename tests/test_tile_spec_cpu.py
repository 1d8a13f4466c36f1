"""CPU: the tile selection of topology.py -- the height rule, the two producers of a TileSpec, the entry-count policy and the rule of
which statistic words a tiling's launches write -- against the structure oracle (oracle/dss2_topology_oracle.py).  Pure functions: no
device, no library call."""
import functools

import numpy as np
import pytest
import torch

import dss2_topology_oracle as topo_oracle
from conftest import load_pkg

T = load_pkg().topology
CHOICES = T._NRB_CHOICES
HEIGHTS = [None, 1, 2, 3, 6]
GRID_POINTS = ([(("cigre14",), B) for B in (1, 2, 3, 4, 5, 7, 8, 9, 64, 515)] + [(("cigre14", "cigre14_reswitched"), B) for B in (6, 13)]
               + [(("ober_sub",), B) for B in (1, 2, 3, 37)] + [(("ober179",), B) for B in (1, 5)])


@functools.lru_cache(maxsize=None)
def _grid_batch(grids, B, seed):
    pkg = load_pkg()
    b = pkg.synthetic.make_batch(list(grids), B, seed=seed)
    return b["edge_index"], b["x"].shape[0], max(pkg.synthetic.load_grid(g).e for g in grids)


def _stars(n_graphs, leaves=11):
    n = leaves + 1
    return torch.cat([torch.stack([torch.zeros(leaves, dtype=torch.int64), torch.arange(1, n)]) + k * n for k in range(n_graphs)], 1), n_graphs * n


def _star_hint(directed=True):
    return T.TopologyHint(directed=directed, nodes_per_graph=12, max_degree=11, max_edges_per_graph=11, edges_per_graph=11)


def _walk_stats(ref, choices):
    """What dss2_tiles_walk and the CSR build leave in the 16 words, from the oracle: the dictionary Topology._read_stats returns."""
    seg = np.diff(ref.bounds)
    nts = [(0 if ts is None else len(ts) - 1) for ts in (topo_oracle.pack_tiles(ref.bounds, 32 * c) for c in choices)]
    return dict(max_deg=ref.max_deg, max_degT=ref.max_degT, max_segment=int(seg.max()), n_segments=len(seg), min_segment=int(seg.min()),
                error=0, max_nnz=0, max_nnzT=0, ntiles_cand=nts + [0] * (8 - len(nts)))


@pytest.mark.parametrize("nrb", HEIGHTS, ids=lambda h: f"nrb{h}")
@pytest.mark.parametrize("grids,B", GRID_POINTS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_closed_form_spec_equals_the_oracle(grids, B, nrb):
    ei, N, e_max = _grid_batch(grids, B, 5)
    ref = topo_oracle.TopologyOracle(ei, N, nrb=nrb)
    hint = T.TopologyHint(directed=True, nodes_per_graph=N // B, max_degree=max(ref.max_deg, ref.max_degT), max_edges_per_graph=e_max)
    spec = T.spec_from_hint(hint, N, True, (nrb,) if nrb else CHOICES)
    if not ref.tiled:
        assert spec is None
        return
    assert (spec.nrb, spec.ntiles, spec.ell, spec.ellT, spec.max_segment) == (ref.nrb, ref.ntiles, ref.ell, ref.ellT, ref.max_segment)
    assert abs(spec.utilisation - ref.utilisation) < 1e-12
    per = (32 * spec.nrb) // (N // B)
    assert spec.uniform_rows == spec.max_tile_rows == per * (N // B) and spec.walk_index is None
    assert ref.tile_start.tolist() == [min(t * spec.uniform_rows, N) for t in range(spec.ntiles + 1)]
    assert spec.nnz == T.NNZ_HINT and spec.max_nnz == spec.max_nnzT == per * e_max * 2 and spec.max_nnz >= max(ref.max_nnz, ref.max_nnzT)


def _walk_cases():
    ei, N, _ = _grid_batch(("cigre14", "ober_sub"), 21, 7)
    chain = torch.stack([torch.arange(399), torch.arange(1, 400)])
    return {"mixed21": (ei, N), "stars7": _stars(7), "stars16": _stars(16), "chain400": (chain, 400)}


@pytest.mark.parametrize("nrb", HEIGHTS, ids=lambda h: f"nrb{h}")
@pytest.mark.parametrize("name", ["mixed21", "stars7", "stars16", "chain400"])
def test_walked_spec_equals_the_oracle(name, nrb):
    ei, N = _walk_cases()[name]
    choices = (nrb,) if nrb else CHOICES
    ref = topo_oracle.TopologyOracle(ei, N, nrb=nrb)
    spec = T.spec_from_stats(_walk_stats(ref, choices), N, choices)
    if not ref.tiled:
        assert spec is None
        return
    assert name != "chain400"
    assert (spec.nrb, spec.ntiles, spec.ell, spec.ellT, spec.max_segment) == (ref.nrb, ref.ntiles, ref.ell, ref.ellT, ref.max_segment)
    assert abs(spec.utilisation - ref.utilisation) < 1e-12
    assert spec.uniform_rows == 0 and choices[spec.walk_index] == ref.nrb
    seg = np.diff(ref.bounds)
    if seg.min() == seg.max():
        assert spec.max_tile_rows == (32 * ref.nrb) // int(seg.max()) * int(seg.max()) > 0
    else:
        assert name == "mixed21" and spec.max_tile_rows == 0


def test_height_rule_margin_and_tie_order():
    # equal utilisation: the first of the choices wins, whatever the order; a later one needs more than 0.03
    assert T.best_height(128, (2, 4), lambda c: 128 // (32 * c)) == (1.0, 2, 2)
    assert T.best_height(128, (4, 2), lambda c: 128 // (32 * c)) == (1.0, 4, 1)
    nt = {2: 100, 3: 65}        # 6000 rows: 0.9375 at 64 rows, 0.9615 at 96: inside the margin, 64 rows stay
    assert T.best_height(6000, (2, 3), nt.__getitem__)[1] == 2
    nt = {2: 100, 3: 64}        # 0.9766 at 96 rows: outside it
    assert T.best_height(6000, (2, 3), nt.__getitem__)[1] == 3
    assert T.best_height(400, CHOICES, lambda c: 0) is None


def test_entry_count_policy_has_three_kinds():
    # a bound from the hint (here exact: every star is full)
    ei, N = _stars(16)
    for h, want in [(None, 176), (1, 44), (2, 110), (4, 220), (6, 352)]:
        ref = topo_oracle.TopologyOracle(ei, N, nrb=h)
        spec = T.spec_from_hint(_star_hint(), N, True, (h,) if h else CHOICES)
        assert ref.nrb == spec.nrb == (h or 3) and (ref.ell, ref.ellT) == (spec.ell, spec.ellT) == (0, 0)
        assert spec.nnz == T.NNZ_HINT and (spec.max_nnz, spec.max_nnzT) == (ref.max_nnz, ref.max_nnzT) == (want, want)
    assert T.spec_from_hint(_star_hint(directed=False), N, False, (3,)).max_nnz == 88       # (the list as given: not doubled)
    # read back after the launch: hub graphs without a hint -- nothing known before it (the launch will report the oracle's 154)
    ei, N = _stars(7)
    ref = topo_oracle.TopologyOracle(ei, N)
    spec = T.spec_from_stats(_walk_stats(ref, CHOICES), N, CHOICES)
    assert spec.nnz == T.NNZ_READBACK and (spec.max_nnz, spec.max_nnzT) == (0, 0) and (ref.max_nnz, ref.max_nnzT) == (154, 154)
    # max_deg * tm where ELL slices exist both ways
    ei, N, _ = _grid_batch(("cigre14", "ober_sub"), 21, 7)
    ref = topo_oracle.TopologyOracle(ei, N)
    spec = T.spec_from_stats(_walk_stats(ref, CHOICES), N, CHOICES)
    assert spec.ell > 0 and spec.ellT > 0 and spec.nnz == T.NNZ_ELL
    assert (spec.max_nnz, spec.max_nnzT) == (ref.max_deg * 32 * ref.nrb, ref.max_degT * 32 * ref.nrb) and spec.max_nnz >= ref.max_nnz
    # one width above 8 is enough for the read-back: the tile kernels then stage CSR slices
    s = dict(_walk_stats(ref, CHOICES), max_degT=9)
    spec = T.spec_from_stats(s, N, CHOICES)
    assert (spec.ell > 0, spec.ellT) == (True, 0) and spec.nnz == T.NNZ_READBACK


def test_statistic_word_ownership_table():
    want = {  # (primary, closed form, has ELL slices)
        (True, True, True): "own", (True, True, False): "own", (True, False, True): "own", (True, False, False): "own",
        (False, False, True): "copy", (False, False, False): "copy",      # walked alternates: the walk and the ELL launch post maxima
        (False, True, True): "own",                                      # posts no statistic (uniform_rows > 0), only the hint's error flag
        (False, True, False): None,                                      # the hinted hub alternate: no launch at all
    }
    got = {k: T.stat_words(*k) for k in want}
    assert got == want
    # the words an ELL launch may write are the error flag and the two entry maxima, and the table is the header's
    assert T._WORDS == dict(max_deg=0, max_degT=1, max_segment=2, n_segments=3, min_segment=4, error=5, max_nnz=6, max_nnzT=7, ntiles_cand=8)
    assert list(range(16))[T._PER_TILING] == [5, 6, 7]
