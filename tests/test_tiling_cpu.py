"""CPU: ``topology.Tiling`` built directly from CPU tensors, and what the three fillers of kernel graph arguments write from it
(``ops._fill_graph`` for GemmPropArgs, ``ops._fill_wgrad_graph`` for WgradArgs, ``stack._fill_common`` for StackArgs), field by field.

No GPU and no ``Topology``: a stub with the CSR arrays stands in for the topology, and where a whole wrapper runs (``gemm_prop`` /
``gemm_prop_chain``, for the one field only the chain sets) a recorder stands in for the library and keeps the args struct of every
launch.  Every array has its own storage, so a pointer identifies the array it came from; every width and count differs between the
by-target and by-source side and between the primary and the alternate tiling, so a mixed-up pairing cannot pass."""
import importlib
import types

import torch

from conftest import load_pkg

N = 120          # 8 graphs of 15 nodes
CSR = ("rowptr", "col", "ent", "w", "rowptrT", "colT", "entT", "wT")


def _tiling(pkg, nrb, ell, ellT, max_nnz, max_nnzT, rows):
    tm = 32 * nrb
    ntiles = -(-N // rows)

    def slab(width):
        return torch.zeros(ntiles, width, tm, 2, dtype=torch.int32) if width else None
    return pkg.topology.Tiling(global_only=False, nrb=nrb, ntiles=ntiles, tile_start=torch.arange(ntiles + 1, dtype=torch.int32) * rows,
                               utilisation=N / float(ntiles * tm), max_segment=15, max_tile_rows=rows, max_nnz=max_nnz, max_nnzT=max_nnzT,
                               ell=ell, ellT=ellT, ell_tiles=slab(ell), ellT_tiles=slab(ellT), ell_ent_tiles=slab(ell), ellT_ent_tiles=slab(ellT))


def _topo(primary, alternates=()):
    arrays = {name: torch.zeros(N + 1, dtype=(torch.float32 if name in ("w", "wT") else torch.int32)) for name in CSR}
    alts = {ts.nrb: ts for ts in alternates}
    return types.SimpleNamespace(N=N, hint=None, device=torch.device("cpu"), tiling=primary, deg_pows=torch.zeros(N, 4),
                                 tiles_for=lambda nrb: primary if nrb == primary.nrb else alts.get(nrb), **arrays)


def test_a_tiling_is_a_plain_record_with_its_own_caches():
    pkg = load_pkg()
    a, b = _tiling(pkg, 2, 3, 4, 192, 256, 60), _tiling(pkg, 1, 3, 4, 96, 128, 30)
    assert (a.nrb, a.ntiles, a.ell, a.ellT, a.max_nnz, a.max_nnzT, a.max_tile_rows) == (2, 2, 3, 4, 192, 256, 60)
    assert tuple(a.ell_tiles.shape) == (2, 3, 64, 2) and tuple(b.ellT_ent_tiles.shape) == (4, 4, 32, 2)
    assert a.gain_bits == {} and a.gain_bits is not b.gain_bits and not hasattr(a, "gate_words")      # (the chain's words come with its plan)
    assert not hasattr(a, "__dict__")      # (slots: a misspelt field is an error, not a new attribute)


def test_fill_graph_takes_the_csr_from_the_topology_and_the_rest_from_the_tiling():
    pkg = load_pkg()
    ts = _tiling(pkg, 2, 3, 4, 192, 256, 60)
    topo = _topo(ts)
    for transposed, csr, nnz, width, tiles in ((False, ("rowptr", "col", "w"), 192, 3, ts.ell_tiles),
                                               (True, ("rowptrT", "colT", "wT"), 256, 4, ts.ellT_tiles)):
        a = pkg._lib.GemmPropArgs()
        pkg.ops._fill_graph(a, topo, ts, transposed)
        assert (a.nrb, a.ntiles, a.tile_start) == (2, ts.ntiles, ts.tile_start.data_ptr())
        assert (a.rowptr, a.col, a.w) == tuple(getattr(topo, n).data_ptr() for n in csr)
        assert (a.max_nnz, a.ell_width, a.ell_tiles) == (nnz, width, tiles.data_ptr())
        assert a.max_tile_rows == 0      # (the layer chain's alone)


def test_fill_graph_passes_null_ell_tiles_at_width_zero():
    pkg = load_pkg()
    ts = _tiling(pkg, 2, 0, 0, 700, 900, 60)      # a hub bus: CSR staging, exact sizes
    assert ts.ell_tiles is None and ts.ellT_tiles is None
    topo = _topo(ts)
    for transposed, nnz in ((False, 700), (True, 900)):
        a = pkg._lib.GemmPropArgs()
        pkg.ops._fill_graph(a, topo, ts, transposed)
        assert (a.ell_width, a.ell_tiles, a.max_nnz) == (0, None, nnz)
    w = pkg._lib.WgradArgs()
    pkg.ops._fill_wgrad_graph(w, topo, ts)
    assert (w.ell_width, w.ell_tiles, w.max_nnz) == (0, None, 900)


def test_fill_wgrad_graph_mixes_the_topologys_csr_with_the_walked_tiling():
    pkg = load_pkg()
    primary, alt = _tiling(pkg, 2, 3, 4, 192, 256, 60), _tiling(pkg, 1, 3, 5, 96, 160, 30)
    topo = _topo(primary, (alt,))
    for ts in (primary, alt):
        a = pkg._lib.WgradArgs()
        pkg.ops._fill_wgrad_graph(a, topo, ts)
        assert (a.rowptrT, a.colT, a.wT) == (topo.rowptrT.data_ptr(), topo.colT.data_ptr(), topo.wT.data_ptr())
        assert (a.nrb, a.ntiles, a.tile_start) == (ts.nrb, ts.ntiles, ts.tile_start.data_ptr())
        assert (a.max_nnz, a.ell_width, a.ell_tiles) == (ts.max_nnzT, ts.ellT, ts.ellT_tiles.data_ptr())
    assert (a.nrb, a.ntiles, a.max_nnz, a.ell_width) == (1, 4, 160, 5)      # the alternate's, none of them the primary's
    assert a.tile_start != primary.tile_start.data_ptr() and a.ell_tiles != primary.ellT_tiles.data_ptr()


class _Recorder:
    """Stands in for the library: every entry point answers 0 and keeps its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


def test_only_the_chain_sets_max_tile_rows(monkeypatch):
    pkg = load_pkg()
    ts = _tiling(pkg, 2, 3, 4, 192, 256, 60)
    topo = _topo(ts)
    rec = _Recorder()
    monkeypatch.setattr(pkg._lib, "lib", lambda: rec)
    monkeypatch.setattr(pkg._lib, "stream_ptr", lambda dev: 0)
    H = 32
    X, Y, Bp = torch.zeros(N, H), torch.zeros(N, H), torch.zeros(8)
    pkg.ops.gemm_prop(topo, X, H, H, Bp, 3, H, Y, transposed=True)
    pkg.ops.gemm_prop_chain(topo, X, H, 3, [dict(Bp=Bp, Y=Y, relu=True), dict(Bp=Bp, Y=torch.zeros(N, H))])
    (n1, a1), (n2, a2) = rec.calls
    single, chain = a1[0]._obj, a2[0]._obj
    assert (n1, n2) == ("dss2_gemm_prop", "dss2_gemm_prop_chain")
    assert single.max_tile_rows == 0 and chain.max_tile_rows == 60
    assert (single.rowptr, single.max_nnz, single.ell_width, single.ell_tiles) == (topo.rowptrT.data_ptr(), 256, 4, ts.ellT_tiles.data_ptr())
    assert (chain.rowptr, chain.max_nnz, chain.ell_width, chain.ell_tiles) == (topo.rowptr.data_ptr(), 192, 3, ts.ell_tiles.data_ptr())
    assert (single.nrb, single.ntiles, chain.nrb, chain.ntiles) == (2, 2, 2, 2)


def test_stack_fill_common_reads_the_tiling_it_is_given(monkeypatch):
    pkg = load_pkg()
    primary, alt = _tiling(pkg, 2, 3, 4, 192, 256, 60), _tiling(pkg, 1, 3, 5, 96, 160, 30)
    topo = _topo(primary, (alt,))
    st = importlib.import_module(pkg.__name__ + ".stack")
    monkeypatch.setattr(st, "STACK_NRB", "auto")
    monkeypatch.setattr(st, "_cu_count", lambda dev: 1)        # more 64-row tiles than CUs: the primary tiling itself
    assert st.tiles_of(topo) is primary
    monkeypatch.setattr(st, "_cu_count", lambda dev: 256)      # CUs left idle: the 32-row alternate
    assert st.tiles_of(topo) is alt
    plan = types.SimpleNamespace(dims=pkg._lib.StackDims(), wpack=torch.zeros(4, dtype=torch.int32))
    x, ea, acts, eacache = torch.zeros(N, 8), torch.zeros(N, 6), torch.zeros(N, 32), torch.zeros(4)
    for ts in (primary, alt):
        a = pkg._lib.StackArgs()
        st._fill_common(a, plan, topo, ts, x, 8, ea, 6, acts, None, None, 0.0, eacache)
        assert (a.tile_start, a.ntiles, a.tm) == (ts.tile_start.data_ptr(), ts.ntiles, 32 * ts.nrb)
        assert (a.ell_w, a.ell_e, a.ell_width) == (ts.ell_tiles.data_ptr(), ts.ell_ent_tiles.data_ptr(), ts.ell)
        assert (a.ellT_w, a.ellT_e, a.ellT_width) == (ts.ellT_tiles.data_ptr(), ts.ellT_ent_tiles.data_ptr(), ts.ellT)
        assert (a.deg_pows, a.n_nodes, a.xs, a.drop_state) == (topo.deg_pows.data_ptr(), N, None, None)
