"""The layer chain's one selection function (dss2_gemm_prop_chain_plan, csrc/dss2_gemm_chain.hip) on the host: the record for the
benchmark's shapes, the seven older shape queries as readers of it, the one-column-group tile count, the environment switches -- each
changing the shapes it governs and no other -- and how often a block's route asks the library.  No GPU needed: the library answers from
the arguments alone."""
import itertools
import json
import os
import subprocess
import sys
import types

from conftest import load_pkg
from test_route_cpu import BATCHES, _topo

HIDS = (32, 64, 96, 128, 256)
NONE, FP32, BF16X6, SP, SP6 = range(5)
FIELDS = ("family", "row_split", "waves", "block", "lds_bytes", "gate_words", "head_modes", "head_wgrad", "edge_modes")

# (nrb, ELL width, hid) -> per K = 1, 2, 3: the PARENT library's answers (the build before chain_select) to
# (_chain_supported, _chain16_supported, _chain_f16_supported, _chain_gate_words, _chain_head_supported and _chain_head_wgrad_supported at
#  nout = 2, _chain_edge_supported at the edge kernels' width = the ELL width, the head pair again at nout = 4), run on these shapes
QUERIES = {
    (2, 3, 32): ((1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0)),
    (2, 3, 64): ((1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0)),
    (2, 3, 96): ((1, 1, 1, 96, 3, 1, 0, 3, 0), (1, 1, 1, 96, 3, 1, 0, 3, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
    (2, 3, 128): ((1, 1, 1, 128, 3, 1, 0, 3, 0), (1, 1, 1, 128, 3, 1, 3, 3, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
    (2, 3, 256): ((1, 1, 1, 256, 3, 1, 0, 3, 0), (1, 1, 1, 256, 3, 1, 0, 3, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
    (3, 3, 32): ((1, 1, 1, 64, 2, 1, 0, 2, 0), (1, 1, 1, 64, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (3, 3, 64): ((1, 1, 1, 128, 2, 1, 0, 2, 0), (1, 1, 1, 128, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (3, 3, 96): ((1, 1, 1, 192, 2, 1, 0, 2, 0), (1, 1, 1, 192, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (3, 3, 128): ((1, 1, 1, 256, 2, 1, 0, 2, 0), (1, 1, 1, 256, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (3, 3, 256): ((0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (6, 3, 32): ((0, 1, 1, 96, 2, 1, 0, 2, 0), (0, 1, 1, 96, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (6, 3, 64): ((0, 1, 1, 192, 2, 1, 0, 2, 0), (0, 1, 1, 192, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (6, 3, 96): ((0, 1, 1, 288, 2, 1, 0, 2, 0), (0, 1, 1, 288, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (6, 3, 128): ((0, 1, 1, 384, 2, 1, 0, 2, 0), (0, 1, 1, 384, 2, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (6, 3, 256): ((0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0)),
    (2, 4, 32): ((1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0)),
    (2, 4, 64): ((1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0)),
    (2, 4, 96): ((1, 1, 1, 96, 3, 1, 0, 3, 0), (1, 1, 1, 96, 3, 1, 0, 3, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
    (2, 4, 128): ((1, 1, 1, 128, 3, 1, 0, 3, 0), (1, 1, 1, 128, 3, 1, 3, 3, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
    (2, 4, 256): ((1, 1, 1, 256, 3, 1, 0, 3, 0), (1, 1, 1, 256, 3, 1, 0, 3, 0), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
}

# What the parent's dispatch launched, from its launchers' formulas: (batch, hid, K, b_format) -> (family, row split, waves, block, LDS bytes).
# Split planes: column groups x region (64 rows 16 KB, 96 rows 18 KB, 192 rows 36 KB) + the ELL slice + 64; multi-wave: the fp32 X tile
# (rows x (kpad + 4)), the stage per column group ([32][rows + 4], or per matrix [rows][36] with two waves per group) and the ELL slice.
GEOMETRY = {
    ("cigre14_4096", 128, 2, 1): (SP, 1, 4, 256, 4 * 16384 + 64 * 3 * 8 + 64),
    ("cigre14_4096", 128, 2, 2): (SP, 1, 4, 256, 4 * 16384 + 64 * 3 * 8 + 64),
    ("cigre14_4096", 128, 2, 0): (FP32, 1, 4, 256, 64 * 132 * 4 + 4 * 32 * 68 * 4 + 64 * 3 * 8),
    ("mixed_4096", 256, 2, 2): (SP, 1, 8, 512, 8 * 16384 + 64 * 4 * 8 + 64),
    ("cigre14_64", 64, 2, 1): (BF16X6, 2, 4, 256, 64 * 68 * 4 + 2 * 3 * 64 * 36 * 4 + 64 * 3 * 8),
    ("cigre14_64", 64, 3, 1): (BF16X6, 2, 4, 256, 64 * 68 * 4 + 2 * 32 * 68 * 4 + 64 * 3 * 8),
    ("ober_sub_1024", 128, 2, 2): (SP6, 1, 4, 256, 4 * 18432 + 96 * 3 * 8 + 64),
    ("ober_sub_1024", 32, 2, 1): (SP6, 1, 1, 64, 18432 + 96 * 3 * 8 + 64),
    ("ober_sub_64", 32, 2, 1): (BF16X6, 3, 12, 192, 96 * 36 * 4 + 32 * 100 * 4 + 96 * 3 * 8),
    ("ober_sub_64", 32, 2, 2): (NONE, 0, 0, 0, 0),
    ("ober179_1024", 128, 2, 1): (SP6, 1, 4, 256, 4 * 36864 + 192 * 3 * 8 + 64),
    ("ober179_1024", 128, 2, 0): (NONE, 0, 0, 0, 0),
}


def _plan(pkg, nrb, nmat, hid, ell, ntiles=0, nout=0, edge=0):
    p = pkg._lib.ChainPlan()
    assert pkg._lib.lib().dss2_gemm_prop_chain_plan(nrb, nmat, hid, ell, ntiles, nout, edge, p) == 0
    return p


def _row(k):
    return tuple(getattr(k, f) for f in FIELDS)


def _readers(p2, p4=None):
    """The seven queries' answers as read from the record (p2: asked with nout = 2 and the edge width; p4: nout = 4)."""
    r = (int(p2.fmt[0].family != 0), int(p2.fmt[1].family != 0), int(p2.fmt[2].gate_words > 0), p2.fmt[1].gate_words,
         p2.fmt[1].head_modes, p2.fmt[1].head_wgrad, p2.fmt[2].edge_modes)
    return r if p4 is None else r + (p4.fmt[1].head_modes, p4.fmt[1].head_wgrad)


def test_the_benchmarks_shapes_are_pinned():
    pkg = load_pkg()
    assert [getattr(pkg._lib, "CHAIN_" + k) for k in ("NONE", "FP32", "BF16X6", "SP", "SP6")] == [NONE, FP32, BF16X6, SP, SP6]
    assert {(b[0], b[3]) for b in BATCHES.values()} == {k[:2] for k in QUERIES} and all(b[3] == b[4] for b in BATCHES.values())
    for name, (nrb, ntiles, _, ell, *_rest) in BATCHES.items():
        for hid, K in itertools.product(HIDS, (1, 2, 3)):
            want = QUERIES[(nrb, ell, hid)][K - 1]
            cap = _readers(_plan(pkg, nrb, K + 1, hid, ell, 0, 2, ell), _plan(pkg, nrb, K + 1, hid, ell, 0, 4, ell))
            assert cap == want, (name, hid, K)
            # at the batch's own tile count: the same, except one column group on tall tiles below the policy count (768 tiles) -- there
            # the parent's host declined every split-plane capability (ops._single_group_tall_veto) and kept the multi-wave bf16x6 chain,
            # which 96-row tiles have and 192-row tiles do not
            real = _readers(_plan(pkg, nrb, K + 1, hid, ell, ntiles, 2, ell), _plan(pkg, nrb, K + 1, hid, ell, ntiles, 4, ell))
            if hid <= 32 and nrb in (3, 6) and ntiles < 768:
                want = (want[0], int(nrb == 3 and want[1])) + (0,) * 7
            assert real == want, (name, hid, K, ntiles)
    for (name, hid, K, f), want in GEOMETRY.items():
        nrb, ntiles, _, ell, *_rest = BATCHES[name]
        assert _row(_plan(pkg, nrb, K + 1, hid, ell, ntiles).fmt[f])[:5] == want, (name, hid, K, f)


def test_the_older_queries_read_the_plan():
    pkg = load_pkg()
    L = pkg._lib.lib()
    for nrb, nmat, hid, ell in itertools.product((1, 2, 3, 4, 5, 6), (1, 2, 3, 4, 5), (4, 30, 32, 64, 100, 128, 256, 260), (0, 3, 8, 33)):
        a = (nrb, nmat, hid, hid, ell)
        for nout, ew in ((0, 0), (1, 3), (2, 9), (4, 3), (5, 33)):
            p = _plan(pkg, nrb, nmat, hid, ell, 0, nout, ew)
            got = (L.dss2_gemm_prop_chain_supported(*a), L.dss2_gemm_prop_chain16_supported(*a), L.dss2_gemm_prop_chain_f16_supported(*a),
                   L.dss2_gemm_prop_chain_gate_words(*a), L.dss2_gemm_prop_chain_head_supported(*a, nout),
                   L.dss2_gemm_prop_chain_head_wgrad_supported(*a, nout), L.dss2_gemm_prop_chain_edge_supported(*a, ew))
            assert got == _readers(p), (a, nout, ew)
            for k in p.fmt:      # a family comes with a geometry, a head or an edge phase with a split-plane family
                assert (k.family != NONE) == (k.block > 0 and k.lds_bytes > 0 and k.waves > 0 and k.row_split > 0)
                assert k.lds_bytes <= 160 * 1024 and k.block == 64 * ((hid + 31) // 32) * k.row_split
                assert not (k.head_modes or k.head_wgrad or k.edge_modes) or k.family in (SP, SP6)
                assert not k.head_wgrad or k.head_modes & 2
            assert L.dss2_gemm_prop_chain_supported(nrb, nmat, hid + 4, hid, ell) == 0      # (a chain's layers are square)


def test_one_column_group_on_tall_tiles_follows_the_tile_count():
    pkg = load_pkg()
    m = pkg._lib.lib().dss2_chain_sp6_single_group_min_tiles()
    assert m == 768
    for nrb, f in itertools.product((3, 6), (1, 2)):
        at, below, cap = (_plan(pkg, nrb, 3, 32, 3, n, 2).fmt[f] for n in (m, m - 1, 0))
        assert _row(at) == _row(cap) and at.family == SP6 and (at.waves, at.block) == (1, 64) and at.gate_words > 0 and at.head_modes == 2
        assert (below.gate_words, below.head_modes, below.head_wgrad) == (0, 0, 0)
        # below the count: the multi-wave bf16x6 chain where the tile height has one (96 rows, bf16x3 weights), else no chain at all
        assert _row(below)[:4] == ((BF16X6, 3, 12, 192) if (nrb, f) == (3, 1) else (NONE, 0, 0, 0))
    assert all(k.family == NONE for k in _plan(pkg, 6, 3, 32, 3, m - 1).fmt)
    # two column groups: no tile count in it
    assert _row(_plan(pkg, 6, 3, 64, 3, 1).fmt[1]) == _row(_plan(pkg, 6, 3, 64, 3, 0).fmt[1]) != (0,) * 9


def _rows(pkg):
    """{'batch/hid/K': the three formats' rows at the batch's tile count, head nout = 2, the batch's edge width}"""
    return {"%s/%d/%d" % (name, hid, K): [list(_row(k)) for k in _plan(pkg, b[0], K + 1, hid, b[3], b[1], 2, b[3]).fmt]
            for (name, b), hid, K in itertools.product(BATCHES.items(), HIDS, (1, 2, 3))}


def _split_plane(rows, fmts=(1, 2)):
    return any(rows[f][0] in (SP, SP6) or rows[f][5] for f in fmts)


# switch setting -> which pinned shapes it governs, from the shape (nrb, ntiles, hid, K) and the default rows
SWITCHES = {
    "DSS2_CHAIN_SP=0": lambda nrb, ntiles, hid, K, rows: _split_plane(rows),
    "DSS2_CHAIN_SP_F16=0": lambda nrb, ntiles, hid, K, rows: _split_plane(rows, (2,)),
    "DSS2_CHAIN_SP6_NCG1=0": lambda nrb, ntiles, hid, K, rows: nrb in (3, 6) and hid <= 32 and _split_plane(rows),
    "DSS2_CHAIN_RS=1": lambda nrb, ntiles, hid, K, rows: nrb == 2 and hid <= 64,      # (default: two waves per column group)
    "DSS2_CHAIN_RS=2": lambda nrb, ntiles, hid, K, rows: nrb == 2 and 64 < hid <= 128,     # (default: one; above 128 there is no room for two)
    "DSS2_CHAIN_RS3=0": lambda nrb, ntiles, hid, K, rows: rows[1][:2] == [BF16X6, 3],
}


def test_each_switch_governs_its_own_shapes():
    pkg = load_pkg()
    base = _rows(pkg)
    code = ("import json, sys; sys.path.insert(0, %r); import test_chain_plan_cpu as t; "
            "print('ROWS' + json.dumps(t._rows(t.load_pkg())))" % os.path.dirname(os.path.abspath(__file__)))
    procs = {sw: subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **dict([sw.split("=")])), stdout=subprocess.PIPE, text=True)
             for sw in SWITCHES}
    for sw, pr in procs.items():
        out = pr.communicate()[0]
        assert pr.returncode == 0, sw
        rows = json.loads([ln for ln in out.splitlines() if ln.startswith("ROWS")][0][4:])
        changed = {k for k in base if rows[k] != base[k]}
        governed = set()
        for k in base:
            name, hid, K = k.split("/")
            if SWITCHES[sw](BATCHES[name][0], BATCHES[name][1], int(hid), int(K), base[k]):
                governed.add(k)
        assert changed == governed and governed, sw
        for k in changed:
            for f in range(3):
                if sw in ("DSS2_CHAIN_SP=0", "DSS2_CHAIN_SP6_NCG1=0") or (sw == "DSS2_CHAIN_SP_F16=0" and f == 2):
                    assert rows[k][f][0] not in (SP, SP6) and rows[k][f][5:] == [0, 0, 0, 0], (sw, k, f)
                elif sw == "DSS2_CHAIN_SP_F16=0":
                    assert rows[k][f] == base[k][f], (sw, k, f)
                elif sw.startswith("DSS2_CHAIN_RS="):
                    assert rows[k][f][0] not in (SP, SP6) and rows[k][f][1] in (0, int(sw[-1])), (sw, k, f)
                else:
                    assert rows[k][f] == base[k][f] or rows[k][f][:4] == [BF16X6, 1, 4, 64], (sw, k, f)


class _Spy:
    def __init__(self, lib):
        self.lib, self.asked = lib, []

    def __getattr__(self, name):
        self.asked.append(name)
        return getattr(self.lib, name)


def test_a_block_route_asks_about_the_chain_once_per_direction(monkeypatch):
    pkg = load_pkg()
    spy = _Spy(pkg._lib.lib())
    monkeypatch.setattr(pkg._lib, "lib", lambda: spy)
    mod = types.SimpleNamespace(dim_hid=128, n_gnn_layers=4, K=2, dim_out=2, dim_featn=8, dim_feate=6)
    r = pkg.route.block_route(mod, _topo("cigre14_4096"), False, False)
    assert r.n_chain == 3 and r.f16 and r.head and r.edge and r.bwd_head_wgrad and r.bwd_edge      # the C2 route, every fused form on
    chain = [n for n in spy.asked if "chain" in n]
    assert chain == ["dss2_gemm_prop_chain_plan"] * 2 and len(spy.asked) <= 3, spy.asked
