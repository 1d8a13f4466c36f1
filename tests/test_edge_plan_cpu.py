"""The edge MLP's one selection function (dss2_edge_plan, csrc/dss2_edge.hip) on the host: the record of its three passes for the
benchmark's shapes, the environment switches -- each changing the shapes it governs and no other --, the exact pairing of forward and
backward, and the host's one predicate for "tile kernels or CSR kernels".  No GPU needed: the library answers from the arguments and
the environment alone."""
import json
import os
import subprocess
import sys
import types

import torch

from conftest import load_pkg
from test_route_cpu import BATCHES, _topo

NONE, CSR, VALU, HALF, MFMA, BF16X6 = range(6)
FIELDS = ("family", "nrb", "parts", "block", "wg_per_tile", "lds_bytes")
EMPTY = (NONE, 0, 0, 0, 0, 0)
ON_CSR = (CSR, 0, 1, 256, 0, 0)


# The parent's launch formulas (dss2_edge_tile_fwd_paired / dss2_edge_tile_bwd and their launchers, before edge_select), in bytes, for a
# part of TM rows of a tile of XT rows at ELL width D:
#   staging (all tile kernels): the tile's x rows [XT][8], the slots' edge features [D][TM][8], their validity words [D][TM]
#   bf16x6 forward: + the x_i planes [3][TM][16 B] + every slot's planes [D][6][TM][16 B]
#   bf16x6 backward: + the x_i planes + ONE slot's planes [6][TM][16 B] + the transposed images 3 x 24 columns of 2 TM + 16 bytes
def _stage(TM, D, XT):
    return (XT * 8 + D * TM * 8) * 4 + D * TM * 4


def _f16(TM, D, XT):
    return _stage(TM, D, XT) + 3 * TM * 16 + D * 6 * TM * 16


def _b16(TM, D, XT):
    return _stage(TM, D, XT) + 3 * TM * 16 + 6 * TM * 16 + 3 * 24 * (2 * TM + 16)


def _m32(TM, D, waves, bwd):      # fp32 MFMA form: + one slot's operand rows [TM][36]; backward: + a dZ tile [TM][32] per wave
    return _stage(TM, D, TM) + TM * 36 * 4 + (waves * TM * 32 * 4 if bwd else 0)


# (nrb, ELL width by target, by source, hid, with_u) -> (forward, backward by target, backward by source): what the parent launched.
# Matrix pipe: a wave per 32 hidden units; forward one workgroup per tile (two with parts); the backward passes min(n_slabs, ntiles)
# persistent workgroups (0).  With U the by-source pass runs the VALU tile kernel (256 threads), and above 64 rows all three do.
GEOMETRY = {
    # cigre14, 64-row tiles
    (2, 3, 3, 128, 0): ((BF16X6, 2, 1, 256, 1, _f16(64, 3, 64)), (BF16X6, 2, 1, 256, 0, _b16(64, 3, 64)), EMPTY),
    (2, 3, 3, 128, 1): ((BF16X6, 2, 1, 256, 1, _f16(64, 3, 64)), (BF16X6, 2, 1, 256, 0, _b16(64, 3, 64)), (VALU, 2, 1, 256, 0, _stage(64, 3, 64))),
    (2, 3, 3, 256, 0): ((BF16X6, 2, 1, 512, 1, _f16(64, 3, 64)), (BF16X6, 2, 1, 512, 0, _b16(64, 3, 64)), EMPTY),
    (2, 4, 4, 256, 0): ((BF16X6, 2, 1, 512, 1, _f16(64, 4, 64)), (BF16X6, 2, 1, 512, 0, _b16(64, 4, 64)), EMPTY),      # (the mixed shard)
    # ober_sub, 96-row tiles: with U neither matrix-pipe backward is built, so the pair runs the VALU tile kernels
    (3, 3, 3, 128, 0): ((BF16X6, 3, 1, 256, 1, _f16(96, 3, 96)), (BF16X6, 3, 1, 256, 0, _b16(96, 3, 96)), EMPTY),
    (3, 3, 3, 128, 1): ((VALU, 3, 1, 256, 1, _stage(96, 3, 96)), (VALU, 3, 1, 256, 0, _stage(96, 3, 96)), (VALU, 3, 1, 256, 0, _stage(96, 3, 96))),
    (3, 3, 3, 32, 0): ((BF16X6, 3, 1, 64, 1, _f16(96, 3, 96)), (BF16X6, 3, 1, 64, 0, _b16(96, 3, 96)), EMPTY),
    (3, 3, 3, 32, 1): ((HALF, 3, 1, 256, 1, _stage(96, 3, 96)), (HALF, 3, 1, 256, 0, _stage(96, 3, 96)), (HALF, 3, 1, 256, 0, _stage(96, 3, 96))),
    # 128-row tiles (forced): two parts of 64 rows
    (4, 3, 3, 128, 0): ((BF16X6, 2, 2, 256, 2, _f16(64, 3, 128)), (BF16X6, 2, 2, 256, 0, _b16(64, 3, 128)), EMPTY),
    (4, 3, 3, 128, 1): ((VALU, 4, 1, 256, 1, _stage(128, 3, 128)), (VALU, 4, 1, 256, 0, _stage(128, 3, 128)), (VALU, 4, 1, 256, 0, _stage(128, 3, 128))),
    # ober179, 192-row tiles: two parts of 96 rows
    (6, 3, 3, 128, 0): ((BF16X6, 3, 2, 256, 2, _f16(96, 3, 192)), (BF16X6, 3, 2, 256, 0, _b16(96, 3, 192)), EMPTY),
    (6, 3, 3, 32, 0): ((BF16X6, 3, 2, 64, 2, _f16(96, 3, 192)), (BF16X6, 3, 2, 64, 0, _b16(96, 3, 192)), EMPTY),
    (6, 3, 3, 32, 1): ((HALF, 6, 1, 256, 1, _stage(192, 3, 192)), (HALF, 6, 1, 256, 0, _stage(192, 3, 192)), (HALF, 6, 1, 256, 0, _stage(192, 3, 192))),
    # a tiling without entry tables (a hub beyond the ELL width): the row-per-wave kernels on the CSR
    (2, 0, 0, 128, 0): (ON_CSR, ON_CSR, EMPTY),
    (2, 0, 0, 128, 1): (ON_CSR, ON_CSR, ON_CSR),
    # ... and a table on one side only, as the library sees it (the host sends such a tiling to the CSR on both sides, below)
    (2, 1, 0, 64, 1): ((BF16X6, 2, 1, 128, 1, _f16(64, 1, 64)), (BF16X6, 2, 1, 128, 0, _b16(64, 1, 64)), ON_CSR),
}


def _plan(pkg, nrb, ell, ellT, hid, with_u):
    p = pkg._lib.EdgePlan()
    assert pkg._lib.lib().dss2_edge_plan(hid, nrb, ell, ellT, with_u, p) == 0
    return p


def _row(k):
    return tuple(getattr(k, f) for f in FIELDS)


def _rows(pkg):
    """{'nrb/ell/ellT/hid/with_u': [forward, backward, by source, pair_exact]}"""
    out = {}
    for key in GEOMETRY:
        p = _plan(pkg, *key)
        out["/".join(map(str, key))] = [list(_row(p.fwd)), list(_row(p.bwd)), list(_row(p.bwd_src)), p.pair_exact]
    return out


def test_the_benchmarks_shapes_are_pinned():
    pkg = load_pkg()
    names = ("NONE", "CSR", "VALU", "VALU_HALF", "FP32_MFMA", "BF16X6")
    assert [getattr(pkg._lib, "EDGE_" + k) for k in names] == [NONE, CSR, VALU, HALF, MFMA, BF16X6]
    assert {(b[0], b[3], b[4]) for b in BATCHES.values()} <= {k[:3] for k in GEOMETRY}      # every batch the route tests know
    for key, want in GEOMETRY.items():
        p = _plan(pkg, *key)
        assert (_row(p.fwd), _row(p.bwd), _row(p.bwd_src)) == want, key
        assert max(k.lds_bytes for k in (p.fwd, p.bwd, p.bwd_src)) <= 160 * 1024, key
    # ops.edge_plan is that record
    p = pkg.ops.edge_plan(128, 2, 3, 3, False)
    assert (_row(p.fwd), _row(p.bwd), _row(p.bwd_src)) == GEOMETRY[(2, 3, 3, 128, 0)]


def test_the_pair_recomputes_exactly_on_every_pinned_shape():
    """Up to the ELL width the host ever sends (8), forward and backward by target run one family under the default switches."""
    pkg = load_pkg()
    for (nrb, ell, ellT, hid, with_u) in GEOMETRY:
        for w in range(0 if ell == 0 else 1, 1 if ell == 0 else 9):
            p = _plan(pkg, nrb, w, w, hid, with_u)
            assert p.pair_exact == 1 and p.fwd.family == p.bwd.family != NONE, (nrb, w, hid, with_u)
    # refused shapes have no pair
    assert _plan(pkg, 2, 3, 3, 288, 0).pair_exact == 0 and _row(_plan(pkg, 2, 33, 3, 128, 1).fwd) == EMPTY


def _matrix(row):
    return row[0] in (MFMA, BF16X6)


# switch setting -> (which pinned shapes it governs, from their default rows; what each pass becomes there, from its default row)
def _valu(r, hid, D):
    nrb = r[1] * r[2]      # (parts: the whole tile is staged)
    return [HALF if hid <= 32 else VALU, nrb, 1, 256, min(r[4], 1), _stage(32 * nrb, D, 32 * nrb)]


SWITCHES = {
    "DSS2_EDGE_MFMA=0": lambda rows: any(_matrix(r) for r in rows[:2]),
    "DSS2_EDGE_MFMA_FWD=0": lambda rows: _matrix(rows[0]),
    "DSS2_EDGE_MFMA_BWD=0": lambda rows: _matrix(rows[1]),
    "DSS2_EDGE_BF16=0": lambda rows: any(r[0] == BF16X6 for r in rows[:2]),
    "DSS2_EDGE_TILE_HALF=0": lambda rows: any(r[0] == HALF for r in rows[:3]),
}


def test_each_switch_governs_its_own_shapes():
    pkg = load_pkg()
    base = _rows(pkg)
    code = ("import json, sys; sys.path.insert(0, %r); import test_edge_plan_cpu as t; "
            "print('ROWS' + json.dumps(t._rows(t.load_pkg())))" % os.path.dirname(os.path.abspath(__file__)))
    procs = {sw: subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **dict([sw.split("=")])), stdout=subprocess.PIPE, text=True)
             for sw in SWITCHES}
    for sw, pr in procs.items():
        out = pr.communicate()[0]
        assert pr.returncode == 0, sw
        rows = json.loads([ln for ln in out.splitlines() if ln.startswith("ROWS")][0][4:])
        changed = {k for k in base if rows[k] != base[k]}
        governed = {k for k in base if SWITCHES[sw](base[k])}
        assert changed == governed and governed, sw
        for k in changed:
            nrb, ell, ellT, hid, with_u = map(int, k.split("/"))
            f0, b0, s0, _ = base[k]
            f1, b1, s1, exact = rows[k]
            assert s1 == s0 or (sw == "DSS2_EDGE_TILE_HALF=0" and s1 == [VALU] + s0[1:]), (sw, k)      # by source: the VALU tile kernel always
            if sw == "DSS2_EDGE_TILE_HALF=0":
                assert [f1, b1] == [[VALU] + f0[1:], [VALU] + b0[1:]] and exact == 1, (sw, k)
            elif sw == "DSS2_EDGE_BF16=0":      # whole tiles: the fp32 MFMA form of the same geometry (its own LDS); parts have none
                for r0, r1, bwd in ((f0, f1, False), (b0, b1, True)):
                    if r0[2] == 2:
                        assert r1 == _valu(r0, hid, ell), (sw, k)
                    else:
                        assert r1 == [MFMA] + r0[1:5] + [_m32(32 * nrb, ell, hid // 32, bwd)], (sw, k)
                assert exact == 1, (sw, k)
            else:
                off_f, off_b = sw != "DSS2_EDGE_MFMA_BWD=0", sw != "DSS2_EDGE_MFMA_FWD=0" or f0[2] == 2      # (parts: no backward without the forward)
                assert f1 == (_valu(f0, hid, ell) if off_f else f0) and b1 == (_valu(b0, hid, ell) if off_b else b0), (sw, k)
                assert exact == int(off_f and off_b), (sw, k)      # one pass alone off the matrix pipe: the pair is no longer exact


class _Spy:
    """Stands in for the loaded library: records the edge launches' argument structs instead of launching."""
    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("dss2_edge_fwd", "dss2_edge_bwd"):
            def record(a, stream):
                self.calls.append((name, {f: getattr(a._obj, f) for f, _ in type(a._obj)._fields_}))
                return 0
            return record
        return getattr(self.lib, name)


def test_one_predicate_sends_both_passes_to_the_same_kernels(monkeypatch):
    """A tiling with the entry table by target but none by source (in-degree <= 8 < out-degree) runs the CSR kernels in BOTH passes;
    with both tables both passes take the tiles; flags.EDGE_TILE_KERNELS = False: the CSR again."""
    pkg = load_pkg()
    nw, ops = pkg.networks, pkg.ops
    spy = _Spy(pkg._lib.lib())
    monkeypatch.setattr(pkg._lib, "lib", lambda: spy)
    monkeypatch.setattr(ops, "_stream", lambda t: 0)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    N, hid = 960, 64
    x, ea, W1, b1, dS = torch.zeros(N, 8), torch.zeros(4, 6), torch.zeros(hid, 22), torch.zeros(hid), torch.zeros(N, hid)
    slab, U = torch.zeros(16 * (hid * 23)), torch.zeros(2, N, hid)

    def run(ts):
        ts.tile_start = i32(ts.ntiles + 1)
        topo = types.SimpleNamespace(N=N, tiling=ts, rowptr=i32(N + 1), col=i32(4), ent=i32(4), rowptrT=i32(N + 1), colT=i32(4), entT=i32(4))
        del spy.calls[:]
        tiled, n_slabs = nw._edge_tiled(ts, N)
        nw._edge_aggr_forward(topo, x, 8, ea, 6, W1, b1, None, None, hid, hid, 8, 6, second_linear=False, need_dx=True)
        ops.edge_bwd(topo, tiled, x, 8, ea, 6, W1, b1, dS, slab, n_slabs, U[0], hid, hid, 8, 6, False)
        ops.edge_bwd(topo, tiled, x, 8, ea, 6, W1, b1, dS, None, n_slabs, U[1], hid, hid, 8, 6, True)
        assert [c[0] for c in spy.calls] == ["dss2_edge_fwd", "dss2_edge_bwd", "dss2_edge_bwd"]
        return tiled, n_slabs, topo, [c[1] for c in spy.calls]

    both = _topo("cigre14_64")
    both.ell_ent_tiles, both.ellT_ent_tiles = torch.zeros(1), torch.zeros(1)
    tiled, n_slabs, topo, calls = run(both)
    assert tiled and n_slabs == both.ntiles
    assert [c["ell_ent"] for c in calls] == [both.ell_ent_tiles.data_ptr()] * 2 + [both.ellT_ent_tiles.data_ptr()]
    assert all(c["ell_width"] == 3 and c["nrb"] == 2 and c["ntiles"] == 16 and c["rowptr"] is None for c in calls)
    assert [c["bwd_with_u"] for c in calls] == [1, 0, 0] and [c["by_source"] for c in calls] == [0, 0, 1]

    one_sided = _topo("cigre14_64")
    one_sided.ell_ent_tiles, one_sided.ellT_ent_tiles, one_sided.ell, one_sided.ellT = torch.zeros(1), None, 1, 0
    tiled, n_slabs, topo, calls = run(one_sided)
    assert not tiled and n_slabs == (N + 15) // 16
    assert all(c["ell_ent"] is None and c["n_nodes"] == N for c in calls)      # NULL table: the library's CSR family
    assert [c["rowptr"] for c in calls] == [topo.rowptr.data_ptr()] * 2 + [topo.rowptrT.data_ptr()]
    p = ops.edge_plan(hid, one_sided.nrb, 0, 0, True)
    assert p.fwd.family == p.bwd.family == p.bwd_src.family == CSR and p.pair_exact == 1

    keep = pkg.flags.EDGE_TILE_KERNELS
    pkg.flags.EDGE_TILE_KERNELS = False
    try:
        assert nw._edge_tiled(both, N) == (False, (N + 15) // 16)
    finally:
        pkg.flags.EDGE_TILE_KERNELS = keep


def test_the_chains_edge_phases_follow_the_edge_plan():
    """dss2_gemm_prop_chain_edge_supported: bit 0 / bit 1 exactly where the edge kernels of 64-row tiles run bf16x6 forward / backward
    (by target, without U) and the images fit the chain's regions (4 x 16 KB at hid = 128)."""
    pkg = load_pkg()
    L = pkg._lib.lib()
    for w in range(0, 34):
        p = _plan(pkg, 2, w, w, 128, 0)
        want = (int(p.fwd.family == BF16X6 and p.fwd.lds_bytes <= 65536) | 2 * int(p.bwd.family == BF16X6 and p.bwd.lds_bytes <= 65536)) if 1 <= w <= 32 else 0
        assert L.dss2_gemm_prop_chain_edge_supported(2, 3, 128, 128, 3, w) == want, w
    assert L.dss2_gemm_prop_chain_edge_supported(2, 3, 128, 128, 3, 3) == 3
