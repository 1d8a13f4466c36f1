"""The single-layer tile GEMM + propagation launch's one selection function (dss2_gemm_prop_plan, csrc/dss2_gemm_prop.hip) on the host:
the record for the benchmark's shapes, the two older shape queries as readers of it, what the operands change, the environment
switches -- each changing the shapes it governs and no other -- and how often the host asks the library.  No GPU needed: the library
answers from the arguments alone."""
import itertools
import json
import os
import subprocess
import sys
import types

from conftest import load_pkg
from test_chain_plan_cpu import _Spy
from test_route_cpu import BATCHES, _topo

HIDS = (32, 64, 128, 256)
NONE, NARROW_STREAM, NARROW, FP32, FP32_KHALF, BF16X6_KHALF = range(6)
FIELDS = ("kernel", "row_split", "waves", "block", "lds_bytes")
REFUSED = (NONE, 0, 0, 0, 0)
LDS = 160 * 1024

# What the parent's dispatch launched, from its launchers' formulas: (tile rows, hid) -> for K = 1 and for K = 2, 3, fp32 weights:
# (kernel, waves, LDS bytes without the graph slice).  The X tile [rows][kpad + 4] and one stage [32][rows + 4] per wave; a wave per
# column group up to four, fewer where the stages do not fit beside the tile; 192-row tiles in matrix-sequential mode (rows / 32 * (K + 1)
# >= 16: K >= 2) then stage the tile in two K halves and keep every column group's wave.  The ELL slice, rows * width * 8, comes on top.
GENERAL = {
    (64, 32): ((FP32, 1, 64 * 36 * 4 + 1 * 32 * 68 * 4),) * 2,
    (64, 64): ((FP32, 2, 64 * 68 * 4 + 2 * 32 * 68 * 4),) * 2,
    (64, 128): ((FP32, 4, 64 * 132 * 4 + 4 * 32 * 68 * 4),) * 2,
    (64, 256): ((FP32, 4, 64 * 260 * 4 + 4 * 32 * 68 * 4),) * 2,      # (eight column groups: four waves take two each)
    (96, 32): ((FP32, 1, 96 * 36 * 4 + 1 * 32 * 100 * 4),) * 2,
    (96, 64): ((FP32, 2, 96 * 68 * 4 + 2 * 32 * 100 * 4),) * 2,
    (96, 128): ((FP32, 4, 96 * 132 * 4 + 4 * 32 * 100 * 4),) * 2,
    (96, 256): ((FP32, 4, 96 * 260 * 4 + 4 * 32 * 100 * 4),) * 2,
    (192, 32): ((FP32, 1, 192 * 36 * 4 + 1 * 32 * 196 * 4),) * 2,
    (192, 64): ((FP32, 2, 192 * 68 * 4 + 2 * 32 * 196 * 4),) * 2,
    (192, 128): ((FP32, 2, 192 * 132 * 4 + 2 * 32 * 196 * 4), (FP32_KHALF, 4, 192 * 68 * 4 + 4 * 32 * 196 * 4)),
    (192, 256): (None, None),      # the X tile alone is 192 * 260 * 4 B: refused with code 3
}
# bf16x3 weights: the K-halved tall-tile form only, two waves per column group; every other pinned shape is refused (code 2, or 3 as above)
BF16 = {(192, 128): (None, (BF16X6_KHALF, 2, 4, 512, 192 * 68 * 4 + 4 * 32 * 196 * 4))}
# narrow heads hid -> nout: (K + 1) * nout <= 8 streams X (weights [8][kpad], results [rows][8]); else the X tile and one [rows][32]
# stage.  Both 256 threads, and both refused where the TILE form does not fit (192 rows x 256: the parent tested that first).
def _narrow(rows, hid, K, nout, ell):
    tile = rows * (hid + 4) * 4 + rows * 32 * 4 + rows * ell * 8
    if tile > LDS:
        return REFUSED
    return (NARROW_STREAM, 1, 4, 256, 8 * hid * 4 + rows * 8 * 4 + rows * ell * 8) if (K + 1) * nout <= 8 else (NARROW, 1, 4, 256, tile)


def _row(p):
    return tuple(int(getattr(p, f)) for f in FIELDS)


def _plan(pkg, nrb, nmat, kreal, hout, nnz, ell, b_format=0, narrow_h=0, X=0, ldx=0, **more):
    """The record of a launch filled by hand (the benchmark's shapes go through ops.gemm_plan instead)."""
    a, p = pkg._lib.GemmPropArgs(), pkg._lib.GemmPlan()
    a.nrb, a.nmat, a.kreal, a.kpad = nrb, nmat, kreal, ((kreal + 15) // 16 * 16 if b_format == 1 else (kreal + 7) // 8 * 8)
    a.hout, a.ncg, a.max_nnz, a.ell_width, a.ell_tiles = hout, (1 if narrow_h else (hout + 31) // 32), nnz, ell, (1 if ell > 0 else None)
    a.b_format, a.narrow_h, a.X, a.ldx = b_format, narrow_h, X or None, ldx
    for k, v in more.items():
        setattr(a, k, v)
    assert pkg._lib.lib().dss2_gemm_prop_plan(a, p) == 0
    return p


def _rows(pkg):
    """{'batch/hid/K/what': the record's row} of every pinned shape: what = fp32 | bf16 | head2 | head8"""
    out = {}
    for name, hid, K in itertools.product(BATCHES, HIDS, (1, 2, 3)):
        ts = _topo(name)
        for what, kw in (("fp32", dict(hout=hid)), ("bf16", dict(hout=hid, b_format=1)), ("head2", dict(hout=2, narrow_h=2)), ("head8", dict(hout=8, narrow_h=8))):
            out["%s/%d/%d/%s" % (name, hid, K, what)] = list(_row(pkg.ops.gemm_plan(ts, K + 1, hid, **kw)))
    return out


def test_the_benchmarks_shapes_are_pinned():
    pkg = load_pkg()
    L = pkg._lib
    assert [L.GEMM_NONE, L.GEMM_NARROW_STREAM, L.GEMM_NARROW, L.GEMM_FP32, L.GEMM_FP32_KHALF, L.GEMM_BF16X6_KHALF] == list(range(6))
    rows = _rows(pkg)
    for name, hid, K in itertools.product(BATCHES, HIDS, (1, 2, 3)):
        nrb, _, _, ell, ellT, *_rest = BATCHES[name]
        R, key = 32 * nrb, "%s/%d/%d/" % (name, hid, K)
        g = GENERAL[(R, hid)][K > 1]
        assert tuple(rows[key + "fp32"]) == (REFUSED if g is None else (g[0], 1, g[1], 64 * g[1], g[2] + R * ell * 8)), key
        b = BF16.get((R, hid), (None, None))[K > 1]
        assert tuple(rows[key + "bf16"]) == (REFUSED if b is None else b[:4] + (b[4] + R * ell * 8,)), key
        for nout in (2, 8):
            assert tuple(rows[key + "head%d" % nout]) == _narrow(R, hid, K, nout, ell), (key, nout)
        # the refusals' codes, and the by-source direction (the data gradient): the same record where the widths are the same
        ts = _topo(name)
        assert pkg.ops.gemm_plan(ts, K + 1, hid, hid).reason == (0 if g else 3)
        assert pkg.ops.gemm_plan(ts, K + 1, hid, hid, b_format=1).reason == (0 if b else 2 if g else 3)
        assert pkg.ops.gemm_plan(ts, K + 1, hid, 2, narrow_h=2).reason == (0 if _narrow(R, hid, K, 2, ell)[0] else 3)
        assert ell != ellT or _row(pkg.ops.gemm_plan(ts, K + 1, hid, hid, True)) == tuple(rows[key + "fp32"])


def test_the_older_queries_read_the_plan():
    pkg = load_pkg()
    L = pkg._lib.lib()
    V = (4, 30, 32, 64, 100, 128, 256, 260)
    for nrb, nmat, k, h, nnz, ell in itertools.product((1, 2, 3, 4, 5, 6), (1, 2, 3, 4, 5), V, V, (0, 500), (0, 3, 9, 32, 33)):
        p, p16 = _plan(pkg, nrb, nmat, k, h, nnz, ell), _plan(pkg, nrb, nmat, k, h, nnz, ell, 1)
        assert L.dss2_gemm_prop_lds_bytes(nrb, nmat, (k + 7) // 8 * 8, (h + 31) // 32, nnz, ell) == p.sizing_lds, (nrb, nmat, k, h, nnz, ell)
        assert L.dss2_gemm_prop16_supported(nrb, nmat, k, h, nnz, ell) == int(p16.kernel == BF16X6_KHALF), (nrb, nmat, k, h, nnz, ell)
        for q in (p, p16) + ((_plan(pkg, nrb, nmat, k, h, nnz, ell, narrow_h=h),) if nmat * h <= 32 else ()):
            assert (q.kernel != NONE) == (q.block > 0 and q.lds_bytes > 0) and (q.kernel != NONE) == (q.reason == 0) and q.reason in (0, 2, 3)
            assert q.lds_bytes <= LDS
            if q.kernel in (NARROW_STREAM, NARROW):
                assert (q.block, q.row_split) == (256, 1)
            else:
                assert q.block == 64 * q.waves * q.row_split and q.waves <= max(1, min(4, (h + 31) // 32))
                assert (q.kernel == BF16X6_KHALF) == (q is p16 and q.kernel != NONE) and q.row_split == (2 if q.kernel == BF16X6_KHALF else q.kernel != NONE)
                if q.kernel in (FP32_KHALF, BF16X6_KHALF):      # K-halving: where the full tile left a column group without its wave
                    assert q.waves == (h + 31) // 32 and q.lds_bytes != q.sizing_lds and nrb * nmat >= 16
                elif q.kernel == FP32:
                    assert q.lds_bytes == q.sizing_lds


def test_the_operands_can_take_a_launch_off_the_fast_kernel():
    pkg = load_pkg()
    head = dict(nrb=2, nmat=3, kreal=32, hout=2, nnz=192, ell=3, narrow_h=2)
    tall = dict(nrb=6, nmat=3, kreal=128, hout=128, nnz=576, ell=3)
    assert _plan(pkg, **head).kernel == NARROW_STREAM and _plan(pkg, **tall).kernel == FP32_KHALF
    for shape, slow in ((head, NARROW), (tall, FP32)):
        base = _row(_plan(pkg, **shape))
        assert _row(_plan(pkg, **shape, X=1 << 20, ldx=shape["kreal"])) == base      # (an aligned X and a leading dimension of whole float4s)
        for change in (dict(kreal=shape["kreal"] - 2), dict(X=(1 << 20) + 4), dict(ldx=shape["kreal"] + 2)):      # (kpad stays a multiple of 16)
            p = _plan(pkg, **dict(shape, **change))
            assert p.kernel == slow and p.reason == 0, change
        assert _plan(pkg, **dict(shape, ell=0)).kernel == slow and _plan(pkg, **shape, ell_tiles=None).kernel == (slow if shape is head else FP32_KHALF)
    # fp32: two waves beside the full tile; bf16x3 weights have no such form -- refused, as is a row-scaled bias or input-side propagation
    assert _row(_plan(pkg, **tall, X=4))[1:4] == (1, 2, 128)
    ok16 = _plan(pkg, **tall, b_format=1)
    assert _row(ok16)[:4] == (BF16X6_KHALF, 2, 4, 512) and ok16.lds_bytes == _plan(pkg, **tall).lds_bytes
    for change in (dict(X=4), dict(ldx=130), dict(rowscale=1 << 20), dict(kreal=126), dict(hout=126)):
        p = _plan(pkg, **dict(tall, **change), b_format=1)
        assert (p.kernel, p.reason) == (NONE, 2), change
    assert _plan(pkg, nrb=2, nmat=1, kreal=16, hout=32, nnz=192, ell=3, prop_in=1).sizing_lds == _plan(pkg, nrb=2, nmat=2, kreal=16, hout=32, nnz=192, ell=3).sizing_lds


# switch setting -> which pinned rows it governs, from the default row, and what becomes of one
SWITCHES = {
    "DSS2_NARROW_STREAM=0": (lambda row: row[0] == NARROW_STREAM, lambda row, new: new[:4] == [NARROW, 1, 4, 256]),
    "DSS2_GEMM_KHALF=0": (lambda row: row[0] in (FP32_KHALF, BF16X6_KHALF), lambda row, new: new[:4] == ([FP32, 1, 2, 128] if row[0] == FP32_KHALF else [NONE, 0, 0, 0])),
    "DSS2_GEMM_RS=1": (lambda row: row[0] == BF16X6_KHALF, lambda row, new: new == [BF16X6_KHALF, 1, 4, 256, row[4]]),
}


def test_each_switch_governs_its_own_shapes():
    pkg = load_pkg()
    base = _rows(pkg)
    code = ("import json, sys; sys.path.insert(0, %r); import test_gemm_plan_cpu as t; "
            "print('ROWS' + json.dumps(t._rows(t.load_pkg())))" % os.path.dirname(os.path.abspath(__file__)))
    procs = {sw: subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **dict([sw.split("=")])), stdout=subprocess.PIPE, text=True)
             for sw in SWITCHES}
    for sw, pr in procs.items():
        out = pr.communicate()[0]
        assert pr.returncode == 0, sw
        rows = json.loads([ln for ln in out.splitlines() if ln.startswith("ROWS")][0][4:])
        governs, becomes = SWITCHES[sw]
        changed, governed = {k for k in base if rows[k] != base[k]}, {k for k in base if governs(base[k])}
        assert changed == governed and governed, sw
        assert all(becomes(base[k], rows[k]) for k in changed), sw


def test_the_host_asks_once(monkeypatch):
    pkg = load_pkg()
    spy = _Spy(pkg._lib.lib())
    monkeypatch.setattr(pkg._lib, "lib", lambda: spy)
    mod = types.SimpleNamespace(dim_hid=128, n_gnn_layers=4, K=2, dim_out=2, dim_featn=8, dim_feate=6)
    assert pkg.route.block_route(mod, _topo("cigre14_4096"), False, False).n_chain == 3
    assert spy.asked == ["dss2_gemm_prop_chain_plan"] * 2      # (the parent's two: this shape's route asks nothing of the single-layer launch)
    del spy.asked[:]
    mod = types.SimpleNamespace(dim_hid=64, n_gnn_layers=3, K=3, dim_out=2, dim_featn=8, dim_feate=6)
    pkg.route.block_route(mod, _topo("ober_sub_64"), False, False)      # (unchained layers: the parent asked dss2_gemm_prop16_supported four times)
    assert spy.asked == ["dss2_gemm_prop_chain_plan"] * 2 + ["dss2_gemm_prop_plan"] * 4
    del spy.asked[:]
    assert pkg.ops.gemm16_supported(_topo("ober179_1024"), 3, 128, False) and pkg.ops.gemm16_supported(_topo("ober179_1024"), 3, 128, True)
    assert not pkg.ops.gemm16_supported(_topo("cigre14_4096"), 3, 128, False)
    assert spy.asked == ["dss2_gemm_prop_plan"] * 3
    del spy.asked[:]
    pkg.topology.Topology.lds_check(types.SimpleNamespace(tiling=_topo("ober179_1024")), 3, 128, 4)
    assert spy.asked == ["dss2_gemm_prop_plan"]
