"""GPU: the dataset kernels of csrc/dss2_dataset.hip on their own -- ``dss2_measure_nodes`` / ``dss2_measure_edges``,
``dss2_masked_zscore``, ``dss2_collate`` / ``dss2_collate_cursor`` / ``dss2_collate_ragged`` / ``dss2_collate_ragged_multi`` and
``dss2_accum_scalar`` driven through ctypes with hand-built tables, against the plain references of tests/dataset_kernel_cases.py, at
the shapes, masks, flags and values the models' data never produces; then the Python layer above them (dataset.py) at part counts
and edge-list forms the other tests do not reach.

Every operand sits in one device buffer with NaN in all gaps and every output in one buffer prefilled with a sentinel bit pattern,
guard bands in front and behind (gaps, guards and unwritten cells must keep it bit for bit).  Every launch runs twice from the same
inputs with equal bits.

What is compared, and how:
  measurement model   every row bit for bit with the oracle (float64 arithmetic rounded once; NaN in the same cells)
  collation           bit for bit with numpy indexing; every cell of a store holds its own flat index, so a misplaced chunk shows
  z-score, output     bit for bit (sign of zero included) with the oracle normalising by the KERNEL's statistics: given those, every
                      output is one chain of correctly rounded fp32 operations
  z-score, statistics against numpy float64:  |mean - mean64| <= 3 u |mean64|,  |std - std64| <= 8 u std64,  u = 2^-24.
      mean: the kernel's sum is exact to double; the bound allows one rounding of the sum, one of the quotient, one in reserve.
      std:  d = fl(v - mean32) carries the mean's error e_m <= u |mean| and its own rounding; fl(d d) one more: three roundings on
            each squared deviation, (3 u) on the variance, then the quotient and the root (u + u/2 after halving by the root): < 5 u;
            the mean's error enters the variance as e_m^2 / var <= (u |mean| / std)^2 = 1e4 u^2 at |mean| / std <= 100, far below
            one u (the first-order term sum(v - mean) e_m vanishes around the true mean); 8 u leaves three in reserve.
      Columns whose statistics the reference defines by nan_to_num (a NaN or an Inf entry) must equal the oracle's 0 / +-FLT_MAX;
      constant columns must give mean = the value and std = 0 exactly; a column of sub-normal values std = 0 (its fp32 squares
      underflow) and outputs of +-FLT_MAX.

Measured on the MI355X, worst |error| / bound over the random columns of a case (rows x ld, feature columns), mean then std:
    63x6 (6) 0.214 0.047     64x13 (8) 0.094 0.127    65x16 (16) 0.187 0.126    256x6 (6) 0.184 0.029    257x13 (8) 0.197 0.147
    65280x16 (16) 0.157 0.085    over all cases, the four beyond 65 280 rows included: 0.239 0.147
    data_from_tables at S = 3, n = 5, e = 4: x 0.209 0.118, edge_attr 0.087 0.066
  (the mean now carries one fp32 rounding, at most 1/3 of its bound.)
Everything else is exact: the measurement model, every collation, the normalised output, the constant columns, the cursor.

What these tests changed in csrc/dss2_dataset.hip, and the test that fails without each change:
  the mean (and the variance) is the double sum divided in double and rounded once -- test_masked_zscore_constant_columns
      (tests/test_dataset_kernel_cases_cpu.py shows on the CPU that fl(fl(n v) / n) != v for the value of every count that is no
      power of two, and that (float)(n v / n) = v);
  a NaN standard deviation keeps its NaN weight -- test_measurement_model[nonfinite] and [nonfinite_unmeasured];
  ld_out < ld, or in place with ld_out != ld, returns 2 before any launch -- test_masked_zscore_refusals_and_scratch;
  the cursor advances by (position + batch) mod length -- test_collate_cursor[len5_batch16_pos0-1] and [len5_batch16_pos3-1];
  mean and std go through the reference's nan_to_num (+-inf -> +-FLT_MAX, not only nan -> 0) and the squared deviations are
      multiplied by the mask as the reference writes them (inf * 0 = nan) -- the "inf" and "inf_dense" columns of test_masked_zscore.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import dataset_kernel_cases as dc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                  # sentinel words in front of and behind every output


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


class _Arena:
    """int32 images of host arrays (any dtype; bytes padded to whole words) laid end to end, each on a 16-byte boundary, the space
    between them holding ``fill``; ``device()`` uploads a fresh copy."""

    def __init__(self, fill):
        self.fill, self.parts, self.n = fill, [], 0

    def gap(self, n):
        self.parts.append(np.full(n, self.fill, np.int32))
        self.n += n

    def add(self, a):
        self.gap((-self.n) % 4)
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if b.size % 4:
            b = np.concatenate([b, np.full((-b.size) % 4, 0xFF, np.uint8)])
        off = self.n
        self.parts.append(b.view(np.int32))
        self.n += b.size // 4
        return off

    def out(self, words):
        """A sentinel block of ``words`` between two guard bands; its offset."""
        self.gap(GUARD)
        off = self.add(np.full(words, self.fill, np.int32))
        self.gap(GUARD)
        return off

    def host(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(4, np.int32)

    def device(self):
        t = torch.from_numpy(self.host()).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t


def _ptr(t, off):
    return t.data_ptr() + 4 * off


def _view(words, off, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize // 4
    return words[off:off + n].view(dtype).reshape(shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _last_error(pkg):
    return (pkg._lib.lib().dss2_last_error() or b"").decode()


def _st(pkg):
    return pkg._lib.stream_ptr(DEV)


def _only_written(got, outs, extents, what):
    """Every word outside the logical extents [(offset, words)] keeps the prefill."""
    expect = outs.host().copy()
    for off, n in extents:
        expect[off:off + n] = got[off:off + n]
    assert np.array_equal(got, expect), f"{what}: a gap, a guard band or an unwritten cell lost its sentinel"


# ------------------------------------------------------------------------------------------
# A. measurement model
# ------------------------------------------------------------------------------------------
def _measure_setup(c):
    nodes, zn = dc.node_tables(c)
    edges, ze = dc.edge_tables(c)
    ins, outs = _Arena(dc.NAN_BITS), _Arena(dc.SENTINEL)
    o = dict(nodes=ins.add(nodes), zn=ins.add(zn), edges=ins.add(edges), ze=ins.add(ze), mask=ins.add(c.mask_bytes()))
    ins.gap(GUARD)
    o["x"], o["ea"] = outs.out(c.rows * 11), outs.out(c.rows * 13)
    return ins, outs, o


def _measure_run(pkg, c, outs, o, din, rows=None, per=None, null=None):
    L, nz, dout = pkg._lib.lib(), dc.NOISES[c.noise], outs.device()
    rows = c.rows if rows is None else rows
    per = c.per if per is None else per
    p = {k: (None if k == null else _ptr(dout if k in ("x", "ea") else din, v)) for k, v in o.items()}
    rn = L.dss2_measure_nodes(p["nodes"], p["mask"], per, p["zn"], nz["v_noise"], nz["pm_noise"], nz["p_noise"], nz["zero_inj_coef"],
                              p["x"], rows, _st(pkg))
    err_n = _last_error(pkg)
    re = L.dss2_measure_edges(p["edges"], p["mask"], per, p["ze"], nz["p_noise"], p["ea"], rows, _st(pkg))
    err_e = _last_error(pkg)
    torch.cuda.synchronize()
    return rn, re, err_n, err_e, dout.cpu().numpy()


@pytest.mark.parametrize("c", dc.MEASURE_CASES, ids=lambda c: c.name)
def test_measurement_model(pkg, c):
    ins, outs, o = _measure_setup(c)
    din = ins.device()
    rn, re, en, ee, got = _measure_run(pkg, c, outs, o, din)
    assert rn == 0 and re == 0, (en, ee)
    assert np.array_equal(got, _measure_run(pkg, c, outs, o, din)[4]), "two launches from the same inputs differ in bits"
    x, ea = _view(got, o["x"], (c.rows, 11), np.float32), _view(got, o["ea"], (c.rows, 13), np.float32)
    wx, wea = dc.ref_nodes(c), dc.ref_edges(c)
    bad = np.flatnonzero(~((_bits(x) == _bits(wx)) | (np.isnan(x) & np.isnan(wx))).all(1))
    assert dc.same_bits_or_both_nan(x, wx), (c.name, f"node rows {bad[:6]} differ", x[bad[:2]], wx[bad[:2]])
    bad = np.flatnonzero(~((_bits(ea) == _bits(wea)) | (np.isnan(ea) & np.isnan(wea))).all(1))
    assert dc.same_bits_or_both_nan(ea, wea), (c.name, f"edge rows {bad[:6]} differ", ea[bad[:2]], wea[bad[:2]])
    _only_written(got, outs, [(o["x"], c.rows * 11), (o["ea"], c.rows * 13)], c.name)


def test_measurement_model_refusals(pkg):
    c = dc.MEASURE_CASES[2]
    ins, outs, o = _measure_setup(c)
    din = ins.device()
    for rows in (0, -1):
        rn, re, _, _, got = _measure_run(pkg, c, outs, o, din, rows=rows)
        assert rn == 0 and re == 0 and np.array_equal(got, outs.host()), "rows <= 0 returns 0 and writes nothing"
    for kw in (dict(per=0), dict(per=-1), dict(null="mask"), dict(null="nodes"), dict(null="zn"), dict(null="x"), dict(null="edges"),
               dict(null="ze"), dict(null="ea")):
        rn, re, en, ee, got = _measure_run(pkg, c, outs, o, din, **kw)
        nodes_hit = kw.get("null") in (None, "mask", "nodes", "zn", "x")
        edges_hit = kw.get("null") in (None, "mask", "edges", "ze", "ea")
        assert rn == (2 if nodes_hit else 0) and re == (2 if edges_hit else 0), kw
        assert (not nodes_hit or en.startswith("measure_nodes:")) and (not edges_hit or ee.startswith("measure_edges:")), (kw, en, ee)
        expect = outs.host().copy()
        if not nodes_hit:
            expect[o["x"]:o["x"] + c.rows * 11] = got[o["x"]:o["x"] + c.rows * 11]
        if not edges_hit:
            expect[o["ea"]:o["ea"] + c.rows * 13] = got[o["ea"]:o["ea"] + c.rows * 13]
        assert np.array_equal(got, expect), (kw, "a refused launch wrote")


# ------------------------------------------------------------------------------------------
# B. masked z-score
# ------------------------------------------------------------------------------------------
def _zs_run(pkg, t, num_feat, layout, ld_out=None, rows=None, null=None, ld=None):
    """One call on a fresh pair of arenas.  Returns (rc, outs, offsets, words read back)."""
    R, LD = t.shape
    ld_out = (LD + 3 if layout == "wider" else LD) if ld_out is None else ld_out
    ins, outs = _Arena(dc.NAN_BITS), _Arena(dc.SENTINEL)
    o = {}
    if layout == "in_place":
        outs.gap(GUARD)
        o["t"] = o["out"] = outs.add(t)
        outs.gap(GUARD)
    else:
        o["t"] = ins.add(t)
        o["out"] = outs.out(R * max(ld_out, 1))
    ins.gap(GUARD)
    o["mean"], o["std"] = outs.out(16), outs.out(16)
    din, dout = ins.device(), outs.device()
    L = pkg._lib.lib()
    scratch = torch.full((int(L.dss2_masked_zscore_scratch_doubles(R)),), float("nan"), dtype=torch.float64, device=DEV)
    p = dict(t=_ptr(dout if layout == "in_place" else din, o["t"]), out=_ptr(dout, o["out"]), mean=_ptr(dout, o["mean"]),
             std=_ptr(dout, o["std"]), scratch=scratch.data_ptr())
    if null:
        p[null] = None
    rc = L.dss2_masked_zscore(p["t"], R if rows is None else rows, LD if ld is None else ld, num_feat, p["out"], ld_out, p["mean"], p["std"],
                              p["scratch"], _st(pkg))
    torch.cuda.synchronize()
    return rc, outs, o, dout.cpu().numpy()


def _zs_results(t, num_feat, layout, outs, o, got, what):
    R, LD = t.shape
    ld_out = LD + 3 if layout == "wider" else LD
    out = _view(got, o["out"], (R, ld_out), np.float32)
    mean, std = _view(got, o["mean"], (num_feat,), np.float32).copy(), _view(got, o["std"], (num_feat,), np.float32).copy()
    rows = [(o["out"], R * LD)] if ld_out == LD else [(o["out"] + r * ld_out, LD) for r in range(R)]
    _only_written(got, outs, rows + [(o["mean"], num_feat), (o["std"], num_feat)], what)
    return np.ascontiguousarray(out[:, :LD]), mean, std


_ZS_WORST = {"mean": 0.0, "std": 0.0}


@pytest.mark.parametrize("c", dc.ZSCORE_CASES, ids=lambda c: c.name)
def test_masked_zscore(pkg, c):
    t = dc.zscore_table(c)
    rc, outs, o, got = _zs_run(pkg, t, c.num_feat, c.layout)
    assert rc == 0, _last_error(pkg)
    assert np.array_equal(got, _zs_run(pkg, t, c.num_feat, c.layout)[3]), "two launches from the same inputs differ in bits"
    out, mean, std = _zs_results(t, c.num_feat, c.layout, outs, o, got, c.name)
    assert np.array_equal(_bits(out[:, c.num_feat:]), _bits(t[:, c.num_feat:])), "a passthrough column is no bit copy"
    n, mean64, std64 = dc.stats64(t, c.num_feat)
    omean, ostd = dc.oracle_stats(t, c.num_feat)
    lines = []
    for j, kind in enumerate(c.kinds):
        if kind in dc.ZS_ORACLE_STATS:
            assert mean[j] == omean[j] and std[j] == ostd[j], (c.name, j, kind, mean[j], omean[j], std[j], ostd[j])
            continue
        em, bm = abs(float(mean[j]) - mean64[j]), dc.ZS_MEAN_BOUND * abs(mean64[j])
        lines.append(f"col {j} {kind}: n {n[j]} |mean err| {em:.3e} bound {bm:.3e}")
        assert em <= bm, (c.name, j, kind, mean[j], mean64[j])
        if kind == "subnormal" and c.rows > 1:
            assert std[j] == 0, (c.name, j, std[j])
            continue
        es, bs = abs(float(std[j]) - std64[j]), dc.ZS_STD_BOUND * std64[j]
        lines[-1] += f"  |std err| {es:.3e} bound {bs:.3e}"
        assert es <= bs, (c.name, j, kind, std[j], std64[j])
        if kind in dc.ZS_BOUNDED:
            _ZS_WORST["mean"] = max(_ZS_WORST["mean"], em / bm if bm else 0.0)
            _ZS_WORST["std"] = max(_ZS_WORST["std"], es / bs if bs else 0.0)
        if kind == "allzero":
            assert n[j] == 0 and mean[j] == 0 and std[j] == 0 and (out[:, j] == 0).all()
        if kind == "single":
            assert mean[j] == np.float32(-2.75) and std[j] == 0
    print(f"[masked_zscore {c.name}] " + "; ".join(lines))
    print(f"[masked_zscore] worst |error| / bound so far: mean {_ZS_WORST['mean']:.3f}  std {_ZS_WORST['std']:.3f}")
    want = dc.ref_normalised(t, c.num_feat, mean, std)
    bad = np.argwhere(_bits(out) != _bits(want))
    assert bad.size == 0, (c.name, f"{len(bad)} cells differ from the oracle run with the kernel's statistics, first {bad[:4].tolist()}",
                           [(out[r, k], want[r, k], t[r, k]) for r, k in bad[:4]])
    if "subnormal" in c.kinds and c.rows > 1:
        j = c.kinds.index("subnormal")
        assert (np.abs(out[:, j][t[:, j] != 0]) == np.float32(dc.FLT_MAX)).all()


@pytest.mark.parametrize("g", range(len(dc.CONST_GROUPS)))
@pytest.mark.parametrize("layout", ["in_place", "wider"])
def test_masked_zscore_constant_columns(pkg, g, layout):
    """A column of n equal values v: mean v, std 0, every z-score 0, for n = 1..33 and 960 (a mean rounded twice is one ulp off for
    these v, its "std" that ulp and the z-scores +-1)."""
    t, counts = dc.const_table(g), dc.CONST_GROUPS[g]
    nf = len(counts)
    rc, outs, o, got = _zs_run(pkg, t, nf, layout)
    assert rc == 0, _last_error(pkg)
    assert np.array_equal(got, _zs_run(pkg, t, nf, layout)[3]), "two launches from the same inputs differ in bits"
    out, mean, std = _zs_results(t, nf, layout, outs, o, got, f"constant group {g}")
    vals = np.array([dc.const_values()[n] for n in counts], np.float32)
    wrong = [(n, float(v), float(m)) for n, v, m in zip(counts, vals, mean) if m != v]
    assert not wrong, f"(count, value, mean): {wrong}"
    assert (std == 0).all(), [(n, float(s)) for n, s in zip(counts, std) if s != 0]
    assert (out[:, :nf] == 0).all() and np.array_equal(_bits(out), _bits(dc.ref_normalised(t, nf, mean, std)))


def test_masked_zscore_refusals_and_scratch(pkg):
    L = pkg._lib.lib()
    assert [L.dss2_masked_zscore_scratch_doubles(r) for r in (0, 1, 65_280, 65_281)] == [48, 48, 16 + 255 * 32, 16 + 256 * 32]
    t, nf = dc.zscore_table(dc.ZS_REFUSAL_CASE), dc.ZS_REFUSAL_NUM_FEAT          # 63 x 6, 4 feature columns: ld < 16
    R, LD = t.shape
    assert nf < LD < 16

    def untouched(layout, **kw):
        rc, outs, o, got = _zs_run(pkg, t, kw.pop("num_feat", nf), layout, **kw)
        assert np.array_equal(got, outs.host()), (kw, "a refused call wrote")
        return rc

    for rows in (0, -5):
        assert untouched("same_ld", rows=rows) == 0
    for bad_nf in (0, 17, -1):
        assert untouched("same_ld", num_feat=bad_nf) == 2 and _last_error(pkg).startswith("masked_zscore: num_feat")
    for bad_nf in (LD + 1, 16):      # within 1..16 and wider than a row: the kernels would read the next row's cells as features
        assert untouched("same_ld", num_feat=bad_nf) == 2 and _last_error(pkg).startswith("masked_zscore: num_feat") and f"ld {LD}" in _last_error(pkg)
        assert untouched("in_place", num_feat=bad_nf) == 2
    for null in ("t", "out", "mean", "std", "scratch"):
        assert untouched("same_ld", null=null) == 2 and _last_error(pkg).startswith("masked_zscore:")
    # finding 3: a shorter output row would run into the next one and past the end of out
    for ld_out in (LD - 1, nf, 1, 0):
        assert untouched("same_ld", ld_out=ld_out) == 2 and "ld_out" in _last_error(pkg), ld_out
    wide = np.ascontiguousarray(np.concatenate([t, t[:, :3]], axis=1))       # in place: the two strides must agree
    rc, outs, o, got = _zs_run(pkg, wide, nf, "in_place", ld=LD, ld_out=LD + 3)
    assert rc == 2 and "ld_out" in _last_error(pkg) and np.array_equal(got, outs.host())


# ------------------------------------------------------------------------------------------
# C. collation
# ------------------------------------------------------------------------------------------
_DT = {0: np.float32, 1: np.int64, 2: np.int32}


def _words(kind, cells):
    return cells * (2 if kind == 1 else 1)


def _collate_setup(layout, B, S=dc.COLLATE_S):
    """Stores in the input arena, destinations in the output arena: [(kind, shared, chunk, src array, src offset, dst offset, dst cells)]."""
    ins, outs, items = _Arena(dc.NAN_BITS), _Arena(dc.SENTINEL), []
    for i, (kind, shared, chunk) in enumerate(layout):
        src = dc.collate_source(kind, shared, chunk, S, base=3 * i)
        cells = B * chunk * (2 if kind == 1 else 1)
        items.append((kind, shared, chunk, src, ins.add(src), outs.out(_words(kind, cells)), cells))
    ins.gap(GUARD)
    return ins, outs, items


def _descs(pkg, items, din, dout, nps):
    descs = (pkg._lib.CollateDesc * max(len(items), 1))()
    for d, (kind, shared, chunk, _, so, do, _) in zip(descs, items):
        d.src, d.dst, d.chunk, d.kind, d.shared, d.nodes_per_sample = _ptr(din, so), _ptr(dout, do), chunk, kind, shared, nps
    return descs


def _collate_check(got, outs, items, ids, B, nps, what, extra=()):
    for kind, shared, chunk, src, _, do, cells in items:
        res = _view(got, do, (cells,), _DT[kind])
        want = dc.ref_collate(kind, shared, src, ids, B, nps).reshape(-1)
        bad = np.flatnonzero(_bits(res) != _bits(want))
        assert bad.size == 0, (what, f"kind {kind} shared {shared} chunk {chunk}: {bad.size} cells differ, first at {bad[:4]}",
                               res[bad[:4]], want[bad[:4]])
    _only_written(got, outs, [(do, _words(kind, cells)) for kind, _, _, _, _, do, cells in items] + list(extra), what)


@pytest.mark.parametrize("how", dc.COLLATE_IDS)
@pytest.mark.parametrize("B", dc.COLLATE_BATCHES)
@pytest.mark.parametrize("layout", sorted(dc.COLLATE_LAYOUTS))
def test_collate(pkg, layout, B, how):
    """One launch of four descriptors -- float rows, int32 words, a shared and a per-sample edge list -- with chunks 1, 255, 257 and
    11 * 179 (descriptors with short chunks return early under the grid of the longest)."""
    ins, outs, items = _collate_setup(dc.COLLATE_LAYOUTS[layout], B)
    ids = dc.collate_ids(how, B)
    oid = None if ids is None else ins.add(ids)
    din = ins.device()

    def run():
        dout = outs.device()
        descs = _descs(pkg, items, din, dout, dc.COLLATE_NPS)
        rc = pkg._lib.lib().dss2_collate(C.addressof(descs), 4, None if ids is None else _ptr(din, oid), B, _st(pkg))
        assert rc == 0, _last_error(pkg)
        torch.cuda.synchronize()
        return dout.cpu().numpy()

    got = run()
    assert np.array_equal(got, run()), "two launches from the same inputs differ in bits"
    _collate_check(got, outs, items, ids, B, dc.COLLATE_NPS, f"collate {layout} B={B} ids={how}")


def test_collate_adds_node_offsets_in_int64(pkg):
    """nodes_per_sample = 2^31 and three slots: the offsets are only added, and the sums must be the int64 ones."""
    B, nps = 3, 2 ** 31
    ins, outs, items = _collate_setup([(1, 0, 3), (1, 1, 1)], B, S=4)
    ids = np.array([2, 0, 3], np.int64)
    oid = ins.add(ids)
    din = ins.device()

    def run():
        dout = outs.device()
        descs = _descs(pkg, items, din, dout, nps)
        assert pkg._lib.lib().dss2_collate(C.addressof(descs), 2, _ptr(din, oid), B, _st(pkg)) == 0, _last_error(pkg)
        torch.cuda.synchronize()
        return dout.cpu().numpy()

    got = run()
    assert np.array_equal(got, run()), "two launches from the same inputs differ in bits"
    _collate_check(got, outs, items, ids, B, nps, "collate nodes_per_sample 2^31")
    assert _view(got, items[0][5], (2, 9), np.int64)[1, -1] == dc.collate_source(1, 0, 3, 4)[3, 1, 2] + 2 * 2 ** 31


def test_collate_refusals(pkg):
    B = 3
    ins, outs, items = _collate_setup(dc.COLLATE_LAYOUTS["B"], B)
    oid = ins.add(dc.collate_ids("reversed", B))
    din, dout = ins.device(), outs.device()
    L, st = pkg._lib.lib(), _st(pkg)
    good = _descs(pkg, items, din, dout, dc.COLLATE_NPS)
    five = (pkg._lib.CollateDesc * 5)(*([good[0]] * 5))
    assert L.dss2_collate(C.addressof(five), 5, _ptr(din, oid), B, st) == 2 and _last_error(pkg).startswith("collate:")
    for field, value in (("src", None), ("dst", None), ("chunk", 0)):
        descs = (pkg._lib.CollateDesc * 4)(*good)
        setattr(descs[2], field, value)
        assert L.dss2_collate(C.addressof(descs), 4, _ptr(din, oid), B, st) == 2 and "descriptor 2" in _last_error(pkg), field
        cur = torch.zeros(2, dtype=torch.int64, device=DEV)
        assert L.dss2_collate_cursor(C.addressof(descs), 4, _ptr(din, oid), cur.data_ptr(), B, 1, st) == 2, field
    assert L.dss2_collate(C.addressof(good), 4, _ptr(din, oid), 0, st) == 0
    cur = torch.tensor([1, 3], dtype=torch.int64, device=DEV)
    assert L.dss2_collate_cursor(C.addressof(good), 4, None, cur.data_ptr(), B, 1, st) == 2 and _last_error(pkg).startswith("collate_cursor:")
    assert L.dss2_collate_cursor(C.addressof(good), 4, _ptr(din, oid), None, B, 1, st) == 2 and _last_error(pkg).startswith("collate_cursor:")
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), outs.host()) and cur.tolist() == [1, 3], "a refused launch wrote"


@pytest.mark.parametrize("advance", [0, 1])
@pytest.mark.parametrize("case", dc.CURSOR_CASES, ids=lambda c: "len%d_batch%d_pos%d" % c)
def test_collate_cursor(pkg, case, advance):
    """Slot b reads sample_ids[(position + b) mod length] (no wrap when length <= 0); an advance leaves (position + batch) mod length,
    inside [0, length) also when the batch is longer than the epoch."""
    length, B, pos = case
    ins, outs, items = _collate_setup([(0, 0, 33), (1, 0, 5), (2, 0, 1)], B)
    ids = ((np.arange(dc.CURSOR_IDS) * 11) % dc.COLLATE_S).astype(np.int64)
    oid = ins.add(ids)
    ins.gap(GUARD)
    outs.gap(GUARD)
    ocur = outs.add(np.array([pos, length], np.int64))
    outs.gap(GUARD)
    din = ins.device()

    def run():
        dout = outs.device()
        descs = _descs(pkg, items, din, dout, dc.COLLATE_NPS)
        rc = pkg._lib.lib().dss2_collate_cursor(C.addressof(descs), 3, _ptr(din, oid), _ptr(dout, ocur), B, advance, _st(pkg))
        assert rc == 0, _last_error(pkg)
        torch.cuda.synchronize()
        return dout.cpu().numpy()

    got = run()
    assert np.array_equal(got, run()), "two launches from the same inputs differ in bits"
    _collate_check(got, outs, items, ids[dc.cursor_reads(length, B, pos)], B, dc.COLLATE_NPS, f"collate_cursor {case}", extra=[(ocur, 4)])
    cur = _view(got, ocur, (2,), np.int64).tolist()
    assert cur == [dc.cursor_next(length, B, pos) if advance else pos, length], (case, advance, cur)
    if advance and length > 0:
        assert 0 <= cur[0] < length


def _ragged_setup(m):
    mix = dc.ragged_mix(m)
    ins, outs, per_case = _Arena(dc.NAN_BITS), _Arena(dc.SENTINEL), []
    for k, cnt, tab in zip(mix["cases"], mix["counts"], mix["tables"]):
        if cnt == 0:
            per_case.append(None)          # a case with no item in the batch: null tables, null descriptors
            continue
        st = dc.ragged_store(k)
        per_case.append(dict(st=st, x=ins.add(st["x"]), y=ins.add(st["y"]), ea=ins.add(st["ea"]), ei=ins.add(st["ei"]),
                             samp=ins.add(tab["samp"]), noff=ins.add(tab["node_off"]), eoff=ins.add(tab["edge_off"]), cnt=cnt))
    ins.gap(GUARD)
    e_total = mix["E"] + dc.RAGGED_E_PAD
    o = dict(x=outs.out(mix["N"] * 11), y=outs.out(mix["N"] * 2), ea=outs.out(mix["E"] * 13), ei=outs.out(2 * 2 * e_total))
    return mix, ins, outs, per_case, o, e_total


def _ragged_descs(pkg, pc, o, din, dout, descs, at):
    st = pc["st"]
    n, e = st["n"], st["e"]
    rows = [(pc["x"], o["x"], n * 11, 0, 0, 11), (pc["y"], o["y"], n * 2, 0, 0, 2), (pc["ea"], o["ea"], e * 13, 0, 1, 13),
            (pc["ei"], o["ei"], e, 1, st["shared"], 0)]
    for i, (so, do, chunk, kind, shared, width) in enumerate(rows):
        d = descs[at + i]
        d.src, d.dst, d.chunk, d.kind, d.shared, d.nodes_per_sample = _ptr(din, so), _ptr(dout, do), chunk, kind, shared, width


def _ragged_multi(pkg, per_case, o, e_total, din, outs):
    dout, nc = outs.device(), len(per_case)
    descs = (pkg._lib.CollateDesc * (4 * nc))()
    samp, noff, eoff, cnt = (C.c_void_p * nc)(), (C.c_void_p * nc)(), (C.c_void_p * nc)(), (C.c_int64 * nc)()
    for k, pc in enumerate(per_case):
        if pc is None:
            continue
        _ragged_descs(pkg, pc, o, din, dout, descs, 4 * k)
        samp[k], noff[k], eoff[k], cnt[k] = _ptr(din, pc["samp"]), _ptr(din, pc["noff"]), _ptr(din, pc["eoff"]), pc["cnt"]
    rc = pkg._lib.lib().dss2_collate_ragged_multi(C.addressof(descs), nc, 4, C.addressof(samp), C.addressof(noff), C.addressof(eoff),
                                                  C.addressof(cnt), e_total, _st(pkg))
    assert rc == 0, _last_error(pkg)
    torch.cuda.synchronize()
    return dout.cpu().numpy()


def _ragged_single(pkg, per_case, o, e_total, din, outs):
    dout = outs.device()
    for pc in per_case:
        if pc is None:
            continue
        descs = (pkg._lib.CollateDesc * 4)()
        _ragged_descs(pkg, pc, o, din, dout, descs, 0)
        rc = pkg._lib.lib().dss2_collate_ragged(C.addressof(descs), 4, _ptr(din, pc["samp"]), _ptr(din, pc["noff"]), _ptr(din, pc["eoff"]),
                                                pc["cnt"], e_total, _st(pkg))
        assert rc == 0, _last_error(pkg)
    torch.cuda.synchronize()
    return dout.cpu().numpy()


@pytest.mark.parametrize("m", range(len(dc.RAGGED_MIXES)), ids=lambda m: "cases%s_counts%s" % tuple("-".join(map(str, v)) for v in dc.RAGGED_MIXES[m]))
def test_collate_ragged(pkg, m):
    """A batch whose slots interleave up to four cases of different bus and branch counts: the one ``_multi`` launch and a
    ``dss2_collate_ragged`` call per case leave the same bits, those of numpy indexing; the edge list's row stride is e_total."""
    mix, ins, outs, per_case, o, e_total = _ragged_setup(m)
    din = ins.device()
    multi = _ragged_multi(pkg, per_case, o, e_total, din, outs)
    assert np.array_equal(multi, _ragged_multi(pkg, per_case, o, e_total, din, outs)), "two launches from the same inputs differ in bits"
    single = _ragged_single(pkg, per_case, o, e_total, din, outs)
    N, E = mix["N"], mix["E"]
    for name, got in (("dss2_collate_ragged_multi", multi), ("dss2_collate_ragged", single)):
        for key, shape in (("x", (N, 11)), ("y", (N, 2)), ("ea", (E, 13))):
            res = _view(got, o[key], shape, np.float32)
            bad = np.argwhere(_bits(res) != _bits(mix[key]))
            assert bad.size == 0, (name, key, f"{len(bad)} cells differ, first {bad[:4].tolist()}")
        ei = _view(got, o["ei"], (2, e_total), np.int64)
        assert np.array_equal(ei[:, :E], mix["ei"]), (name, "edge_index", np.argwhere(ei[:, :E] != mix["ei"])[:4].tolist())
        _only_written(got, outs, [(o["x"], N * 11), (o["y"], N * 2), (o["ea"], E * 13), (o["ei"], 2 * E), (o["ei"] + 2 * e_total, 2 * E)], name)
    assert np.array_equal(multi, single), "the single-case entry point and the one launch of all cases differ in bits"


def test_collate_ragged_refusals(pkg):
    mix, ins, outs, per_case, o, e_total = _ragged_setup(1)
    din, dout = ins.device(), outs.device()
    L, st, CD = pkg._lib.lib(), _st(pkg), pkg._lib.CollateDesc
    nc = len(per_case)
    descs = (CD * (4 * 5))()
    for k, pc in enumerate(per_case):
        _ragged_descs(pkg, pc, o, din, dout, descs, 4 * k)

    def tables(n=nc):
        samp, noff, eoff, cnt = (C.c_void_p * 5)(), (C.c_void_p * 5)(), (C.c_void_p * 5)(), (C.c_int64 * 5)()
        for k, pc in enumerate(per_case[:n]):
            samp[k], noff[k], eoff[k], cnt[k] = _ptr(din, pc["samp"]), _ptr(din, pc["noff"]), _ptr(din, pc["eoff"]), pc["cnt"]
        return samp, noff, eoff, cnt

    def multi(samp, noff, eoff, cnt, n=nc, d=descs):
        return L.dss2_collate_ragged_multi(C.addressof(d), n, 4, C.addressof(samp), C.addressof(noff), C.addressof(eoff), C.addressof(cnt), e_total, st)

    assert multi(*tables(), n=5) == 2 and _last_error(pkg).startswith("collate_ragged_multi:")
    assert multi(*tables(), n=0) == 2
    samp, noff, eoff, cnt = tables()
    cnt[0] = cnt[1] = 0
    assert multi(samp, noff, eoff, cnt) == 0, "all counts 0: nothing to do"
    for which in range(3):
        tabs = tables()
        tabs[which][1] = None
        assert multi(*tabs) == 2 and "case 1" in _last_error(pkg), which
    for field, value in (("src", None), ("dst", None), ("chunk", 0)):
        d2 = (CD * (4 * 5))(*descs)
        setattr(d2[4 + 3], field, value)
        assert multi(*tables(), d=d2) == 2 and "descriptor 3 of case 1" in _last_error(pkg), field
    pc = per_case[0]
    one = (CD * 5)(*descs[0:4], descs[0])
    args = (_ptr(din, pc["samp"]), _ptr(din, pc["noff"]), _ptr(din, pc["eoff"]))
    assert L.dss2_collate_ragged(C.addressof(one), 4, *args, 0, e_total, st) == 0
    assert L.dss2_collate_ragged(C.addressof(one), 5, *args, pc["cnt"], e_total, st) == 2 and _last_error(pkg).startswith("collate_ragged:")
    for which in range(3):
        a = list(args)
        a[which] = None
        assert L.dss2_collate_ragged(C.addressof(one), 4, *a, pc["cnt"], e_total, st) == 2, which
    one[1].src = None
    assert L.dss2_collate_ragged(C.addressof(one), 4, *args, pc["cnt"], e_total, st) == 2 and "descriptor 1" in _last_error(pkg)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), outs.host()), "a refused launch wrote"


def test_accum_scalar(pkg):
    L, st = pkg._lib.lib(), _st(pkg)
    outs = _Arena(dc.SENTINEL)
    outs.gap(GUARD)
    oacc = outs.add(np.zeros(2, np.float64))
    outs.gap(GUARD)
    vals = np.array([0.1, 1.0e8, -3.25, np.nan], np.float32)
    dv = torch.from_numpy(vals).to(DEV)
    dout = outs.device()
    want = 0.0
    for i in range(3):
        assert L.dss2_accum_scalar(_ptr(dout, oacc), dv.data_ptr() + 4 * i, st) == 0, _last_error(pkg)
        want += float(vals[i])
    torch.cuda.synchronize()
    got = dout.cpu().numpy()
    acc = _view(got, oacc, (2,), np.float64)
    assert acc[0] == want and acc[1] == 3.0, (acc.tolist(), want)
    assert L.dss2_accum_scalar(_ptr(dout, oacc), dv.data_ptr() + 12, st) == 0
    assert L.dss2_accum_scalar(None, dv.data_ptr(), st) == 2 and _last_error(pkg).startswith("accum_scalar:")
    assert L.dss2_accum_scalar(_ptr(dout, oacc), None, st) == 2
    torch.cuda.synchronize()
    got = dout.cpu().numpy()
    acc = _view(got, oacc, (2,), np.float64)
    assert np.isnan(acc[0]) and acc[1] == 4.0
    _only_written(got, outs, [(oacc, 4)], "accum_scalar")


# ------------------------------------------------------------------------------------------
# D. the Python layer above them (dataset.py)
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parts(pkg):
    """Six single-grid parts normalised with common statistics: (grid, samples) = cigre14 5, reswitched 4, ober_sub 3, cigre14 6,
    reswitched 4, cigre14 3 -- bus counts 15, 15, 70, 15, 15, 15; branch counts 14, 15, 69, 14, 15, 14."""
    stats = pkg.synthetic.make_batch(["cigre14"], 8, seed=0)["stats"]
    spec = [("cigre14", 5), ("cigre14_reswitched", 4), ("ober_sub", 3), ("cigre14", 6), ("cigre14_reswitched", 4), ("cigre14", 3)]
    return [pkg.dataset.DeviceDataset.from_batch(pkg.synthetic.make_batch([g], S, seed=11 + k, stats=stats), device=DEV)
            for k, (g, S) in enumerate(spec)]


def _oracle_batch(ds, ids):
    import dss2_dataset_oracle as dso
    xs, eis, eas, ys = [], [], [], []
    for g in ids:
        k = int(np.searchsorted(ds.start, g, side="right") - 1)
        p, s = ds.parts[k], int(g - ds.start[k])
        xs.append(p.x[s].cpu()); eas.append(p.edge_attr[s].cpu()); ys.append(p.y[s].cpu())
        eis.append(p.edge_index[s if p.edge_index.size(0) == p.S else 0].cpu())
    return dso.collate(xs, eis, eas, ys), np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])])


def _same(bt, want):
    x, ei, ea, y = want
    return (torch.equal(bt.x.cpu(), x) and torch.equal(bt.edge_index.cpu(), ei) and torch.equal(bt.edge_attr.cpu(), ea)
            and torch.equal(bt.y.cpu(), y))


@pytest.mark.parametrize("which", ["same3", "same4", "same5", "mixed3", "mixed4", "mixed5"])
def test_mixed_dataset_of_three_to_five_parts(pkg, parts, which):
    """3 and 4 parts go through the one ``_multi`` launch, 5 through a launch per case; with equal and with different bus counts (the
    latter carry graph_ptr and max_nodes); one batch draws nothing from part 1.  Every batch = the oracle's collate of its samples."""
    sel = {"same3": [0, 1, 3], "same4": [0, 1, 3, 4], "same5": [0, 1, 3, 4, 5], "mixed3": [0, 2, 1], "mixed4": [0, 2, 1, 3], "mixed5": [0, 2, 1, 3, 4]}[which]
    ds = pkg.dataset.MixedDataset([parts[k] for k in sel])
    total = len(ds)
    rng = np.random.default_rng(len(sel))
    perm = rng.permutation(total).astype(np.int64)
    skip1 = np.array([g for g in perm if not ds.start[1] <= g < ds.start[2]], np.int64)[:7]
    for ids in (perm[:9], perm[9:], skip1, perm[:1]):
        bt = ds.collate(ids)
        want, ptr = _oracle_batch(ds, ids)
        assert bt.num_graphs == len(ids) and _same(bt, want), (which, ids.tolist())
        if which.startswith("mixed"):
            assert bt.max_nodes == 70 and bt.graph_ptr.cpu().tolist() == ptr.tolist()
        else:
            assert bt.graph_ptr is None and bt.max_nodes is None
    if len(sel) == 5:      # a batch of the 5-part set that draws from parts 0..3 only = the same batch of the 4-part set
        four = pkg.dataset.MixedDataset([parts[k] for k in sel[:4]])
        ids = np.array([g for g in perm if g < ds.start[4]], np.int64)[:10]
        a, b = ds.collate(ids), four.collate(ids)
        assert _same(a, (b.x.cpu(), b.edge_index.cpu(), b.edge_attr.cpu(), b.y.cpu()))


def test_device_dataset_with_per_sample_edge_lists(pkg, parts):
    """Two branch sets of equal size: no shared topology, the batch edge list is gathered per batch and never cached."""
    import dss2_dataset_oracle as dso
    p = parts[3]
    ei = p.edge_index.clone()
    ei[1::2, 1, -1] = (ei[1::2, 1, -1] + 1) % p.n          # odd samples: the last branch ends one bus further
    ds = pkg.dataset.DeviceDataset(p.x, p.edge_attr, p.y, ei)
    assert not ds.shared_topology and ds.e == p.e
    outs = []
    for ids in ([0, 1, 2], [1, 2, 3], [5, 5, 0]):
        bt = ds.collate(torch.tensor(ids, device=DEV))
        want = dso.collate([ds.x[s].cpu() for s in ids], [ei[s].cpu() for s in ids], [ds.edge_attr[s].cpu() for s in ids], [ds.y[s].cpu() for s in ids])
        assert _same(bt, want), ids
        outs.append(bt.edge_index)
    assert not torch.equal(outs[0], outs[1]) and outs[0].data_ptr() != outs[1].data_ptr() and not ds._ei_cache


def test_data_from_tables_small(pkg):
    """S = 3, n = 5, e = 4: raw columns and labels exact, the zero pattern the oracle's, statistics inside the z-score's bounds against
    float64 of the un-normalised features, normalised features bit-equal to the oracle run with the device statistics.
    One departure: column 3 of x is constant, the oracle's OWN statistics turn it into +-1 of rounding noise
    (tests/test_dataset_kernel_cases_cpu.py asserts that), so its zero pattern is taken from the oracle run with the device statistics
    only; every other column's is also the pattern of the oracle's own run."""
    import dss2_dataset_oracle as dso
    T = dc.small_tables()
    ds, *stats = pkg.dataset.data_from_tables(T["nodes"], T["edges"], T["labels"], T["noise"], 8, 6, T["meas_v"], T["meas_pflow"], device=DEV,
                                              z_nodes=T["z_nodes"], z_edges=T["z_edges"])
    stats = [s.cpu() for s in stats]
    keys = ("nodes", "edges", "labels", "noise", "meas_v", "meas_pflow", "z_nodes", "z_edges")
    own = dso.data_from_tables(*(T[k] for k in keys))
    ref = dso.data_from_tables(*(T[k] for k in keys), stats=dict(zip(("x_mean", "x_std", "edge_mean", "edge_std"), stats)))
    x, ea = ds.x.reshape(-1, 11).cpu(), ds.edge_attr.reshape(-1, 13).cpu()
    assert torch.equal(x[:, 8:], ref["x"][:, 8:]) and torch.equal(ea[:, 6:], ref["edge_attr"][:, 6:]) and torch.equal(ds.y.reshape(-1, 2).cpu(), ref["y"])
    raw_x = np.concatenate([dso.measure_nodes(T["nodes"][i, :, 0:4], T["nodes"][i, :, 5], T["nodes"][i, :, 6], T["meas_v"], T["noise"], T["z_nodes"][i]).numpy() for i in range(3)])
    raw_e = np.concatenate([dso.measure_edges(T["edges"][i, :, 2:4], T["edges"][i, :, 4:6], T["meas_pflow"], T["noise"], T["z_edges"][i]).numpy() for i in range(3)])
    # The zero pattern is the oracle's own, except in a column whose measured entries are all one value (the weight of theta at the
    # slack bus): the oracle's fp32 column sum puts its mean an ulp off and its z-scores at +-1 of rounding noise; the device gives 0.
    const = [c for c in range(8) if len(np.unique(raw_x[:, c][raw_x[:, c] != 0])) == 1]
    keep = [c for c in range(11) if c not in const]
    assert const == [3] and (x[:, 3] == 0).all()
    assert torch.equal(x[:, keep] == 0, own["x"][:, keep] == 0) and torch.equal(ea == 0, own["edge_attr"] == 0)
    assert np.array_equal(_bits(x.numpy()), _bits(ref["x"].numpy())) and np.array_equal(_bits(ea.numpy()), _bits(ref["edge_attr"].numpy()))
    assert all(torch.equal(ds.edge_index[s].cpu(), own["edge_index"][s]) for s in range(3))
    for raw, nf, mean, std, name in ((raw_x, 8, stats[0], stats[1], "x"), (raw_e, 6, stats[2], stats[3], "edge_attr")):
        n, mean64, std64 = dc.stats64(raw, nf)
        em, es = np.abs(mean.numpy().astype(np.float64) - mean64), np.abs(std.numpy().astype(np.float64) - std64)
        print(f"[data_from_tables {name}] |mean err| / bound {np.max(em / np.maximum(dc.ZS_MEAN_BOUND * np.abs(mean64), 1e-300)):.3f}  "
              f"|std err| / bound {np.max(es / np.maximum(dc.ZS_STD_BOUND * std64, 1e-300)):.3f}")
        assert (em <= dc.ZS_MEAN_BOUND * np.abs(mean64)).all() and (es <= dc.ZS_STD_BOUND * std64).all(), name
