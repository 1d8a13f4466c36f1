"""GPU: the weight-space kernels of csrc/dss2_weightspace.hpp on their own -- ``dss2_small_gemm``, ``dss2_pack_weights`` (fp32 and
bf16x3 layouts) and ``dss2_reduce_slabs`` / ``dss2_reduce_slabs_multi`` driven through ctypes with hand-built tables, against the
plain references of tests/weightspace_cases.py, at the shapes, flags and offsets the models never produce.

Every operand sits in one device buffer with NaN in all gaps (a load outside a logical extent poisons the result) and every output
in one buffer prefilled with a sentinel bit pattern (gaps, guard bands and unwritten cells must keep it bit for bit).  Integer data
must give the fp64 result exactly (all partial sums are below 2^24, so no order of summation can differ): a dropped, doubled or
misplaced term cannot hide.  N(0,1) data must stay, component by component, inside the bound of a chain of fp32 roundings:
(nbatch K + 8) 2^-24 (sum |a||b| + |u v| + |C_old|) for the GEMM, n_slabs 2^-24 sum |slab| for the reductions.  Every launch runs
twice from the same inputs with equal bits; each parametrisation is ONE launch of many descriptors (blockIdx.y dispatch, early
return of the descriptors with fewer tiles / elements / blocks than the largest).

Measured on the MI355X, worst |error| / bound over the cases of a group:
  small GEMM, by shape M x N x K (nbatch), the largest of the four transposition pairs (x accumulate x rank-1 x pointer / offset):
    1x1x1 0.100    32x32x128 0.011    33x31x129 0.011    64x96x384 0.004    5x70x385 0.003    40x1x50 0.030    1x40x50 0.033
    7x9x0 0.172    33x34x130 (2) 0.006    33x34x130 (4) 0.004
  reductions, by form, the batched and the single entry point alike (their bits are equal):
    vector 0.081    tall 0.002    scalar 0.397    the mixed launch of 32 descriptors 0.431
All integer cases are exact.

What these tests cannot see: a re-partitioning of the 16-byte form's slab loop that keeps each lane's additions in the same
sequence (for instance an unrolled pass that stops one step earlier and leaves the rest to the remainder loop) gives the same
bits from both entry points, which share one device body, so no comparison of results can tell it from the original.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import weightspace_cases as wc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


class _Arena:
    """int32 images of host arrays laid end to end, each starting ``mis`` elements past a 16-byte boundary, the space between
    them holding ``fill``; ``device()`` uploads a fresh copy and ``ptr`` turns an element offset into a device address."""

    def __init__(self, fill):
        self.fill, self.parts, self.n = fill, [], 0

    def gap(self, n):
        self.parts.append(np.full(n, self.fill, np.int32))
        self.n += n

    def add(self, a, mis=0):
        self.gap((-self.n) % 4 + mis)
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize == 4
        off = self.n
        self.parts.append(a.reshape(-1).view(np.int32))
        self.n += a.size
        return off

    def host(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, np.int32)

    def device(self):
        t = torch.from_numpy(self.host()).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t


def _ptr(t, off):
    return t.data_ptr() + 4 * off


def _last_error(pkg):
    return (pkg._lib.lib().dss2_last_error() or b"").decode()


# ------------------------------------------------------------------------------------------
# small GEMM
# ------------------------------------------------------------------------------------------
_GEMM = {}


def _gemm_setup(tA, tB, data):
    """(operand descriptions, input arena, output arena, per-case offsets) of one launch; made once."""
    key = (tA, tB, data)
    if key not in _GEMM:
        cases = wc.gemm_cases(tA, tB)
        descs = [wc.gemm_operands(c, data, seed=100 * i + 10 * tA + tB) for i, c in enumerate(cases)]
        ins, outs, offs = _Arena(NAN_BITS), _Arena(wc.SENTINEL), []
        for d in descs:
            c = d["case"]
            o = dict(A=[ins.add(a) for a in d["A"]], B=[ins.add(b) for b in d["B"]],
                     u=ins.add(d["u"]) if c.uv else None, v=ins.add(d["v"]) if c.uv else None)
            blk = np.full((c.M, c.ldc), wc.SENTINEL, np.int32)
            if c.accumulate:
                blk[:, :c.N] = d["C_old"].view(np.int32)
            outs.gap(wc.GEMM_C_GUARD)
            o["C"] = outs.add(blk)
            outs.gap(wc.GEMM_C_GUARD)
            offs.append(o)
        # behind the operands: NaN as far as a read with the wrong transposition of the largest operand would reach, so that
        # such a defect shows as a wrong number, not as a fault
        ins.gap((max(max(s[:3]) for s in wc.GEMM_SHAPES) + 8) ** 2)
        _GEMM[key] = (descs, ins, outs, offs)
    return _GEMM[key]


def _gemm_table(pkg, descs, offs, din, dout):
    arr = np.zeros(len(descs), dtype=pkg.plans._SG_DTYPE)
    for r, d, o in zip(arr, descs, offs):
        c = d["case"]
        for b in range(c.nbatch):
            r["A"][b], r["B"][b] = _ptr(din, o["A"][b]), _ptr(din, o["B"][b])
        if c.uv:
            r["u"], r["v"] = _ptr(din, o["u"]), _ptr(din, o["v"])
        if c.c_by_offset:
            r["C"], r["c_off"] = 0, o["C"]
        else:
            r["C"], r["c_off"] = _ptr(dout, o["C"]), -1
        r["M"], r["N"], r["K"], r["lda"], r["ldb"], r["ldc"] = c.M, c.N, c.K, c.lda, c.ldb, c.ldc
        r["transA"], r["transB"], r["nbatch"], r["accumulate"] = c.tA, c.tB, c.nbatch, c.accumulate
    return torch.from_numpy(arr.view(np.uint8).copy()).to(DEV)


def _gemm_run(pkg, descs, ins, outs, offs, din):
    dout = outs.device()
    tab = _gemm_table(pkg, descs, offs, din, dout)
    mx = max(d["case"].tiles for d in descs)
    rc = pkg._lib.lib().dss2_small_gemm(tab.data_ptr(), len(descs), mx, dout.data_ptr(), pkg._lib.stream_ptr(DEV))
    assert rc == 0, _last_error(pkg)
    torch.cuda.synchronize()
    return dout.cpu().numpy()


@pytest.mark.parametrize("data", ["int", "normal"])
@pytest.mark.parametrize("tA,tB", wc.GEMM_TRANS, ids=["NN", "NT", "TN", "TT"])
def test_small_gemm(pkg, tA, tB, data):
    descs, ins, outs, offs = _gemm_setup(tA, tB, data)
    din = ins.device()
    got = _gemm_run(pkg, descs, ins, outs, offs, din)
    again = _gemm_run(pkg, descs, ins, outs, offs, din)
    assert np.array_equal(got, again), "two launches from the same inputs differ in bits"
    untouched = outs.host().copy()
    worst = {}
    for d, o in zip(descs, offs):
        c = d["case"]
        blk = got[o["C"]:o["C"] + c.M * c.ldc].reshape(c.M, c.ldc)
        res = np.ascontiguousarray(blk[:, :c.N]).view(np.float32)
        want = wc.ref_gemm(d)
        if data == "int":
            assert torch.equal(torch.from_numpy(res), torch.from_numpy(want).float()), c.name
        else:
            err, bound = np.abs(res.astype(np.float64) - want), wc.gemm_bound(d)
            assert np.isfinite(res).all() and (err <= bound).all(), (c.name, float((err / np.maximum(bound, 1e-300)).max()))
            ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
            shape = f"{c.M}x{c.N}x{c.K}({c.nbatch})"
            worst[shape] = max(worst.get(shape, 0.0), ratio)
        untouched[o["C"]:o["C"] + c.M * c.ldc].reshape(c.M, c.ldc)[:, :c.N] = blk[:, :c.N]
    assert np.array_equal(got, untouched), "a gap of C or a guard band lost its sentinel"
    if worst:
        print(f"[small_gemm {'T' if tA else 'N'}{'T' if tB else 'N'}] worst |error| / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_small_gemm_refusals(pkg):
    descs, ins, outs, offs = _gemm_setup(0, 0, "int")
    din, dout = ins.device(), outs.device()
    tab = _gemm_table(pkg, descs, offs, din, dout)
    lib, st = pkg._lib.lib(), pkg._lib.stream_ptr(DEV)
    for mt in (0, -1):
        assert lib.dss2_small_gemm(tab.data_ptr(), len(descs), mt, dout.data_ptr(), st) == 2
        assert _last_error(pkg).startswith("small_gemm:")
    assert lib.dss2_small_gemm(tab.data_ptr(), 0, 6, dout.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), outs.host()), "a refused launch wrote"


# ------------------------------------------------------------------------------------------
# weight packing
# ------------------------------------------------------------------------------------------
_PACK = {}


def _pack_setup(layout):
    if layout not in _PACK:
        kgroup = 8 if layout == "fp32" else 16
        ins, outs, recs, groups = _Arena(NAN_BITS), _Arena(wc.SENTINEL), [], []
        for gi, g in enumerate(wc.PACK_GROUPS):
            srcs, logical = wc.pack_sources(g, seed=40 + gi)
            kpad = g.kpad(kgroup)
            words = kpad * 32 * g.ncg if layout == "fp32" else 3 * kpad * 32 * g.ncg // 2
            outs.gap(8)
            dst = outs.add(np.full(words, wc.SENTINEL, np.int32))
            outs.gap(8)
            for b, s in zip(g.blocks, srcs):
                recs.append((ins.add(s), dst, b.rows, b.cols, b.ld, b.transpose | (0 if layout == "fp32" else 2), b.koff, kpad, g.ncg, b.joff))
            want = wc.expected_fp32(g, logical) if layout == "fp32" else wc.expected_bf16x3(g, logical).view(np.int32)
            assert want.size == words
            groups.append((g, logical, dst, kpad, want))
        max_elems = max(wc.pack_block_elems(b, kgroup) for g in wc.PACK_GROUPS for b in g.blocks)
        _PACK[layout] = (ins, outs, recs, groups, max_elems)
    return _PACK[layout]


def _pack_run(pkg, ins, outs, recs, max_elems, din):
    dout = outs.device()
    arr = np.array([(_ptr(din, r[0]), _ptr(dout, r[1])) + r[2:] for r in recs], dtype=pkg.plans._DESC_DTYPE)
    tab = torch.from_numpy(arr.view(np.uint8).copy()).to(DEV)
    rc = pkg._lib.lib().dss2_pack_weights(tab.data_ptr(), len(recs), max_elems, pkg._lib.stream_ptr(DEV))
    assert rc == 0, _last_error(pkg)
    torch.cuda.synchronize()
    return dout.cpu().numpy()


@pytest.mark.parametrize("layout", ["fp32", "bf16x3"])
def test_pack_weights(pkg, layout):
    ins, outs, recs, groups, max_elems = _pack_setup(layout)
    din = ins.device()
    got = _pack_run(pkg, ins, outs, recs, max_elems, din)
    again = _pack_run(pkg, ins, outs, recs, max_elems, din)
    assert np.array_equal(got, again), "two launches from the same inputs differ in bits"
    expect = outs.host().copy()
    for g, logical, dst, kpad, want in groups:
        buf = got[dst:dst + want.size]
        if layout == "bf16x3":      # the pieces of every written element sum to the source exactly
            planes = wc.unpack_bf16x3(buf.view(np.int16), kpad, g.ncg)
            for b, w in zip(g.blocks, logical):
                sl = (slice(b.koff, b.koff + b.K), slice(b.joff, b.joff + b.J))
                h, m, l = (torch.from_numpy(np.ascontiguousarray(p[sl])).view(torch.bfloat16).double() for p in planes)
                assert torch.equal(h + m + l, torch.from_numpy(np.ascontiguousarray(w)).double()), (g.name, b)
        bad = np.flatnonzero(buf != want)
        assert bad.size == 0, (g.name, f"{bad.size} of {want.size} words differ, first at {bad[:4]}")
        expect[dst:dst + want.size] = want
    assert np.array_equal(got, expect), "a guard band between the packed matrices lost its sentinel"


# ------------------------------------------------------------------------------------------
# slab reductions
# ------------------------------------------------------------------------------------------
_REDUCE = {}


def _reduce_setup(name, cases, data):
    key = (name, data)
    if key not in _REDUCE:
        ins, outs, items = _Arena(NAN_BITS), _Arena(wc.SENTINEL), []
        for i, c in enumerate(cases):
            slab = wc.reduce_operands(c, data, seed=7 * i + 1)
            so = ins.add(slab, mis=c.slab_off)
            oo = outs.add(np.full(c.len, wc.SENTINEL, np.int32), mis=c.out_off)
            outs.gap(wc.REDUCE_OUT_GUARD)
            items.append((c, so, oo) + wc.ref_reduce(c, slab))
        _REDUCE[key] = (ins, outs, items)
    return _REDUCE[key]


def _reduce_descs(pkg, items, din, dout):
    descs = (pkg._lib.ReduceDesc * len(items))()
    for d, (c, so, oo, _, _) in zip(descs, items):
        d.slab, d.out, d.stride, d.len, d.n_slabs = _ptr(din, so), _ptr(dout, oo), c.stride, c.len, c.n_slabs
        form = "scalar" if (c.stride % 4 or d.slab % 16 or d.out % 16) else ("tall" if c.n_slabs >= 256 and c.len <= 8192 else "vector")
        assert form == wc.reduce_form(c), "the addresses on the device do not have the alignment the case asks for"
    return descs


def _reduce_multi(pkg, outs, items, din):
    dout = outs.device()
    descs = _reduce_descs(pkg, items, din, dout)
    rc = pkg._lib.lib().dss2_reduce_slabs_multi(C.addressof(descs), len(items), pkg._lib.stream_ptr(DEV))
    assert rc == 0, _last_error(pkg)
    torch.cuda.synchronize()
    return dout.cpu().numpy()


def _reduce_single(pkg, outs, items, din):
    dout = outs.device()
    lib, st = pkg._lib.lib(), pkg._lib.stream_ptr(DEV)
    for c, so, oo, _, _ in items:
        rc = lib.dss2_reduce_slabs(_ptr(din, so), c.n_slabs, c.stride, _ptr(dout, oo), c.len, st)
        assert rc == 0, (c.name, _last_error(pkg))
    torch.cuda.synchronize()
    return dout.cpu().numpy()


def _reduce_check(got, outs, items, data, what):
    """Values against fp64 (exact for integers, inside the bound otherwise), sentinels everywhere else; the worst ratio."""
    expect, worst = outs.host().copy(), 0.0
    for c, so, oo, want, bound in items:
        res = got[oo:oo + c.len].view(np.float32)
        if data == "int":
            assert torch.equal(torch.from_numpy(res), torch.from_numpy(want).float()), (what, c.name)
        elif c.len:
            err = np.abs(res.astype(np.float64) - want)
            assert np.isfinite(res).all() and (err <= bound).all(), (what, c.name, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
        expect[oo:oo + c.len] = got[oo:oo + c.len]
    assert np.array_equal(got, expect), f"{what}: a guard behind an output lost its sentinel"
    return worst


@pytest.mark.parametrize("data", ["int", "normal"])
@pytest.mark.parametrize("form", ["vector", "tall", "scalar"])
def test_reduce_slabs(pkg, form, data):
    ins, outs, items = _reduce_setup(form, wc.REDUCE_CASES[form], data)
    din = ins.device()
    multi = _reduce_multi(pkg, outs, items, din)
    assert np.array_equal(multi, _reduce_multi(pkg, outs, items, din)), "two batched launches from the same inputs differ in bits"
    single = _reduce_single(pkg, outs, items, din)
    wm = _reduce_check(multi, outs, items, data, "dss2_reduce_slabs_multi")
    ws = _reduce_check(single, outs, items, data, "dss2_reduce_slabs")
    for c, so, oo, _, _ in items:
        assert np.array_equal(multi[oo:oo + c.len], single[oo:oo + c.len]), f"{c.name}: batched and single entry point differ in bits"
    if data == "normal":
        print(f"[reduce_slabs {form}] worst |error| / bound: batched {wm:.3f}  single {ws:.3f}")


def test_reduce_slabs_multi_full_table_equals_single_calls(pkg):
    """32 descriptors of all three forms and one empty reduction in one launch = 32 single calls, bit for bit."""
    ins, outs, items = _reduce_setup("mix", wc.REDUCE_MIX, "normal")
    assert len(items) == 32
    din = ins.device()
    multi, single = _reduce_multi(pkg, outs, items, din), _reduce_single(pkg, outs, items, din)
    wm = _reduce_check(multi, outs, items, "normal", "dss2_reduce_slabs_multi")
    _reduce_check(single, outs, items, "normal", "dss2_reduce_slabs")
    for c, so, oo, _, _ in items:
        assert np.array_equal(multi[oo:oo + c.len], single[oo:oo + c.len]), f"{c.name}: batched and single entry point differ in bits"
    assert np.array_equal(multi, single)
    print(f"[reduce_slabs mix of 32] worst |error| / bound: {wm:.3f}")


def test_reduce_slabs_multi_refusals(pkg):
    ins, outs, items = _reduce_setup("mix", wc.REDUCE_MIX, "normal")
    din, dout = ins.device(), outs.device()
    lib, st = pkg._lib.lib(), pkg._lib.stream_ptr(DEV)
    good = _reduce_descs(pkg, items, din, dout)

    def refused(descs, n):
        assert lib.dss2_reduce_slabs_multi(C.addressof(descs), n, st) == 2
        assert _last_error(pkg).startswith("reduce_slabs_multi:"), _last_error(pkg)

    many = (pkg._lib.ReduceDesc * 33)(*([good[0]] * 33))
    refused(many, 33)
    for field, value in (("slab", None), ("n_slabs", 0), ("len", -1)):
        descs = (pkg._lib.ReduceDesc * 3)(good[0], good[1], good[2])
        setattr(descs[1], field, value)
        refused(descs, 3)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), outs.host()), "a refused launch wrote"
