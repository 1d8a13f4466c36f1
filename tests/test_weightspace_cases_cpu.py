"""CPU: the references and case tables of tests/weightspace_cases.py are fit to judge the weight-space kernels on the GPU.

* ``unpack(pack(B)) == B`` bit for bit in both packing layouts, the packed image agrees with the layout text of include/dss2_hip.h
  element by element, blocks at odd K, J and nonzero koff / joff land where the text says and every other cell keeps its sentinel;
* every reduction case resolves (``reduce_form``) to the form its table entry names, all three forms and both sides of every
  boundary (n_slabs 255 / 256, len 8192 / 8196) are present, every listed size appears at least twice, the scalar form is reached
  in all three ways, and the mixed launch fills the 32 descriptors with one empty reduction among them;
* the integer data of every GEMM and reduction case is exact in fp32: the largest possible |partial sum| is below 2^24;
* the bf16 split reference sums back to its input exactly in fp64, for N(0,1) draws scaled by 1, 1e-3 and 300;
* the ctypes mirrors have the sizes of the numpy table dtypes and of the header's structs;
* ``ref_gemm`` on operands with NaN gaps equals a plain float64 product of the logical matrices."""
import collections
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import weightspace_cases as wc
from conftest import load_pkg


# ---- packing references
def _fp32_flat(k, j, kpad):
    """Flat element index of B[k][j] in [ncg][kpad/8][64 lanes][4], spelled out from the header's sentence."""
    cg, c32, kg, half, s = j // 32, j % 32, k // 8, (k % 8) // 4, k % 4
    return ((cg * (kpad // 8) + kg) * 64 + half * 32 + c32) * 4 + s


def _bf16_flat(k, j, plane, kpad):
    cg, c32, kg, half, q = j // 32, j % 32, k // 16, (k % 16) // 8, k % 8
    return (((cg * (kpad // 16) + kg) * 3 + plane) * 64 + half * 32 + c32) * 8 + q


@pytest.mark.parametrize("kpad,ncg", [(8, 1), (24, 2), (40, 3)])
def test_fp32_pack_roundtrip_and_element_positions(kpad, ncg):
    B = np.arange(kpad * 32 * ncg, dtype=np.int32).reshape(kpad, 32 * ncg) * 7 + 3
    buf = wc.pack_fp32(B, kpad, ncg)
    assert buf.shape == (kpad * 32 * ncg,) and buf.dtype == B.dtype
    assert np.array_equal(wc.unpack_fp32(buf, kpad, ncg), B)
    assert np.array_equal(wc.pack_fp32(wc.unpack_fp32(buf, kpad, ncg), kpad, ncg), buf)
    for k in range(kpad):
        for j in range(32 * ncg):
            assert buf[_fp32_flat(k, j, kpad)] == B[k, j], (k, j)


@pytest.mark.parametrize("kpad,ncg", [(16, 1), (32, 2), (48, 3)])
def test_bf16x3_pack_roundtrip_and_element_positions(kpad, ncg):
    n = kpad * 32 * ncg
    planes = [(np.arange(n, dtype=np.int32).reshape(kpad, 32 * ncg) * 3 + p).astype(np.int16) for p in range(3)]
    buf = wc.pack_bf16x3(*planes, kpad, ncg)
    assert buf.shape == (3 * n,) and buf.dtype == np.int16
    for got, want in zip(wc.unpack_bf16x3(buf, kpad, ncg), planes):
        assert np.array_equal(got, want)
    assert np.array_equal(wc.pack_bf16x3(*wc.unpack_bf16x3(buf, kpad, ncg), kpad, ncg), buf)
    for p in range(3):
        for k in range(kpad):
            for j in range(32 * ncg):
                assert buf[_bf16_flat(k, j, p, kpad)] == planes[p][k, j], (p, k, j)


@pytest.mark.parametrize("group", wc.PACK_GROUPS, ids=lambda g: g.name)
def test_expected_images_write_exactly_the_blocks(group):
    """Odd K and J at nonzero offsets: the image unpacks to the blocks at [koff + k][joff + j] and to the sentinel elsewhere."""
    srcs, logical = wc.pack_sources(group, seed=11)
    for b, s, w in zip(group.blocks, srcs, logical):
        assert s.shape == (b.rows, b.ld) and b.ld > b.cols and np.isnan(s[:, b.cols:]).all() and w.shape == (b.K, b.J)
        assert b.koff + b.K <= group.ktot and b.joff + b.J <= 32 * group.ncg
    # fp32
    kpad = group.kpad(8)
    full = wc.unpack_fp32(wc.expected_fp32(group, logical), kpad, group.ncg)
    written = np.zeros(full.shape, bool)
    for b, w in zip(group.blocks, logical):
        sl = (slice(b.koff, b.koff + b.K), slice(b.joff, b.joff + b.J))
        assert not written[sl].any(), "the blocks of a group must be disjoint"
        written[sl] = True
        assert np.array_equal(full[sl], np.ascontiguousarray(w).view(np.int32))
    assert (full[~written] == wc.SENTINEL).all() and (~written).any()
    # bf16x3
    kpad = group.kpad(16)
    planes = wc.unpack_bf16x3(wc.expected_bf16x3(group, logical), kpad, group.ncg)
    written = np.zeros((kpad, 32 * group.ncg), bool)
    for b, w in zip(group.blocks, logical):
        sl = (slice(b.koff, b.koff + b.K), slice(b.joff, b.joff + b.J))
        written[sl] = True
        pieces = [torch.from_numpy(np.ascontiguousarray(p[sl])).view(torch.bfloat16).double() for p in planes]
        assert torch.equal(pieces[0] + pieces[1] + pieces[2], torch.from_numpy(np.ascontiguousarray(w)).double())
    for p in planes:
        assert p.shape == written.shape and (p[~written] == (wc.SENTINEL & 0xFFFF)).all()


def test_pack_groups_hold_the_offsets_the_models_never_use():
    blocks = [b for g in wc.PACK_GROUPS for b in g.blocks]
    assert any(b.koff % 16 and b.koff % 8 for b in blocks) and any(b.joff % 32 for b in blocks)
    assert any(b.joff // 32 != (b.joff + b.J - 1) // 32 and b.joff % 32 for b in blocks), "a block across a 32-column group"
    assert {b.transpose for b in blocks} == {0, 1}
    assert {(b.rows, b.cols) for b in blocks} >= {(13, 37), (37, 13)}
    for kgroup in (8, 16):      # the smaller descriptors of a launch take the idx >= total return
        elems = [wc.pack_block_elems(b, kgroup) for b in blocks]
        assert min(elems) < max(elems)


# ---- bf16 split
@pytest.mark.parametrize("scale", [1.0, 1e-3, 300.0])
def test_bf16_split_is_exact(scale):
    g = torch.Generator().manual_seed(3)
    v = (torch.randn(1 << 16, generator=g) * scale).float()
    h, m, l = wc.split_bf16x3(v)
    assert h.dtype == m.dtype == l.dtype == torch.bfloat16
    err = (h.double() + m.double() + l.double() - v.double()).abs().max().item()
    assert err == 0.0, err


# ---- reductions
@pytest.mark.parametrize("form", ["vector", "tall", "scalar"])
def test_reduce_cases_resolve_to_their_form(form):
    cases = wc.REDUCE_CASES[form]
    assert cases and len(cases) <= wc.REDUCE_MAX_DESC, "one batched launch per form"
    for c in cases:
        assert c.form == form and wc.reduce_form(c) == form, c
        assert c.stride > c.len >= 1 and c.n_slabs >= 1, c
    ns, lens = {"vector": (wc.VECTOR_N, wc.VECTOR_LEN), "tall": (wc.TALL_N, wc.TALL_LEN), "scalar": (wc.SCALAR_N, wc.SCALAR_LEN)}[form]
    cn, cl = collections.Counter(c.n_slabs for c in cases), collections.Counter(c.len for c in cases)
    assert all(cn[n] >= 2 for n in ns) and all(cl[l] >= 2 for l in lens), (cn, cl)


def test_reduce_cases_cover_boundaries_and_ways():
    every = [c for cs in wc.REDUCE_CASES.values() for c in cs]
    form = {(c.n_slabs, c.len): wc.reduce_form(c) for c in every if c.stride % 4 == 0 and not c.slab_off and not c.out_off}
    assert any(f == "vector" for (n, _), f in form.items() if n == 255) and any(f == "tall" for (n, _), f in form.items() if n == 256)
    assert form[(256, 8192)] == "tall" and form[(256, 8196)] == "vector"
    sc = wc.REDUCE_CASES["scalar"]
    assert any(c.stride % 2 == 1 and not c.slab_off and not c.out_off for c in sc)
    assert any(c.stride % 4 == 0 and c.slab_off == 1 and not c.out_off for c in sc)
    assert any(c.stride % 4 == 0 and not c.slab_off and c.out_off == 1 for c in sc)
    largest = max(c.n_slabs * c.stride for c in every)
    assert largest == 256 * 8200 and largest * 4 < 9 << 20


def test_reduce_mix_fills_the_table():
    mix = wc.REDUCE_MIX
    assert len(mix) == wc.REDUCE_MAX_DESC == 32
    forms = collections.Counter(wc.reduce_form(c) for c in mix if c.len)
    assert min(forms[f] for f in ("vector", "tall", "scalar")) >= 10
    assert sum(1 for c in mix if c.len == 0) == 1
    assert len({c.len for c in mix}) >= 8
    assert any(c.slab_off for c in mix) and any(c.out_off for c in mix) and any(c.stride % 2 for c in mix)


# ---- integer data stays exact
def test_integer_data_is_exact_in_fp32():
    for tA, tB in wc.GEMM_TRANS:
        for c in wc.gemm_cases(tA, tB):
            assert wc.gemm_max_int_sum(c) < wc.EXACT, c
    for cs in wc.REDUCE_CASES.values():
        for c in cs:
            assert wc.reduce_max_int_sum(c) < wc.EXACT, c
    c = wc.GemmCase(33, 34, 130, 4, 1, 1, 1, 1, 0)
    d = wc.gemm_operands(c, "int", 5)
    vals = np.concatenate([a[np.isfinite(a)] for a in d["A"] + d["B"] + [d["u"], d["v"], d["C_old"]]])
    assert np.array_equal(vals, np.round(vals)) and np.abs(vals).max() == wc.GEMM_INT_RANGE
    assert np.abs(wc.ref_gemm(d)).max() <= wc.gemm_max_int_sum(c)
    r = wc.ReduceCase(513, 35, 40, 0, 0, "tall")
    s = wc.reduce_operands(r, "int", 5)
    assert np.abs(s[:, :r.len]).max() == wc.REDUCE_INT_RANGE and np.isnan(s[:, r.len:]).all()
    assert np.abs(wc.ref_reduce(r, s)[0]).max() <= wc.reduce_max_int_sum(r)


# ---- GEMM cases and reference
def test_gemm_cases_cover_the_issue():
    for tA, tB in wc.GEMM_TRANS:
        cs = wc.gemm_cases(tA, tB)
        assert len(cs) == 80 and {(c.M, c.N, c.K, c.nbatch) for c in cs} == set(wc.GEMM_SHAPES)
        assert {(c.accumulate, c.uv, c.c_by_offset) for c in cs} == {(a, u, o) for a in (0, 1) for u in (0, 1) for o in (0, 1)}
        assert min(c.tiles for c in cs) == 1 and max(c.tiles for c in cs) == 6
        for c in cs:
            assert c.lda > (c.M if tA else c.K) and c.ldb > (c.K if tB else c.N) and c.ldc > c.N
    chunks = {(M, N, K, nb): nb * ((K + 127) // 128) for M, N, K, nb in wc.GEMM_SHAPES}
    assert chunks[(64, 96, 384, 1)] == 3 and chunks[(5, 70, 385, 1)] == 4 and chunks[(7, 9, 0, 1)] == 0 and chunks[(33, 34, 130, 4)] == 8


@pytest.mark.parametrize("tA,tB", wc.GEMM_TRANS)
def test_ref_gemm_is_the_plain_product(tA, tB):
    c = wc.GemmCase(5, 7, 9, 2, tA, tB, 1, 1, 0)
    d = wc.gemm_operands(c, "normal", 1)
    want = torch.zeros(5, 7, dtype=torch.float64)
    for a, b in zip(d["A"], d["B"]):
        assert a.shape == (c.a_rows, c.lda) and b.shape == (c.b_rows, c.ldb)
        ta, tb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        la = ta[:9, :5].t() if tA else ta[:5, :9]
        lb = tb[:7, :9].t() if tB else tb[:9, :7]
        assert torch.isfinite(la).all() and torch.isfinite(lb).all() and torch.isnan(ta).sum() == c.a_rows * 3
        want += la @ lb
    want += torch.outer(torch.from_numpy(d["u"]).double(), torch.from_numpy(d["v"]).double()) + torch.from_numpy(d["C_old"]).double()
    got = torch.from_numpy(wc.ref_gemm(d))
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-14, atol=1e-14)
    assert (wc.gemm_bound(d) > 0).all()
    plain = wc.gemm_operands(dataclasses.replace(c, accumulate=0, uv=0), "normal", 1)
    assert plain["u"] is None and plain["v"] is None and plain["C_old"] is None


# ---- ABI mirrors
def test_ctypes_sizes():
    pkg = load_pkg()
    assert C.sizeof(pkg._lib.SgemmDesc) == pkg.plans._SG_DTYPE.itemsize == 136
    assert C.sizeof(pkg._lib.PackDesc) == pkg.plans._DESC_DTYPE.itemsize == 48
    assert C.sizeof(pkg._lib.ReduceDesc) == 40
