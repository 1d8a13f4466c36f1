"""The case tables and plain references of the weight-space kernels (csrc/dss2_weightspace.hpp: the batched small GEMM, the
weight packing in its fp32 and bf16x3 layouts, the fixed-order slab reductions), shared by tests/test_weightspace_cases_cpu.py
(the references against themselves, the form every reduction case resolves to, exactness of the integer data; no GPU) and
tests/test_gpu_weightspace.py (the exports of the library, driven with hand-built tables, against these references).

Everything here is numpy / torch on the CPU and written from the layout text of include/dss2_hip.h:

    small GEMM   C[M,N] (+)= sum_b op(A_b)[M,K] op(B_b)[K,N] (+ u[i] v[j]); op = transpose when the flag is set, i.e. A is then
                 stored [K, M] and B is stored [N, K], row-major with leading dimensions lda / ldb / ldc
    fp32 pack    [ncg][kpad/8][64 lanes][4]: lane (half, c32) holds B[8 kg + 4 half + s][32 cg + c32], s = 0..3
    bf16x3 pack  [ncg][kpad/16][3 planes][64 lanes][8]: lane (half, c32) holds B[16 kg + 8 half + q][32 cg + c32], q = 0..7,
                 plane p the p-th piece of h = bf16(v), m = bf16(v - h), l = bf16((v - h) - m), round-to-nearest-even
    reductions   out[j] = sum_{s < n_slabs} slab[s * stride + j], j < len; 16-byte lanes when slab, out and stride allow them,
                 the "tall" form of those when n_slabs >= 256 and len <= 8192, scalar otherwise

A case carries its sizes only; ``gemm_operands`` / ``reduce_operands`` draw its data (integers, whose sums are exact in fp32
whatever the order, or N(0,1)) from a seed, with NaN in every gap between a logical extent and its leading dimension."""
import dataclasses
import itertools

import numpy as np
import torch

U24 = 2.0 ** -24            # unit roundoff of fp32
EXACT = 2 ** 24             # integers below this magnitude are exact in fp32
SENTINEL = 0x7FC57FC5       # int32 prefill of every output: a NaN as fp32 and as each of its bf16 halves


# ------------------------------------------------------------------------------------------
# small GEMM
# ------------------------------------------------------------------------------------------
# (M, N, K, nbatch): one element; one full chunk; one past every edge; exactly three chunks (the ring of three in flight);
# a fourth chunk that re-uses a ring slot; the bias column and the bias row; the rank-1 term alone; 2 and 4 operand pairs of two
# chunks each (up to 8 chunks, batch index decoded from the chunk number)
GEMM_SHAPES = [(1, 1, 1, 1), (32, 32, 128, 1), (33, 31, 129, 1), (64, 96, 384, 1), (5, 70, 385, 1), (40, 1, 50, 1), (1, 40, 50, 1),
               (7, 9, 0, 1), (33, 34, 130, 2), (33, 34, 130, 4)]
GEMM_TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
GEMM_INT_RANGE = 4          # integer data: every operand, u, v and C_old drawn from [-4, 4]
GEMM_LD_PAD = (3, 5, 2)     # lda / ldb / ldc exceed the logical extent by this much
GEMM_C_GUARD = 7            # sentinel floats in front of and behind every C


@dataclasses.dataclass(frozen=True)
class GemmCase:
    M: int
    N: int
    K: int
    nbatch: int
    tA: int
    tB: int
    accumulate: int
    uv: int                 # 1: with the rank-1 term
    c_by_offset: int        # 1: C = base_out + c_off; 0: C given as a pointer

    @property
    def lda(self):
        return (self.M if self.tA else self.K) + GEMM_LD_PAD[0]

    @property
    def ldb(self):
        return (self.K if self.tB else self.N) + GEMM_LD_PAD[1]

    @property
    def ldc(self):
        return self.N + GEMM_LD_PAD[2]

    @property
    def a_rows(self):
        return self.K if self.tA else self.M

    @property
    def b_rows(self):
        return self.N if self.tB else self.K

    @property
    def tiles(self):
        return ((self.M + 31) // 32) * ((self.N + 31) // 32)

    @property
    def name(self):
        return (f"{self.M}x{self.N}x{self.K}b{self.nbatch}-{'T' if self.tA else 'N'}{'T' if self.tB else 'N'}"
                f"-acc{self.accumulate}-uv{self.uv}-{'off' if self.c_by_offset else 'ptr'}")


def gemm_cases(tA, tB):
    """Every shape x accumulate x rank-1 term x (pointer / offset) for one pair of transposition flags: 80 descriptors."""
    return [GemmCase(M, N, K, nb, tA, tB, acc, uv, off)
            for (M, N, K, nb) in GEMM_SHAPES for acc in (0, 1) for uv in (0, 1) for off in (0, 1)]


def gemm_max_int_sum(c: GemmCase) -> int:
    """Largest |partial sum| an integer-data case can reach, whatever the order of summation."""
    r = GEMM_INT_RANGE
    return c.nbatch * c.K * r * r + (r * r if c.uv else 0) + (r if c.accumulate else 0)


def _draw(rng, shape, data):
    if data == "int":
        return rng.integers(-GEMM_INT_RANGE, GEMM_INT_RANGE + 1, size=shape).astype(np.float32)
    return rng.standard_normal(size=shape).astype(np.float32)


def gemm_operands(c: GemmCase, data: str, seed: int) -> dict:
    """The stored operands of a case: A[b] as [a_rows, lda] and B[b] as [b_rows, ldb] with NaN beyond the logical columns,
    u[M], v[N] (None without the rank-1 term) and C_old[M, N] (None unless the case accumulates)."""
    rng = np.random.default_rng(seed)
    A, B = [], []
    for _ in range(c.nbatch):
        a = np.full((c.a_rows, c.lda), np.nan, np.float32)
        a[:, :c.lda - GEMM_LD_PAD[0]] = _draw(rng, (c.a_rows, c.lda - GEMM_LD_PAD[0]), data)
        b = np.full((c.b_rows, c.ldb), np.nan, np.float32)
        b[:, :c.ldb - GEMM_LD_PAD[1]] = _draw(rng, (c.b_rows, c.ldb - GEMM_LD_PAD[1]), data)
        A.append(a)
        B.append(b)
    u = _draw(rng, (c.M,), data) if c.uv else None
    v = _draw(rng, (c.N,), data) if c.uv else None
    c_old = _draw(rng, (c.M, c.N), data) if c.accumulate else None
    return dict(case=c, A=A, B=B, u=u, v=v, C_old=c_old)


def _gemm_logical(desc):
    c = desc["case"]
    As = [(a[:c.K, :c.M].T if c.tA else a[:c.M, :c.K]).astype(np.float64) for a in desc["A"]]
    Bs = [(b[:c.N, :c.K].T if c.tB else b[:c.K, :c.N]).astype(np.float64) for b in desc["B"]]
    return c, As, Bs


def ref_gemm(desc) -> np.ndarray:
    """sum_b op(A_b) op(B_b) (+ u v^T) (+ C_old) in float64."""
    c, As, Bs = _gemm_logical(desc)
    out = np.zeros((c.M, c.N), np.float64)
    for a, b in zip(As, Bs):
        out += a @ b
    if desc["u"] is not None:
        out += np.outer(desc["u"].astype(np.float64), desc["v"].astype(np.float64))
    if desc["C_old"] is not None:
        out += desc["C_old"].astype(np.float64)
    return out


def gemm_bound(desc) -> np.ndarray:
    """Per component (nbatch K + 8) 2^-24 (sum_k |a||b| + |u_i v_j| + |C_old|): a chain of nbatch K + 8 fp32 roundings."""
    c, As, Bs = _gemm_logical(desc)
    mag = np.zeros((c.M, c.N), np.float64)
    for a, b in zip(As, Bs):
        mag += np.abs(a) @ np.abs(b)
    if desc["u"] is not None:
        mag += np.abs(np.outer(desc["u"].astype(np.float64), desc["v"].astype(np.float64)))
    if desc["C_old"] is not None:
        mag += np.abs(desc["C_old"].astype(np.float64))
    return (c.nbatch * c.K + 8) * U24 * mag


# ------------------------------------------------------------------------------------------
# weight packing
# ------------------------------------------------------------------------------------------
def unpack_fp32(buf, kpad, ncg):
    """B[kpad, 32 ncg] of a buffer [ncg][kpad/8][64 lanes][4] (any 4-byte dtype; the bits travel unchanged)."""
    a = np.asarray(buf).reshape(ncg, kpad // 8, 2, 32, 4)                  # [cg][kg][half][c32][s]
    return a.transpose(1, 2, 4, 0, 3).reshape(kpad, 32 * ncg)             # k = (kg, half, s), j = (cg, c32)


def pack_fp32(B, kpad, ncg):
    """The inverse of ``unpack_fp32``: the flat buffer of B[kpad, 32 ncg]."""
    a = np.asarray(B).reshape(kpad // 8, 2, 4, ncg, 32)                    # [kg][half][s][cg][c32]
    return np.ascontiguousarray(a.transpose(3, 0, 1, 4, 2)).reshape(-1)


def unpack_bf16x3(buf, kpad, ncg):
    """The three planes (h, m, l), each B[kpad, 32 ncg], of a buffer [ncg][kpad/16][3][64 lanes][8] of 2-byte elements."""
    a = np.asarray(buf).reshape(ncg, kpad // 16, 3, 2, 32, 8)              # [cg][kg][plane][half][c32][q]
    a = a.transpose(2, 1, 3, 5, 0, 4).reshape(3, kpad, 32 * ncg)          # plane, k = (kg, half, q), j = (cg, c32)
    return a[0], a[1], a[2]


def pack_bf16x3(h, m, l, kpad, ncg):
    """The inverse of ``unpack_bf16x3``."""
    a = np.stack([np.asarray(h), np.asarray(m), np.asarray(l)]).reshape(3, kpad // 16, 2, 8, ncg, 32)   # [plane][kg][half][q][cg][c32]
    return np.ascontiguousarray(a.transpose(4, 1, 0, 2, 5, 3)).reshape(-1)


def split_bf16x3(v: torch.Tensor):
    """(h, m, l) of fp32 values: h = bf16(v), m = bf16(v - h), l = bf16((v - h) - m), torch's CPU casts (round-to-nearest-even)."""
    v = v.to(torch.float32)
    h = v.to(torch.bfloat16)
    r1 = v - h.to(torch.float32)
    m = r1.to(torch.bfloat16)
    l = (r1 - m.to(torch.float32)).to(torch.bfloat16)
    return h, m, l


def bf16_bits(x: torch.Tensor) -> np.ndarray:
    return x.contiguous().view(torch.int16).numpy()


@dataclasses.dataclass(frozen=True)
class PackBlock:
    rows: int
    cols: int
    transpose: int          # bit 0 of the descriptor's field
    koff: int = 0
    joff: int = 0
    ld_pad: int = 3         # ld = cols + ld_pad, NaN in the gap

    @property
    def K(self):
        return self.cols if self.transpose else self.rows

    @property
    def J(self):
        return self.rows if self.transpose else self.cols

    @property
    def ld(self):
        return self.cols + self.ld_pad


@dataclasses.dataclass(frozen=True)
class PackGroup:
    """One packed matrix and the blocks that fill disjoint parts of it (one descriptor each)."""
    name: str
    ktot: int               # kpad = ktot rounded up to the layout's k group (8 / 16)
    ncg: int
    blocks: tuple

    def kpad(self, kgroup):
        return (self.ktot + kgroup - 1) // kgroup * kgroup


def _stack_k(tr):
    # K = 5, 13, 3 at koff 0, 5, 18: no offset is a multiple of 8 or 16, so neighbours share a k group
    mk = (lambda K, koff: PackBlock(37, K, 1, koff)) if tr else (lambda K, koff: PackBlock(K, 37, 0, koff))
    return (mk(5, 0), mk(13, 5), mk(3, 18))


PACK_GROUPS = [
    PackGroup("13x37", 13, 2, (PackBlock(13, 37, 0),)),
    PackGroup("13x37-T", 37, 2, (PackBlock(13, 37, 1),)),
    PackGroup("37x13", 37, 2, (PackBlock(37, 13, 0),)),
    PackGroup("37x13-T", 13, 2, (PackBlock(37, 13, 1),)),
    PackGroup("13x37-at-19-21", 32, 2, (PackBlock(13, 37, 0, 19, 21),)),
    PackGroup("stack-k", 21, 2, _stack_k(0)),
    PackGroup("stack-k-T", 21, 2, _stack_k(1)),
    PackGroup("side-j-2-2-2", 13, 1, (PackBlock(13, 2, 0, 0, 0), PackBlock(2, 13, 1, 0, 2), PackBlock(13, 2, 0, 0, 4))),
    PackGroup("side-j-30-37", 13, 3, (PackBlock(13, 30, 0, 0, 0), PackBlock(37, 13, 1, 0, 30))),
]


def pack_block_elems(b: PackBlock, kgroup: int) -> int:
    """(cg1 - cg0) * nkl * 64 of a block: the threads its descriptor needs (include/dss2_hip.h: max_elems is the largest)."""
    kg0, kg1 = b.koff // kgroup, (b.koff + b.K + kgroup - 1) // kgroup
    cg0, cg1 = b.joff // 32, (b.joff + b.J + 31) // 32
    return (cg1 - cg0) * (kg1 - kg0) * 64


def pack_sources(group: PackGroup, seed: int):
    """One fp32 source [rows, ld] per block (N(0,1) scaled by 1, 1e-3 or 300 per block, NaN in the gap) and the logical
    B[K, J] each one stands for."""
    rng = np.random.default_rng(seed)
    srcs, logical = [], []
    for i, b in enumerate(group.blocks):
        s = np.full((b.rows, b.ld), np.nan, np.float32)
        s[:, :b.cols] = (rng.standard_normal((b.rows, b.cols)) * (1.0, 1e-3, 300.0)[i % 3]).astype(np.float32)
        srcs.append(s)
        w = s[:, :b.cols]
        logical.append(w.T if b.transpose else w)
    return srcs, logical


def expected_fp32(group: PackGroup, logical) -> np.ndarray:
    """The int32 image of the group's buffer after packing into a sentinel-filled buffer."""
    kpad = group.kpad(8)
    full = np.full((kpad, 32 * group.ncg), SENTINEL, np.int32)
    for b, w in zip(group.blocks, logical):
        full[b.koff:b.koff + b.K, b.joff:b.joff + b.J] = np.ascontiguousarray(w).view(np.int32)
    return pack_fp32(full, kpad, group.ncg)


def expected_bf16x3(group: PackGroup, logical) -> np.ndarray:
    """The int16 image of the group's buffer after packing into a sentinel-filled buffer."""
    kpad = group.kpad(16)
    planes = [np.full((kpad, 32 * group.ncg), SENTINEL & 0xFFFF, np.int16) for _ in range(3)]
    for b, w in zip(group.blocks, logical):
        for p, piece in zip(planes, split_bf16x3(torch.from_numpy(np.ascontiguousarray(w)))):
            p[b.koff:b.koff + b.K, b.joff:b.joff + b.J] = bf16_bits(piece)
    return pack_bf16x3(*planes, kpad, group.ncg)


# ------------------------------------------------------------------------------------------
# slab reductions
# ------------------------------------------------------------------------------------------
REDUCE_INT_RANGE = 8
REDUCE_MAX_DESC = 32
REDUCE_OUT_GUARD = 5        # sentinel floats behind every out


@dataclasses.dataclass(frozen=True)
class ReduceCase:
    n_slabs: int
    len: int
    stride: int
    slab_off: int           # floats past a 16-byte boundary at which the slab / the output starts
    out_off: int
    form: str               # the form the case is meant to hit

    @property
    def name(self):
        return f"{self.form}-{self.n_slabs}x{self.len}-s{self.stride}-a{self.slab_off}{self.out_off}"


def reduce_form(d: ReduceCase) -> str:
    """The header's rule: 16-byte lanes need 16-byte aligned slabs and outputs and a stride divisible by 4; of those, many
    short slabs (n_slabs >= 256 and len <= 8192) take the tall form."""
    if d.stride % 4 != 0 or (4 * d.slab_off) % 16 != 0 or (4 * d.out_off) % 16 != 0:
        return "scalar"
    return "tall" if d.n_slabs >= 256 and d.len <= 8192 else "vector"


def _aligned_stride(length):
    return (length + 3) // 4 * 4 + 4             # > len, divisible by 4


def _odd_stride(length):
    return length + 1 if length % 2 == 0 else length + 2


def _pairs(ns, lens, second):
    """n_slabs[i] with lens[i mod] and lens[second(i) mod]: every value of either list at least twice."""
    return [(n, lens[j % len(lens)]) for i, n in enumerate(ns) for j in (i, second(i))]


VECTOR_N = [1, 15, 16, 17, 48, 49, 64, 65, 113, 255]
VECTOR_LEN = [1, 3, 4, 63, 64, 65, 67, 130]
TALL_N = [256, 257, 319, 320, 511, 513]
TALL_LEN = [1, 15, 16, 17, 18, 35]
SCALAR_N = [1, 3, 4, 5, 31, 32, 33, 37]
SCALAR_LEN = [1, 63, 64, 65, 130]
SCALAR_WAYS = ["odd-stride", "slab+1", "out+1"]


def _scalar_case(n, length, way):
    if way == "odd-stride":
        return ReduceCase(n, length, _odd_stride(length), 0, 0, "scalar")
    if way == "slab+1":
        return ReduceCase(n, length, _aligned_stride(length), 1, 0, "scalar")
    return ReduceCase(n, length, _aligned_stride(length), 0, 1, "scalar")


REDUCE_CASES = {
    "vector": [ReduceCase(n, l, _aligned_stride(l), 0, 0, "vector") for n, l in _pairs(VECTOR_N, VECTOR_LEN, lambda i: 3 * i + 1)]
              + [ReduceCase(256, 8196, _aligned_stride(8196), 0, 0, "vector")],
    "tall": [ReduceCase(n, l, _aligned_stride(l), 0, 0, "tall") for n, l in _pairs(TALL_N, TALL_LEN, lambda i: i + 3)]
            + [ReduceCase(256, 8192, _aligned_stride(8192), 0, 0, "tall")],
    "scalar": [_scalar_case(n, l, SCALAR_WAYS[k % 3])
               for k, (n, l) in enumerate(_pairs(SCALAR_N, SCALAR_LEN, lambda i: 2 * i + 1))],
}

# the 32 descriptors of the mixed launch: the three forms with different lengths (the two 8 MB slabs stay out), one with len = 0
REDUCE_MIX = list(itertools.chain.from_iterable(zip(REDUCE_CASES["vector"][:11], REDUCE_CASES["tall"][:11], REDUCE_CASES["scalar"][:11])))[:31] \
    + [ReduceCase(4, 0, 4, 0, 0, "vector")]


def reduce_max_int_sum(c: ReduceCase) -> int:
    return c.n_slabs * REDUCE_INT_RANGE


def reduce_operands(c: ReduceCase, data: str, seed: int) -> np.ndarray:
    """slab[n_slabs, stride] with NaN from column len on."""
    rng = np.random.default_rng(seed)
    s = np.full((c.n_slabs, c.stride), np.nan, np.float32)
    if data == "int":
        s[:, :c.len] = rng.integers(-REDUCE_INT_RANGE, REDUCE_INT_RANGE + 1, size=(c.n_slabs, c.len)).astype(np.float32)
    else:
        s[:, :c.len] = rng.standard_normal((c.n_slabs, c.len)).astype(np.float32)
    return s


def ref_reduce(c: ReduceCase, slab: np.ndarray):
    """(fp64 column sums, n_slabs 2^-24 sum_s |slab[s][j]|)."""
    x = slab[:, :c.len].astype(np.float64)
    return x.sum(0), c.n_slabs * U24 * np.abs(x).sum(0)
