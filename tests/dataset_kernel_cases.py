"""The case tables and plain references of the dataset kernels (csrc/dss2_dataset.hip: the measurement model, the masked z-score,
the four collation entry points with the device cursor, ``dss2_accum_scalar``), shared by tests/test_dataset_kernel_cases_cpu.py
(the properties of the case data that the GPU tests rely on; no GPU) and tests/test_gpu_dataset_kernels.py (the exports of the
library, driven through ctypes with hand-built tables, against these references).

Everything here is numpy / torch on the CPU.  The referee of the measurement model and of the normalised z-scores is
oracle/dss2_dataset_oracle.py (the reference's own numpy-float64 / torch-float32 arithmetic); the referee of the z-score's
statistics is numpy float64; the referee of every collation is numpy indexing of the same tables.

    measurement model   rows of [n_per_sample]-bus samples; the mask byte of row r is mask[r % n_per_sample]
    masked z-score      t [rows][ld] fp32, the first num_feat columns normalised over their non-zero entries, the rest copied
    collation           kind 0 float chunks, kind 2 int32 chunks, kind 1 int64 edge lists [S][2][e] (or one shared [2][e]) that get
                        the slot's node offset added; the ragged forms write every item at its own node / edge row

A case carries its sizes and a seed; its data is drawn on demand and cached."""
import dataclasses
import functools

import numpy as np
import torch

import dss2_dataset_oracle as dso

U24 = 2.0 ** -24            # unit roundoff of fp32
SENTINEL = 0x7FC57FC5       # int32 prefill of every output: a NaN as fp32, and as either half of a double or an int64 far out of range
NAN_BITS = 0x7FC00000       # int32 fill of every gap between operands: NaN as fp32 and (in pairs) as a double
FLT_MAX = float(np.finfo(np.float32).max)

# the project's default noise model (synthetic.NOISE; the CPU test holds the two together) and the two variants of the issue
NOISE_DEFAULT = dict(p_noise=0.02, v_noise=0.01, pm_noise=0.15, zero_inj_coef=0.001)
NOISE_ZERO = dict(p_noise=0.0, v_noise=0.0, pm_noise=0.0, zero_inj_coef=0.0)
NOISE_NO_ZINJ = dict(NOISE_DEFAULT, zero_inj_coef=0.0)
NOISES = {"default": NOISE_DEFAULT, "zero": NOISE_ZERO, "no_zinj": NOISE_NO_ZINJ}

NODE_FLOOR, NODE_CAP = np.float32(1e-6), np.float32(1e12)
EDGE_FLOOR, EDGE_CAP = np.float32(1e-5), np.float32(1e10)


def around(floor):
    """The floor, its two fp32 neighbours below and its five above, ascending."""
    out, v = [], np.float32(floor)
    lo = v
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(0))
        out.append(lo)
    out = out[::-1] + [v]
    for _ in range(5):
        v = np.nextafter(v, np.float32(1))
        out.append(v)
    return np.array(out, np.float32)


def same_bits_or_both_nan(a, b):
    """fp32 arrays: NaN in the same cells, equal bits in every other cell (the sign of zero included)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


# ------------------------------------------------------------------------------------------
# measurement model
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MeasureCase:
    name: str
    per: int                # buses (branches) per sample
    rows: int               # total rows, not necessarily whole samples
    mask: str               # "none" | "all" | "last": which buses (branches) are measured
    noise: str              # key of NOISES
    draws: str              # "normal" | "zero" | "six"
    values: str = "random"  # "random" | "floor" | "nonfinite"
    zinj: bool = True       # False: no zero-injection bus at all

    def mask_bytes(self):
        m = np.zeros(self.per, np.uint8)
        if self.mask == "all":
            m[:] = 1
        elif self.mask == "last":
            m[-1] = 1
        return m


MEASURE_CASES = [
    MeasureCase("one_row", 1, 1, "all", "default", "normal"),
    MeasureCase("n7_255_unmeasured_noiseless", 7, 255, "none", "zero", "zero"),
    MeasureCase("n15_256_last_nozinjcoef", 15, 256, "last", "no_zinj", "normal"),
    MeasureCase("n15_257_all_six", 15, 257, "all", "default", "six"),
    MeasureCase("n179_537_last", 179, 3 * 179, "last", "default", "normal", zinj=False),
    MeasureCase("n7_257_none_default", 7, 257, "none", "default", "six"),
    MeasureCase("n15_255_all_noiseless", 15, 255, "all", "zero", "normal"),
    MeasureCase("floor", 8, 64, "all", "default", "normal", values="floor"),
    MeasureCase("floor_draws_zero", 8, 64, "all", "default", "zero", values="floor"),
    MeasureCase("nonfinite", 7, 70, "all", "default", "normal", values="nonfinite"),
    MeasureCase("nonfinite_unmeasured", 7, 70, "none", "default", "zero", values="nonfinite"),
]


def _draws(c, rng, cols):
    if c.draws == "zero":
        return np.zeros((c.rows, cols))
    if c.draws == "six":      # |z| = 6, both signs, against the negative means that _node_table / _edge_table give these cases
        return np.where(rng.random((c.rows, cols)) < 0.5, -6.0, 6.0)
    return rng.standard_normal((c.rows, cols))


@functools.lru_cache(maxsize=None)
def node_tables(c: MeasureCase):
    """(nodes [rows, 7] float64, z [rows, 4] float64) of a case.  Slack at bus (sample + 1) % per (so mostly not at bus 0), a second
    slack bus in every third sample, the slack bus also a zero-injection bus in even samples, one bus in five zero-injection;
    p = q = 0 at every fifth row; p and q of both signs (all negative for the |z| = 6 draws)."""
    rng = np.random.default_rng(1000 + MEASURE_CASES.index(c))
    R, n = c.rows, c.per
    r = np.arange(R)
    s, b = r // n, r % n
    t = np.zeros((R, 7))
    t[:, 0] = 1.0 + 0.05 * rng.standard_normal(R)
    t[:, 1] = 0.3 * rng.standard_normal(R)
    t[:, 2:4] = 3.0 * rng.standard_normal((R, 2))
    if c.draws == "six":
        t[:, 1:4] = -np.abs(t[:, 1:4])
    t[r % 5 == 2, 2:4] = 0.0
    t[:, 4] = np.where(b == 0, 110.0, 20.0)
    slack = (b == (s + 1) % n) | ((s % 3 == 2) & (b == (s + 4) % n))
    t[:, 5] = slack
    zi = (rng.random(R) < 0.2) | (slack & (s % 2 == 0))
    t[:, 6] = zi if c.zinj else 0.0
    if c.values == "floor":
        # column V at a measured non-slack bus: |std| = |V v_noise| -> the eight fp32 values around the floor, and column P likewise
        # (|P pm_noise|, no zero-injection term) -- raw = target / coefficient in double, which the double product and the one
        # rounding to fp32 bring back to the target (the CPU test checks it)
        tg = around(NODE_FLOOR).astype(np.float64)
        k = np.arange(R) % 8
        t[:, 5:7] = 0.0
        t[:, 0] = tg[k] / NOISE_DEFAULT["v_noise"] * np.where(r % 16 < 8, 1.0, -1.0)
        t[:, 2] = tg[(k + 3) % 8] / NOISE_DEFAULT["pm_noise"]
    if c.values == "nonfinite":
        t[3, 0], t[10, 0], t[17, 0] = np.nan, np.inf, -np.inf
        t[24, 2], t[31, 2], t[38, 2] = np.nan, np.inf, -np.inf
        t[45, 1], t[52, 3] = np.nan, np.inf
    return t, _draws(c, rng, 4)


@functools.lru_cache(maxsize=None)
def edge_tables(c: MeasureCase):
    """(edges [rows, 11] float64, z [rows, 2] float64) of a case, read with ``per`` as the branches per sample."""
    rng = np.random.default_rng(2000 + MEASURE_CASES.index(c))
    R = c.rows
    r = np.arange(R)
    t = rng.standard_normal((R, 11)) * np.array([0, 0, 4.0, 2.0, 30.0, 90.0, 1e-3, 1e-3, 0, 0.1, 0.4])
    t[:, 0], t[:, 1], t[:, 8] = r % c.per, (r + 1) % c.per, 1.0
    if c.draws == "six":
        t[:, 2:4] = -np.abs(t[:, 2:4])
    t[r % 5 == 2, 2:4] = 0.0
    if c.values == "floor":
        tg = around(EDGE_FLOOR).astype(np.float64)
        k = np.arange(R) % 8
        t[:, 2] = tg[k] / NOISE_DEFAULT["p_noise"] * np.where(r % 16 < 8, 1.0, -1.0)
        t[:, 3] = tg[(k + 3) % 8] / NOISE_DEFAULT["p_noise"]
    if c.values == "nonfinite":
        t[3, 2], t[10, 2], t[17, 2] = np.nan, np.inf, -np.inf
        t[24, 3], t[31, 3] = np.nan, np.inf
        t[40, 4] = np.inf                          # a copied parameter column
    return t, _draws(c, rng, 2)


def _samples(c):
    for lo in range(0, c.rows, c.per):
        hi = min(lo + c.per, c.rows)
        yield lo, hi, [j for j in np.flatnonzero(c.mask_bytes()) if j < hi - lo]


@functools.lru_cache(maxsize=None)
def ref_nodes(c: MeasureCase):
    """x [rows, 11] fp32 of the oracle, sample by sample (the last sample may be cut short)."""
    t, z = node_tables(c)
    out = np.empty((c.rows, 11), np.float32)
    with np.errstate(all="ignore"):
        for lo, hi, meas in _samples(c):
            out[lo:hi, :8] = dso.measure_nodes(t[lo:hi, 0:4], t[lo:hi, 5], t[lo:hi, 6], meas, NOISES[c.noise], z[lo:hi]).numpy()
        out[:, 8:] = t[:, 4:7].astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def ref_edges(c: MeasureCase):
    t, z = edge_tables(c)
    out = np.empty((c.rows, 13), np.float32)
    with np.errstate(all="ignore"):
        for lo, hi, meas in _samples(c):
            out[lo:hi, :6] = dso.measure_edges(t[lo:hi, 2:4], t[lo:hi, 4:6], meas, NOISES[c.noise], z[lo:hi]).numpy()
        out[:, 6:] = t[:, 4:11].astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------
# masked z-score
# ------------------------------------------------------------------------------------------
ZS_ROWS = [1, 2, 63, 64, 65, 255, 256, 257, 65_280, 65_281, 65_536, 65_537, 66_305]
ZS_NUM_FEAT = [1, 6, 8, 16]
ZS_LAYOUTS = ["in_place", "same_ld", "wider"]     # out == t | out != t, ld_out == ld | out != t, ld_out = ld + 3
ZS_MEAN_BOUND, ZS_STD_BOUND = 3 * U24, 8 * U24     # relative, against numpy float64 (derivation: tests/test_gpu_dataset_kernels.py)
ZS_MAX_RATIO = 100.0                                # |mean| / std of every column that the std bound is applied to
# column kinds.  "random*": the bounds against float64 apply; the others have exact expectations
ZS_KINDS = ["random", "allzero", "random_shifted", "single", "random_dense", "negzero", "subnormal", "nan", "inf", "inf_dense"]
ZS_BOUNDED = ("random", "random_shifted", "random_dense")
ZS_ORACLE_STATS = ("nan", "inf", "inf_dense")       # statistics are 0 / +-FLT_MAX by the oracle's nan_to_num: compared exactly


@dataclasses.dataclass(frozen=True)
class ZscoreCase:
    rows: int
    num_feat: int
    ld: int
    layout: str
    kinds: tuple            # one per feature column

    @property
    def ld_out(self):
        return self.ld + 3 if self.layout == "wider" else self.ld

    @property
    def name(self):
        return f"{self.rows}x{self.ld}_f{self.num_feat}_{self.layout}"


def _zs_cases():
    cases = []
    for i, rows in enumerate(ZS_ROWS):
        nf = ZS_NUM_FEAT[(i + 3) % 4] if rows != 66_305 else 16
        ld = nf if (i % 2 == 0 or nf == 16) else nf + 5           # num_feat == ld: no passthrough column
        kinds = tuple(ZS_KINDS[(i + j) % len(ZS_KINDS)] for j in range(nf))
        cases.append(ZscoreCase(rows, nf, ld, ZS_LAYOUTS[i % 3], kinds))
    # every kind at a small, odd shape in every layout, and the same past one block
    for rows, layout in ((67, "in_place"), (67, "same_ld"), (67, "wider"), (300, "wider")):
        cases.append(ZscoreCase(rows, len(ZS_KINDS), len(ZS_KINDS) + 3, layout, tuple(ZS_KINDS)))
    return cases


ZSCORE_CASES = _zs_cases()
# the table of the refusal test: ld below the 16-column limit, so that ld < num_feat <= 16 is a case of its own (not the case "17")
ZS_REFUSAL_CASE, ZS_REFUSAL_NUM_FEAT = ZSCORE_CASES[2], 4


def _zs_column(kind, rows, rng):
    r = np.arange(rows)
    if kind.startswith("random"):
        mu, sd = {"random": (0.3, 1.0), "random_shifted": (-40.0, 1.0), "random_dense": (2.0, 0.5)}[kind]
        col = (mu + sd * rng.standard_normal(rows)).astype(np.float32)
        if rows <= 2:          # two entries at a fixed distance: a draw could bring them arbitrarily close (|mean| / std unbounded)
            col = np.array([mu + sd, mu - 0.5 * sd][:rows], np.float32)
        elif kind != "random_dense":
            col[rng.random(rows) < 0.3] = 0.0
            col[rng.random(rows) < 0.05] = -0.0
        return col
    col = np.zeros(rows, np.float32)
    if kind == "allzero":
        col[r % 3 == 1] = -0.0
    elif kind == "single":
        col[rows // 2] = -2.75
    elif kind == "negzero":          # -0.0 is "not measured": two measured values among zeros of both signs
        col[:] = -0.0
        col[r % 4 == 0] = 0.0
        col[0] = 1.5
        col[rows - 1] = 0.5 if rows > 1 else 1.5
    elif kind == "subnormal":
        col[:] = np.where(r % 2 == 0, np.float32(1e-38), np.float32(2e-38))
        if rows > 8:
            col[r % 7 == 3] = 0.0
            col[5] = -np.float32(2e-38)
    elif kind == "nan":
        col[:] = (1.0 + 0.25 * rng.standard_normal(rows)).astype(np.float32)
        col[r % 4 == 1] = 0.0
        col[rows // 3] = np.nan
    elif kind == "inf":              # with unmeasured entries: the oracle's (0 - FLT_MAX)^2 * 0 = nan makes its std 0
        col[:] = (1.0 + 0.25 * rng.standard_normal(rows)).astype(np.float32)
        col[r % 4 == 1] = 0.0
        col[rows // 3] = np.inf
    elif kind == "inf_dense":        # every entry measured: std = FLT_MAX
        col[:] = (1.0 + 0.25 * rng.standard_normal(rows)).astype(np.float32)
        col[col == 0] = 1.0
        col[rows // 3] = -np.inf
    return col


@functools.lru_cache(maxsize=None)
def zscore_table(c: ZscoreCase):
    """t [rows, ld] fp32: the feature columns by kind, the passthrough columns random with zeros of both signs and a NaN."""
    rng = np.random.default_rng(3000 + ZSCORE_CASES.index(c))
    t = rng.standard_normal((c.rows, c.ld)).astype(np.float32)
    for j, k in enumerate(c.kinds):
        t[:, j] = _zs_column(k, c.rows, rng)
    if c.ld > c.num_feat:
        t[::3, c.num_feat] = 0.0
        t[1::5, c.ld - 1] = -0.0
        t[c.rows // 2, c.num_feat] = np.nan
    return t


def stats64(t, num_feat):
    """(count, mean, std) of the non-zero entries of each of the first num_feat columns, numpy float64 (0 where the count is 0)."""
    a = t[:, :num_feat].astype(np.float64)
    m = a != 0
    n = m.sum(0)
    with np.errstate(all="ignore"):
        mean = np.where(n > 0, np.where(m, a, 0).sum(0) / np.maximum(n, 1), 0.0)
        std = np.where(n > 0, np.sqrt((np.where(m, a - mean, 0) ** 2).sum(0) / np.maximum(n, 1)), 0.0)
    return n, mean, std


def stats32(t, num_feat):
    """An fp32 restatement of the reference's statistics (data.py:179-183) with the roundings that the bounds count: every element
    operation in fp32, each column sum rounded to fp32 ONCE (accumulated in float64, as a correctly rounded sum), the quotient and the
    root in fp32.  (A running fp32 sum of 66 305 terms adds an error that grows with the row count and says nothing about a kernel.)"""
    a = t[:, :num_feat]
    m = (a != 0).astype(np.float32)
    with np.errstate(all="ignore"):
        n = m.sum(0, dtype=np.float64).astype(np.float32)
        mean = np.nan_to_num((a * m).sum(0, dtype=np.float64).astype(np.float32) / n)
        std = np.nan_to_num(np.sqrt((((a - mean) ** 2) * m).sum(0, dtype=np.float64).astype(np.float32) / n))
    return mean.astype(np.float32), std.astype(np.float32)


def ref_normalised(t, num_feat, mean, std):
    """The oracle's normalised table given these statistics of the feature columns (fp32 arrays)."""
    with np.errstate(all="ignore"):
        out, _, _ = dso.masked_zscore(torch.from_numpy(np.ascontiguousarray(t)), num_feat,
                                      stats=(torch.from_numpy(np.ascontiguousarray(mean)), torch.from_numpy(np.ascontiguousarray(std))))
    return out.numpy()


def oracle_stats(t, num_feat):
    with np.errstate(all="ignore"):
        _, mean, std = dso.masked_zscore(torch.from_numpy(np.ascontiguousarray(t)), num_feat)
    return mean[:num_feat].numpy(), std[:num_feat].numpy()


# ---- constant columns (the mean must be rounded once)
CONST_COUNTS = list(range(1, 34)) + [960]
CONST_ROWS = 1000
CONST_GIVEN = {3: 1.4595472812652588, 960: 1.8317632675170898}      # the values of the issue


def mean_two_roundings(n, v):
    """fl(fl(n v) / n): the sum n v is exact in double; rounding it to fp32 BEFORE the division is the defect."""
    return (np.float64(n) * np.asarray(v, np.float64)).astype(np.float32) / np.float32(n)


def mean_one_rounding(n, v):
    return ((np.float64(n) * np.asarray(v, np.float64)) / np.float64(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def const_values():
    """{count: fp32 value}: the issue's two values, and for every other count the first of 20 000 seeded fp32 numbers in (0.01, 2.01)
    that the two-rounding mean gets wrong (none exists for a power of two: any value then)."""
    cand = (0.01 + 2.0 * np.random.default_rng(7).random(20_000)).astype(np.float32)
    out = {}
    for n in CONST_COUNTS:
        if n in CONST_GIVEN:
            out[n] = np.float32(CONST_GIVEN[n])
            continue
        bad = np.flatnonzero(mean_two_roundings(n, cand) != cand)
        out[n] = cand[bad[0]] if bad.size else cand[n]
    return out


CONST_GROUPS = [CONST_COUNTS[0:16], CONST_COUNTS[16:32], CONST_COUNTS[32:] + [3, 7, 11, 960]]      # <= 16 columns per launch


@functools.lru_cache(maxsize=None)
def const_table(g: int):
    """t [CONST_ROWS, ld]: column j holds its value at CONST_GROUPS[g][j] seeded rows, negated nowhere, zeros of both signs elsewhere."""
    rng = np.random.default_rng(4000 + g)
    counts = CONST_GROUPS[g]
    t = np.zeros((CONST_ROWS, len(counts) + 1), np.float32)
    t[1::2] = -0.0
    for j, n in enumerate(counts):
        t[rng.permutation(CONST_ROWS)[:n], j] = const_values()[n]
    t[:, -1] = rng.standard_normal(CONST_ROWS)
    return t


# ------------------------------------------------------------------------------------------
# collation
# ------------------------------------------------------------------------------------------
COLLATE_S = 19                      # samples in the store
COLLATE_NPS = 1000                  # nodes per sample of the edge-list descriptors
COLLATE_BATCHES = [1, 3, 17]
COLLATE_IDS = ["null", "reversed", "repeats"]
# (kind, shared, chunk) of the four descriptors of one launch: chunks 1 / 255 / 257 / 11 * 179 under each kind once
COLLATE_LAYOUTS = {
    "A": [(0, 0, 11 * 179), (2, 0, 1), (1, 1, 255), (1, 0, 257)],
    "B": [(0, 0, 255), (2, 0, 257), (1, 1, 11 * 179), (1, 0, 1)],
}


def collate_ids(how, B):
    if how == "null":
        return None
    if how == "reversed":
        return (COLLATE_S - 1 - np.arange(B)).astype(np.int64)
    return ((np.arange(B) * 7) % 5 + 3).astype(np.int64)


def collate_source(kind, shared, chunk, S=COLLATE_S, base=0):
    """A store whose every cell holds its own flat index (+ base): float [S, chunk], int32 [S, chunk], int64 [S, 2, e] or [2, e]."""
    if kind == 0:
        a = np.arange(S * chunk, dtype=np.float32) + np.float32(base)
        assert a[-1] < 2 ** 24
        return a.reshape(S, chunk)
    if kind == 2:
        return (np.arange(S * chunk, dtype=np.int32) + base).reshape(S, chunk)
    if shared:
        return (np.arange(2 * chunk, dtype=np.int64) + base).reshape(2, chunk)
    return (np.arange(S * 2 * chunk, dtype=np.int64) + base).reshape(S, 2, chunk)


def ref_collate(kind, shared, src, ids, B, nps):
    """dst of one descriptor by numpy indexing: [B, chunk], or [2, B * e] int64."""
    s = np.arange(B) if ids is None else np.asarray(ids)
    if kind != 1:
        return src[s]
    per = np.broadcast_to(src, (B,) + src.shape) if shared else src[s]          # [B, 2, e]
    off = (np.arange(B, dtype=np.int64) * np.int64(nps)).reshape(B, 1, 1)
    return np.ascontiguousarray((per + off).transpose(1, 0, 2)).reshape(2, -1)


# cursor: (epoch length as stored in cursor[1], batch, start position); the ids array has CURSOR_IDS entries
CURSOR_IDS = 64
CURSOR_CASES = [(50, 16, 0), (50, 16, 40), (50, 16, 49), (16, 16, 5), (0, 16, 7), (-3, 16, 7), (5, 16, 0), (5, 16, 3)]


def cursor_reads(length, batch, pos):
    p = pos + np.arange(batch)
    return p % length if length > 0 else p


def cursor_next(length, batch, pos):
    return (pos + batch) % length if length > 0 else pos + batch


# ragged: (buses, branches, shared edge list, samples in the store) of the five cases
RAGGED_CASES = [(1, 1, 0, 4), (2, 1, 1, 5), (15, 14, 1, 6), (15, 15, 0, 7), (70, 69, 0, 3)]
# mixes of up to four of them: (case numbers, items of each in the batch); a case with 0 items passes null tables
RAGGED_MIXES = [((2,), (4,)), ((0, 3), (2, 3)), ((1, 2, 4), (3, 2, 1)), ((0, 2, 3, 4), (3, 0, 5, 1)), ((4, 1, 0, 3), (2, 2, 2, 2))]
RAGGED_E_PAD = 3                    # e_total = the batch's edges + this: the row stride of the edge list is its own argument


@functools.lru_cache(maxsize=None)
def ragged_store(k: int):
    """x [S, n, 11], y [S, n, 2], edge_attr [S, e, 13] fp32 and edge lists of case k; every cell its flat index, offset per operand."""
    n, e, shared, S = RAGGED_CASES[k]
    base = 100_000 * k
    x = (np.arange(S * n * 11, dtype=np.float32) + base).reshape(S, n, 11)
    y = (np.arange(S * n * 2, dtype=np.float32) + base + 20_000).reshape(S, n, 2)
    ea = (np.arange(S * e * 13, dtype=np.float32) + base + 40_000).reshape(S, e, 13)
    ei = collate_source(1, shared, e, S, base=7 * k)
    assert max(x.max(), y.max(), ea.max()) < 2 ** 24
    return dict(n=n, e=e, shared=shared, S=S, x=x, y=y, ea=ea, ei=ei)


@functools.lru_cache(maxsize=None)
def ragged_mix(m: int):
    """The batch of mix m: slots of the cases interleaved by a seeded permutation.  Returns dict(slots = [(case, sample)], per-case
    tables samp / node_off / edge_off (int64), totals N and E, and the expected x / y / edge_attr / edge_index [2, E])."""
    cases, counts = RAGGED_MIXES[m]
    rng = np.random.default_rng(5000 + m)
    owner = rng.permutation(np.repeat(np.arange(len(cases)), counts))
    slots = [(cases[o], int(rng.integers(RAGGED_CASES[cases[o]][3]))) for o in owner]
    n_slot = np.array([RAGGED_CASES[k][0] for k, _ in slots], np.int64)
    e_slot = np.array([RAGGED_CASES[k][1] for k, _ in slots], np.int64)
    node_off = np.concatenate([[0], np.cumsum(n_slot)]).astype(np.int64)
    edge_off = np.concatenate([[0], np.cumsum(e_slot)]).astype(np.int64)
    tables = []
    for j, k in enumerate(cases):
        sl = np.flatnonzero(owner == j)
        tables.append(dict(samp=np.array([slots[i][1] for i in sl], np.int64), node_off=node_off[sl], edge_off=edge_off[sl]))
    xs, ys, eas, eis = [], [], [], []
    for i, (k, s) in enumerate(slots):
        st = ragged_store(k)
        xs.append(st["x"][s]); ys.append(st["y"][s]); eas.append(st["ea"][s])
        eis.append((st["ei"] if st["shared"] else st["ei"][s]) + node_off[i])
    return dict(cases=cases, counts=counts, slots=slots, tables=tables, N=int(node_off[-1]), E=int(edge_off[-1]),
                x=np.concatenate(xs), y=np.concatenate(ys), ea=np.concatenate(eas), ei=np.concatenate(eis, axis=1))


# ------------------------------------------------------------------------------------------
# data_from_tables at S = 3, n = 5, e = 4
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_tables():
    rng = np.random.default_rng(6000)
    S, n, e = 3, 5, 4
    nodes = np.zeros((S, n, 7))
    nodes[..., 0] = 1.0 + 0.03 * rng.standard_normal((S, n))
    nodes[..., 1] = 0.2 * rng.standard_normal((S, n))
    nodes[..., 2:4] = 2.0 * rng.standard_normal((S, n, 2))
    nodes[:, 3, 2:4] = 0.0
    nodes[..., 4] = 20.0
    nodes[:, 1, 5] = 1.0                  # slack at bus 1
    nodes[:, 3, 6] = 1.0
    edges = rng.standard_normal((S, e, 11)) * np.array([0, 0, 3.0, 1.0, 20.0, 60.0, 1e-3, 1e-3, 0, 0.1, 0.4])
    edges[..., 0], edges[..., 1], edges[..., 8] = np.arange(e), np.arange(e) + 1, 1.0
    labels = np.stack([nodes[..., 0], nodes[..., 1]], axis=-1)
    return dict(nodes=nodes, edges=edges, labels=labels, noise=NOISE_DEFAULT, meas_v=[1, 4], meas_pflow=[0, 2],
                z_nodes=rng.standard_normal((S, n, 4)), z_edges=rng.standard_normal((S, e, 2)))
