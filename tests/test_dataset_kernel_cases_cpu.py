"""CPU: the case data of tests/dataset_kernel_cases.py has the properties that tests/test_gpu_dataset_kernels.py relies on -- the
measurement tables reach the floor and the cap of the inverse variances from both sides, the non-finite tables give the oracle's NaN
weights, the z-score's bounded columns keep |mean| / std <= 100 and an fp32 restatement of the reference stays inside the derived
bounds, the constant columns are values that a twice-rounded mean gets wrong and a once-rounded mean gets right, and the collation
references agree with the oracle's collate.  No GPU."""
import numpy as np
import pytest
import torch

import dataset_kernel_cases as dc
import dss2_dataset_oracle as dso


def test_default_noise_is_the_projects(pkg):
    assert {k: pkg.synthetic.NOISE[k] for k in dc.NOISE_DEFAULT} == dc.NOISE_DEFAULT
    assert set(dc.NOISE_DEFAULT) == set(pkg.dataset.NOISE_KEYS)


def test_measure_cases_cover_the_issue():
    cs = dc.MEASURE_CASES
    assert {c.per for c in cs} >= {1, 7, 15, 179} and {c.rows for c in cs} >= {1, 255, 256, 257, 3 * 179}
    assert {c.mask for c in cs} == {"none", "all", "last"} and {c.noise for c in cs} == {"default", "zero", "no_zinj"}
    assert {c.draws for c in cs} == {"normal", "zero", "six"} and any(not c.zinj for c in cs)
    for c in cs:
        t, z = dc.node_tables(c)
        s, b = np.arange(c.rows) // c.per, np.arange(c.rows) % c.per
        if c.values == "random" and c.per > 1 and c.rows > 3 * c.per:
            assert (t[b != 0, 5] == 1).any(), "slack at a bus other than 0"
            assert max(t[s == k, 5].sum() for k in range(3)) == 2, "two slack buses in a sample"
            assert ((t[:, 5] == 1) & (t[:, 6] == 1)).any() == c.zinj, "a bus that is slack and zero-injection"
            m = c.mask_bytes()[b] == 1
            if m.any():
                assert (m & (t[:, 2] == 0) & (t[:, 3] == 0)).any() or c.mask == "last", "p = q = 0 at a measured bus"
            assert (t[:, 2] < 0).any() and (t[:, 3] < 0).any()
        if c.draws == "six":
            assert (np.abs(z) == 6).all() and (z > 0).any() and (z < 0).any() and (t[:, 2:4] <= 0).all()
            assert (dc.edge_tables(c)[0][:, 2:4] <= 0).all()
        if not c.zinj:
            assert (t[:, 6] == 0).all()


@pytest.mark.parametrize("which", ["nodes", "edges"])
def test_floor_tables_sit_on_the_cap_edge(which):
    """fp32 |std| = the floor, two values below, five above; 1/floor^2 is NOT below the cap and each of the five above is: the oracle
    zeroes the first three and keeps the others, the first kept one being the largest weight below the cap."""
    floor, cap = (dc.NODE_FLOOR, dc.NODE_CAP) if which == "nodes" else (dc.EDGE_FLOOR, dc.EDGE_CAP)
    tg = dc.around(floor)
    assert tg[2] == floor and (np.diff(tg) > 0).all() and len(tg) == 8
    one = np.float32(1)
    w = one / (np.maximum(tg, floor) ** 2)
    assert w.dtype == np.float32 and not (w[2] < cap) and (w[3:] < cap).all() and (np.diff(w[3:]) <= 0).all()
    for c in (c for c in dc.MEASURE_CASES if c.values == "floor"):
        k = np.arange(c.rows) % 8
        if which == "nodes":
            t, _ = dc.node_tables(c)
            std = np.abs((t[:, 0] * dc.NOISE_DEFAULT["v_noise"]).astype(np.float32))
            std2 = np.abs((t[:, 2] * dc.NOISE_DEFAULT["pm_noise"]).astype(np.float32))
            ref, cols = dc.ref_nodes(c), (1, 5)
        else:
            t, _ = dc.edge_tables(c)
            std = np.abs((t[:, 2] * dc.NOISE_DEFAULT["p_noise"]).astype(np.float32))
            std2 = np.abs((t[:, 3] * dc.NOISE_DEFAULT["p_noise"]).astype(np.float32))
            ref, cols = dc.ref_edges(c), (1, 3)
        assert np.array_equal(std, tg[k]) and np.array_equal(std2, tg[(k + 3) % 8])
        for col, kk in zip(cols, (k, (k + 3) % 8)):
            got = ref[:, col]
            assert (got[kk <= 2] == 0).all(), "at and below the floor the cap zeroes the weight"
            assert np.array_equal(got[kk >= 3], w[kk[kk >= 3]]) and (got[kk == 3] == w[3]).all()
            assert got.max() == w[3] and w[3] < cap, "the largest weight still below the cap is present"


def test_nonfinite_tables_give_the_oracles_nan_weights():
    """Finding 2: a NaN raw value gives value NaN AND weight NaN in the reference path; max-that-drops-NaN followed by the cap gives 0."""
    c = next(c for c in dc.MEASURE_CASES if c.name == "nonfinite")
    x, ea = dc.ref_nodes(c), dc.ref_edges(c)
    assert np.isnan(x[3, 0]) and np.isnan(x[3, 1]) and np.isnan(x[24, 4]) and np.isnan(x[24, 5]) and np.isnan(x[45, 3])
    assert np.isinf(x[10, 0]) and x[10, 1] == 0 and x[17, 1] == 0 and x[31, 5] == 0
    assert np.isnan(ea[3, 0]) and np.isnan(ea[3, 1]) and np.isnan(ea[24, 3]) and ea[10, 1] == 0 and np.isinf(ea[40, 4])
    s = np.float32(np.nan)
    dropped = np.float32(1) / np.fmax(np.abs(s), dc.NODE_FLOOR) ** 2            # fmaxf: the NaN operand is dropped
    assert not (dropped < dc.NODE_CAP)                                            # ... and the cap makes the weight 0
    u = next(c for c in dc.MEASURE_CASES if c.name == "nonfinite_unmeasured")
    assert np.isnan(dc.ref_nodes(u)[3, 0]) and np.isnan(dc.ref_nodes(u)[3, 1]), "NaN * 0 = NaN: an unmeasured NaN stays one"


def test_zscore_cases_cover_the_issue():
    cs = dc.ZSCORE_CASES
    assert [c.rows for c in cs[:len(dc.ZS_ROWS)]] == dc.ZS_ROWS
    assert {c.num_feat for c in cs} >= set(dc.ZS_NUM_FEAT) and {c.layout for c in cs} == set(dc.ZS_LAYOUTS)
    assert any(c.ld == c.num_feat for c in cs) and any(c.ld > c.num_feat for c in cs)
    assert {k for c in cs for k in c.kinds} == set(dc.ZS_KINDS)
    big = max(cs, key=lambda c: c.rows * c.ld)
    assert (big.rows, big.ld, big.num_feat) == (66_305, 16, 16)
    for lay in dc.ZS_LAYOUTS:
        assert {k for c in cs if c.layout == lay for k in c.kinds} == set(dc.ZS_KINDS)


@pytest.mark.parametrize("c", dc.ZSCORE_CASES, ids=lambda c: c.name)
def test_zscore_bounded_columns_and_fp32_restatement(c):
    t = dc.zscore_table(c)
    n, mean64, std64 = dc.stats64(t, c.num_feat)
    mean32, std32 = dc.stats32(t, c.num_feat)
    omean, ostd = dc.oracle_stats(t, c.num_feat)
    for j, kind in enumerate(c.kinds):
        if kind in dc.ZS_BOUNDED:
            if std64[j] > 0:
                assert abs(mean64[j]) / std64[j] <= dc.ZS_MAX_RATIO, (j, kind)
            assert abs(mean32[j] - mean64[j]) <= dc.ZS_MEAN_BOUND * abs(mean64[j]), (j, kind)
            assert abs(std32[j] - std64[j]) <= dc.ZS_STD_BOUND * std64[j], (j, kind)
        elif kind == "allzero":
            assert n[j] == 0 and omean[j] == 0 and ostd[j] == 0
        elif kind == "single":
            assert n[j] == 1 and omean[j] == np.float32(-2.75) and ostd[j] == 0
        elif kind == "negzero":
            assert n[j] == min(2, c.rows) and (np.signbit(t[:, j]) & (t[:, j] == 0)).any() == (c.rows > 2)
        elif kind == "subnormal":
            assert ostd[j] == 0 and std64[j] > 0 or c.rows == 1, "the fp32 squares underflow"
        elif kind == "nan":
            assert omean[j] == 0 and ostd[j] == 0
        elif kind == "inf":
            assert omean[j] == np.float32(dc.FLT_MAX) and ostd[j] == (0 if (t[:, j] == 0).any() else np.float32(dc.FLT_MAX))
        elif kind == "inf_dense":
            assert omean[j] == -np.float32(dc.FLT_MAX) and ostd[j] == np.float32(dc.FLT_MAX) and not (t[:, j] == 0).any()
    if "subnormal" in c.kinds and c.rows > 1:
        j = c.kinds.index("subnormal")
        out = dc.ref_normalised(t, c.num_feat, omean, ostd)[:, j]
        assert set(np.unique(np.abs(out[t[:, j] != 0]))) == {np.float32(dc.FLT_MAX)} and (out[t[:, j] == 0] == 0).all()


def test_mean_rounded_twice_fails_on_the_constant_columns_and_once_does_not():
    """Finding 1.  fl(fl(n v) / n) != v for the value of every count that is no power of two; (float)(n v / n) = v for all of them
    and for every one of the 20 000 candidates at every count."""
    vals = dc.const_values()
    assert vals[3] == np.float32(1.4595472812652588) and vals[960] == np.float32(1.8317632675170898)
    cand = (0.01 + 2.0 * np.random.default_rng(7).random(20_000)).astype(np.float32)
    for n in dc.CONST_COUNTS:
        v = vals[n]
        assert dc.mean_one_rounding(n, v) == v
        assert np.array_equal(dc.mean_one_rounding(n, cand), cand)
        if n & (n - 1):
            assert dc.mean_two_roundings(n, v) != v, n
            frac = float((dc.mean_two_roundings(n, cand) != cand).mean())
            assert 0.01 < frac < 0.25, (n, frac)
        else:
            assert np.array_equal(dc.mean_two_roundings(n, cand), cand)
    assert sorted({n for g in dc.CONST_GROUPS for n in g}) == dc.CONST_COUNTS and all(len(g) <= 16 for g in dc.CONST_GROUPS)
    for g, counts in enumerate(dc.CONST_GROUPS):
        t = dc.const_table(g)
        n, mean64, std64 = dc.stats64(t, len(counts))
        assert n.tolist() == counts and (std64 == 0).all() and np.signbit(t[:, 0]).any()
        assert [np.float32(m) for m in mean64] == [vals[k] for k in counts]
        # a mean one ulp off: the ulp becomes the "std" and every measured entry +-1
        bad = dc.mean_two_roundings(np.array(counts), [vals[k] for k in counts])
        out = dc.ref_normalised(t, len(counts), bad, np.abs(bad - np.array([vals[k] for k in counts], np.float32)))
        assert any((np.abs(out[:, j][t[:, j] != 0]) == 1).all() for j, k in enumerate(counts) if k & (k - 1))


def test_collate_references():
    src = dc.collate_source(1, 0, 3, S=4)
    got = dc.ref_collate(1, 0, src, np.array([2, 0]), 2, 10)
    assert got.tolist() == [[12, 13, 14, 10, 11, 12], [15, 16, 17, 13, 14, 15]]
    assert dc.ref_collate(1, 1, dc.collate_source(1, 1, 2), None, 2, 5).tolist() == [[0, 1, 5, 6], [2, 3, 7, 8]]
    big = dc.ref_collate(1, 0, src, None, 3, 2 ** 31)
    assert big.dtype == np.int64 and big[1, -1] == 17 + 2 * 2 ** 31
    for how in dc.COLLATE_IDS:
        for B in dc.COLLATE_BATCHES:
            ids = dc.collate_ids(how, B)
            assert ids is None or (ids.min() >= 0 and ids.max() < dc.COLLATE_S and len(ids) == B)
    assert len(set(dc.collate_ids("repeats", 17).tolist())) < 17
    for lay in dc.COLLATE_LAYOUTS.values():
        assert sorted(ch for _, _, ch in lay) == [1, 255, 257, 11 * 179] and sorted((k, s) for k, s, _ in lay) == [(0, 0), (1, 0), (1, 1), (2, 0)]
    assert dc.cursor_reads(50, 16, 40).tolist() == list(range(40, 50)) + list(range(6)) and dc.cursor_next(50, 16, 40) == 6
    assert dc.cursor_reads(5, 16, 3).tolist() == [(3 + b) % 5 for b in range(16)] and dc.cursor_next(5, 16, 3) == 4
    assert dc.cursor_reads(-3, 16, 7).tolist() == list(range(7, 23)) and dc.cursor_next(0, 16, 7) == 23
    assert all(0 <= dc.cursor_next(L, B, p) < L for L, B, p in dc.CURSOR_CASES if L > 0)
    assert max(p + B for L, B, p in dc.CURSOR_CASES if L <= 0) <= dc.CURSOR_IDS


@pytest.mark.parametrize("m", range(len(dc.RAGGED_MIXES)))
def test_ragged_mix_equals_the_oracles_collate(m):
    mix = dc.ragged_mix(m)
    xs, eis, eas, ys = [], [], [], []
    for k, s in mix["slots"]:
        st = dc.ragged_store(k)
        xs.append(torch.from_numpy(st["x"][s])); ys.append(torch.from_numpy(st["y"][s])); eas.append(torch.from_numpy(st["ea"][s]))
        eis.append(torch.from_numpy(st["ei"] if st["shared"] else st["ei"][s]))
    x, ei, ea, y = dso.collate(xs, eis, eas, ys)
    assert np.array_equal(x.numpy(), mix["x"]) and np.array_equal(y.numpy(), mix["y"]) and np.array_equal(ea.numpy(), mix["ea"])
    assert np.array_equal(ei.numpy(), mix["ei"]) and mix["ei"].shape == (2, mix["E"]) and mix["x"].shape == (mix["N"], 11)
    assert [len(t["samp"]) for t in mix["tables"]] == list(mix["counts"])
    order = np.array([k for k, _ in mix["slots"]])
    if len(mix["cases"]) > 1 and len(order) > 3:
        assert (np.diff(order) != 0).sum() >= 2, "the slots of the cases are interleaved"


def test_ragged_cases_and_mixes_cover_the_issue():
    assert [(n, e) for n, e, _, _ in dc.RAGGED_CASES] == [(1, 1), (2, 1), (15, 14), (15, 15), (70, 69)]
    assert {s for _, _, s, _ in dc.RAGGED_CASES} == {0, 1}
    assert {len(c) for c, _ in dc.RAGGED_MIXES} == {1, 2, 3, 4} and ((0, 2, 3, 4), (3, 0, 5, 1)) in dc.RAGGED_MIXES
    assert {k for c, n in dc.RAGGED_MIXES for k, cnt in zip(c, n) if cnt} == set(range(5))


def test_zscore_refusal_table_is_narrower_than_the_column_limit():
    """num_feat > ld must be a refusal of its own: with ld = 16 it would fold into the refusal of 17 columns."""
    c, nf = dc.ZS_REFUSAL_CASE, dc.ZS_REFUSAL_NUM_FEAT
    assert 1 <= nf < c.ld < 16 and dc.zscore_table(c).shape == (c.rows, c.ld)


def _small_raw():
    T = dc.small_tables()
    raw_x = np.concatenate([dso.measure_nodes(T["nodes"][i, :, 0:4], T["nodes"][i, :, 5], T["nodes"][i, :, 6], T["meas_v"], T["noise"],
                                              T["z_nodes"][i]).numpy() for i in range(3)])
    raw_e = np.concatenate([dso.measure_edges(T["edges"][i, :, 2:4], T["edges"][i, :, 4:6], T["meas_pflow"], T["noise"],
                                              T["z_edges"][i]).numpy() for i in range(3)])
    return T, raw_x, raw_e


def test_small_tables_keep_the_std_bounds_condition():
    """test_data_from_tables_small applies the z-score's bounds to these tables: |mean| / std <= 100 wherever std > 0, and the fp32
    restatement inside both bounds."""
    _, raw_x, raw_e = _small_raw()
    for raw, nf in ((raw_x, 8), (raw_e, 6)):
        n, mean64, std64 = dc.stats64(raw, nf)
        mean32, std32 = dc.stats32(raw, nf)
        assert (np.abs(mean64)[std64 > 0] / std64[std64 > 0] <= dc.ZS_MAX_RATIO).all(), (mean64, std64)
        assert (np.abs(mean32 - mean64) <= dc.ZS_MEAN_BOUND * np.abs(mean64)).all()
        var = std64 > 0          # (a constant column has std64 = 0: the restatement's twice-rounded mean leaves an ulp there, the
        assert (np.abs(std32 - std64)[var] <= dc.ZS_STD_BOUND * std64[var]).all()      # defect the once-rounded mean removes)
        assert (n[~var] <= 3).all()


def test_small_tables_oracle_turns_the_constant_column_into_rounding_noise():
    """Column 3 of x (the weight of theta, set at the slack bus only) holds one value three times.  The oracle's own fp32 column sum puts
    its mean off that value, the difference becomes its "std", and its z-scores are +-1: the one column whose zero pattern
    test_data_from_tables_small does not take from the oracle's own run (a once-rounded mean gives std 0 and z-scores 0 there)."""
    T, raw_x, _ = _small_raw()
    keys = ("nodes", "edges", "labels", "noise", "meas_v", "meas_pflow", "z_nodes", "z_edges")
    own = dso.data_from_tables(*(T[k] for k in keys))
    const = [c for c in range(8) if len(np.unique(raw_x[:, c][raw_x[:, c] != 0])) == 1]
    assert const == [3]
    v = raw_x[:, 3][raw_x[:, 3] != 0]
    assert len(v) == 3 and own["x_mean"][3].item() != v[0] and own["x_std"][3].item() == abs(own["x_mean"][3].item() - float(v[0]))
    z = own["x"][:, 3].numpy()
    assert (np.abs(z[raw_x[:, 3] != 0]) == 1).all() and (z[raw_x[:, 3] == 0] == 0).all()
    assert dc.mean_one_rounding(3, v[0]) == v[0]
