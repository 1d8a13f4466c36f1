"""The weight gradient's one selection function (dss2_wgrad_plan, csrc/dss2_wgrad.hip) on the host: which kernel a launch of the
benchmark's shapes runs and with which geometry, the three older shape queries as readers of the same record, and the environment
switches, each changing the shapes it governs and no other.  No GPU needed: the library answers from the arguments alone."""
import itertools
import json
import os
import subprocess
import sys

from conftest import ROOT, load_pkg      # (puts the oracle folder on the path)
import dss2_topology_oracle as topo_oracle

_BENCH = {}


def _bench_tiles(name):
    """(nrb, ELL width, largest tile nnz) of the by-source tiles of a bench.py configuration's graphs, from the CPU oracle (per tile: a few graphs do)."""
    if not _BENCH:
        sys.path.insert(0, ROOT)
        import bench
        tagged = lambda start: [c for c in bench.OTHER_CONFIGS if c[0].startswith(start)][0][1]
        grids = {"C2": tagged("C2 shape"), "C3": tagged("C3 ober_sub"), "179": tagged("C3' ober179"), "C5": tagged("C5 model")}
        assert grids == {"C2": ["cigre14"], "C3": ["ober_sub"], "179": ["ober179"], "C5": ["cigre14", "cigre14_reswitched"]}
        assert [c[4][3] for c in bench.OTHER_CONFIGS if c[3] == "SkipPFN"] == [32, 32, 32]      # the driver line: H = 32
        pkg = load_pkg()
        for key, nrb in (("C2", None), ("C2/32", 1), ("C3", None), ("179", None), ("C5", None)):
            b = pkg.synthetic.make_batch(grids[key.split("/")[0]], 16, seed=0)
            o = topo_oracle.TopologyOracle(b["edge_index"], b["x"].shape[0], **({} if nrb is None else {"nrb": nrb}))
            _BENCH[key] = (o.nrb, o.ellT, o.max_nnzT)
    return _BENCH[name]


F16 = 2 | 2 << 8      # the f16x3 mode word with two headroom bits
# label: (tiles, nmat, hout, hin, mode word, narrow, n_layers)
CASES = {
    "C2 primary, 64 rows": ("C2", 3, 128, 128, 1, 0, 3),
    "C2 alternate, 32 rows": ("C2/32", 3, 128, 128, F16, 0, 3),
    "C2 alternate, gathered hops": ("C2/32", 3, 128, 128, F16 | 1 << 16, 0, 3),
    "C2 alternate as bf16x6": ("C2/32", 3, 128, 128, 1, 0, 3),
    "C2 alternate, K = 1": ("C2/32", 2, 128, 128, F16, 0, 1),
    "C5, 64 rows, H = 256": ("C5", 3, 256, 256, 1, 0, 7),
    "C3, 96 rows": ("C3", 3, 128, 128, F16, 0, 3),
    "C3 as bf16x6": ("C3", 3, 128, 128, 1, 0, 3),
    "179-bus feeder, 192 rows": ("179", 3, 128, 128, F16, 0, 3),
    "179-bus feeder as fp32 (W8)": ("179", 3, 128, 128, 0, 0, 3),
    "driver line, 32 rows, H = 32": ("C2/32", 3, 32, 32, F16, 0, 7),
    "driver line, 64 rows, H = 32": ("C2", 3, 32, 32, 1, 0, 7),
    "driver line, 96 rows, H = 32, one layer": ("C3", 3, 32, 32, F16, 0, 1),
    "driver line, 96 rows, H = 32, PAIR": ("C3", 3, 32, 32, F16, 0, 7),
    "narrow head, H -> 2": ("C2", 3, 2, 128, 0, 1, 0),
    "narrow head, H -> 8": ("C2", 3, 8, 128, 0, 1, 0),
    "narrow head in a batch of one": ("C2", 3, 2, 128, 0, 1, 1),
    "K = 3": ("C2/32", 4, 128, 128, F16, 0, 3),
    "ELL width 9": (("C2/32", 9), 3, 128, 128, F16, 0, 3),
    "160 rows (nrb = 5)": (("C3", None, 5), 3, 128, 128, F16, 0, 3),
    "160 rows as bf16x6": (("C3", None, 5), 3, 128, 128, 1, 0, 3),
    "160 rows as fp32": (("C3", None, 5), 3, 128, 128, 0, 0, 3),
}
# label: (kernel, nb, w8, grid_y, z_groups, y_slices, launch_lds, sizing_lds, f16x3_covers).  sizing_lds and y_slices (and z_groups, where the older query
# has the arguments to say it) are the PARENT library's dss2_wgrad_lds_bytes_ex / _y_slices / _batched_groups answers, run on these shapes;
# the kernel is the one the parent's dispatch chain reaches for them (16h -> 16th -> 16 -> pick_nb / W8 / table); launch_lds its launcher's formula;
# f16x3_covers is where the parent's ops._wgrad_mode formed headroom bits (32- and 96- .. 192-row tiles, K <= 2, ELL slices of 1 .. 8), at these widths.
EXPECT = {
    "C2 primary, 64 rows": ("BF16_64", 0, 0, 1, 3, 1, 157184, 157184, 0),
    "C2 alternate, 32 rows": ("F16_32", 0, 0, 2, 3, 2, 45088, 78848, 1),
    "C2 alternate, gathered hops": ("F16_32", 0, 0, 2, 3, 2, 59424, 78848, 1),
    "C2 alternate as bf16x6": ("BF16_32", 0, 0, 2, 3, 2, 78848, 78848, 1),
    "C2 alternate, K = 1": ("F16_32", 0, 0, 2, 1, 2, 36896, 66560, 1),
    "C5, 64 rows, H = 256": ("BF16_64", 0, 0, 4, 7, 4, 157696, 157696, 0),
    "C3, 96 rows": ("F16_TALL", 0, 0, 2, 3, 2, 109632, 150528, 1),
    "C3 as bf16x6": ("BF16_TALL", 0, 0, 2, 3, 2, 150528, 150528, 1),
    "179-bus feeder, 192 rows": ("F16_TALL", 0, 0, 2, 3, 2, 153664, 116736, 1),
    "179-bus feeder as fp32 (W8)": ("FP32", 1, 1, 4, 3, 1, 155136, 159232, 1),
    "driver line, 32 rows, H = 32": ("FP32", 1, 0, 1, 7, 1, 21760, 21760, 0),
    "driver line, 64 rows, H = 32": ("FP32", 1, 0, 1, 7, 1, 39424, 39424, 0),
    "driver line, 96 rows, H = 32, one layer": ("F16_TALL", 0, 0, 1, 1, 1, 109632, 44800, 1),
    "driver line, 96 rows, H = 32, PAIR": ("F16_TALL_PAIR", 0, 0, 1, 4, 1, 109632, 44800, 1),
    "narrow head, H -> 2": ("NARROW_STREAM", 0, 0, 1, 1, 1, 36352, 47616, 0),
    "narrow head, H -> 8": ("FP32_NARROW", 1, 0, 1, 1, 1, 47616, 47616, 0),
    "narrow head in a batch of one": ("FP32_NARROW", 1, 0, 1, 1, 1, 47616, 47616, 0),
    "K = 3": ("FP32", 2, 0, 2, 3, 1, 42240, 42240, 0),
    "ELL width 9": ("FP32", 4, 0, 1, 3, 1, 76544, 76544, 0),
    "160 rows (nrb = 5)": ("F16_TALL", 0, 0, 2, 3, 2, 128064, 107520, 1),
    "160 rows as bf16x6": ("BF16_TALL", 0, 0, 2, 3, 2, 107520, 107520, 1),
    "160 rows as fp32": ("NONE", 1, 0, 1, 3, 1, 0, 133376, 1),
}
KERNELS = ("NONE", "NARROW_STREAM", "FP32_NARROW", "FP32", "BF16_64", "BF16_32", "BF16_TALL", "F16_32", "F16_TALL", "F16_TALL_PAIR")


def _args(pkg, label):
    tiles, nmat, hout, hin, mode, narrow, _ = CASES[label]
    key, ell, nrb = (tiles + (None, None))[:3] if isinstance(tiles, tuple) else (tiles, None, None)
    nrb0, ell0, nnz = _bench_tiles(key)
    a = pkg._lib.WgradArgs()
    a.nrb, a.ell_width, a.max_nnz = nrb or nrb0, ell or ell0, nnz * (nrb or nrb0) // nrb0
    a.nmat, a.hout, a.hin, a.ldg, a.ldx, a.mfma_bf16, a.narrow = nmat, hout, hin, hout, hin, mode, narrow
    a.ell_tiles = 64      # (any aligned non-null address: the host never reads through it)
    return a


def _plan(pkg, a, n_layers):
    p = pkg._lib.WgradPlan()
    assert pkg._lib.lib().dss2_wgrad_plan(a, n_layers, p) == 0
    return p


def _plan_row(pkg, label):
    p = _plan(pkg, _args(pkg, label), CASES[label][6])
    return (KERNELS[p.kernel], p.nb, p.w8, p.grid_y, p.z_groups, p.y_slices, p.launch_lds, p.sizing_lds, p.f16x3_covers)


def test_the_benchmarks_shapes_are_pinned():
    pkg = load_pkg()
    assert [getattr(pkg._lib, "WGRAD_" + k) for k in KERNELS] == list(range(len(KERNELS)))
    assert set(EXPECT) == set(CASES)
    for label in CASES:
        assert _plan_row(pkg, label) == EXPECT[label], label


def test_the_older_queries_read_the_plan():
    """dss2_wgrad_lds_bytes(_ex), _y_slices and _batched_groups against the record, over a reduced grid of shapes."""
    pkg = load_pkg()
    L = pkg._lib.lib()
    for nrb, nmat, h, ell, mode, nl in itertools.product((1, 2, 3, 5, 6), (1, 2, 3, 4), (6, 32, 36, 128, 256), (0, 3, 8, 9), (0, 1, F16), (1, 2, 7)):
        for hin, nnz in ((h, 8 * 32 * nrb), (128, 4000 * nrb)):
            a = pkg._lib.WgradArgs()
            a.nrb, a.nmat, a.hout, a.hin, a.max_nnz, a.ell_width, a.mfma_bf16 = nrb, nmat, h, hin, nnz, ell, mode
            a.ell_tiles = 64 if ell else None
            p = _plan(pkg, a, nl)
            assert p.sizing_lds == L.dss2_wgrad_lds_bytes_ex(nrb, nmat, h, hin, nnz, ell, mode)
            assert mode or p.sizing_lds == L.dss2_wgrad_lds_bytes(nrb, nmat, h, hin, nnz, ell)
            assert p.y_slices == L.dss2_wgrad_y_slices(nrb, nmat, h, hin, ell, mode, 0) == L.dss2_wgrad_y_slices(nrb, nmat, h, hin, ell, mode, 1)
            if nmat in (2, 3) and 1 <= ell <= 8:      # (the older query names neither: it answers for a K and a width the tall f16x3 kernel takes)
                assert p.z_groups == L.dss2_wgrad_batched_groups(nrb, h, hin, mode, nl)
            assert (p.kernel == pkg._lib.WGRAD_NONE) == (p.reason != 0) and p.z_groups * (2 if p.kernel == pkg._lib.WGRAD_F16_TALL_PAIR else 1) in (nl, nl + 1)
            if p.kernel in (pkg._lib.WGRAD_BF16_64, pkg._lib.WGRAD_BF16_32, pkg._lib.WGRAD_BF16_TALL):      # bf16x6: sized by the kernel that runs
                assert (p.launch_lds, p.grid_y) == (p.sizing_lds, p.y_slices)


# switch = 0: {label: the kernel it becomes}; every other pinned row stays as it is
SWITCHES = {
    "DSS2_WGRAD_TALL_F16": {"C3, 96 rows": "BF16_TALL", "179-bus feeder, 192 rows": "BF16_TALL", "160 rows (nrb = 5)": "BF16_TALL",
                            "driver line, 96 rows, H = 32, one layer": "FP32", "driver line, 96 rows, H = 32, PAIR": "FP32"},
    "DSS2_WGRAD_TALL_PAIR": {"driver line, 96 rows, H = 32, PAIR": "F16_TALL"},
    "DSS2_WGRAD_TALL16": {"C3 as bf16x6": "FP32", "160 rows as bf16x6": "NONE"},
    "DSS2_WGRAD_TALL_DB": {},      # (same kernels; the bf16x6 tall-tile launches get one set of planes: their LDS is checked below)
    "DSS2_WGRAD_NB": {label: "NONE" for label, row in EXPECT.items() if row[0] == "FP32"},      # (no NB allowed: the fp32 table is closed)
    "DSS2_NARROW_STREAM": {"narrow head, H -> 2": "FP32_NARROW"},
    "DSS2_WGRAD_KSPLIT": {},       # (an argument of the fp32 kernel, no part of the selection)
}


def test_each_switch_governs_its_own_shapes():
    pkg = load_pkg()
    code = ("import json, sys; sys.path.insert(0, %r); import test_wgrad_plan_cpu as t; pkg = t.load_pkg(); "
            "print('ROWS' + json.dumps({k: t._plan_row(pkg, k) for k in t.CASES}))" % os.path.dirname(os.path.abspath(__file__)))
    procs = {sw: subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **{sw: "0"}), stdout=subprocess.PIPE, text=True) for sw in SWITCHES}
    for sw, pr in procs.items():
        out = pr.communicate()[0]
        assert pr.returncode == 0, sw
        rows = json.loads([ln for ln in out.splitlines() if ln.startswith("ROWS")][0][4:])
        changed = {k: v[0] for k, v in rows.items() if v[0] != EXPECT[k][0]}
        assert changed == SWITCHES[sw], sw
        for k, v in rows.items():
            if k in changed or v[0] == "NONE":      # (no kernel before and after: nothing else to hold)
                continue
            assert tuple(v[:5]) == EXPECT[k][:5], (sw, k)      # the launch: kernel, nb, w8, grid
            assert v[8] == EXPECT[k][8], (sw, k)               # no switch decides whether headroom bits are formed
            if sw == "DSS2_WGRAD_TALL_DB":
                assert v[6] <= EXPECT[k][6] and (v[6] == EXPECT[k][6] or v[0] == "BF16_TALL"), (sw, k)
            else:
                assert v[6] == EXPECT[k][6], (sw, k)
            # (the sizing figures are the bf16x6 / fp32 kernels' whichever kernel runs, so they follow those kernels' switches on every tall row)
            assert (v[5], v[7]) == (EXPECT[k][5], EXPECT[k][7]) or sw in ("DSS2_WGRAD_TALL16", "DSS2_WGRAD_TALL_DB", "DSS2_WGRAD_NB"), (sw, k)
        if sw == "DSS2_WGRAD_TALL_DB":
            assert rows["C3 as bf16x6"][6] < EXPECT["C3 as bf16x6"][6]
