"""Times estimator.wls_estimate_banded (csrc/dss2_wls_banded.hpp: the blocked kernel on a band of the gain matrix, buses numbered by
estimator.band_order) on the GPU.

The protocol of tools/wls_large_probe.py -- median of --runs calls after --warmup, device events around each call, max_iter = 8 and
tol = 0 so that every graph runs all eight iterations; the ordering is made once, before the clock.  Where the dense blocked form serves
the grid too (up to 256 buses) it is timed in the same run, the two arms taking turns call by call.  Default cases: ober179 and radial256
(synthetic.register_radial(256): a feeder at the dense form's cap, in place of the tests' 256-bus `cap` graph, which is a fixture and no
grid that make_batch draws samples of) at B = 1024 against the dense form (and wls_bad_data_large against wls_bad_data_banded); beside the
plain banded solve, in the same turns: wls_bad_data_banded with max_removals = 0 and wls_robust_banded at gamma = 3; radial300 and radial1000 at
B = 256, banded alone.  A case is grid:graphs[:seed] (seed 1 unless given; radial300 runs with seed 2: at B = 256 the batches of seeds 0
and 1 hold one injection weight near 4e6 times the typical one, the fp32 normalisation of x then rounds the small weights away, and every
graph's gain matrix is singular at the flat start -- in the fp64 oracle as in the kernel, status 2 and no iteration).  Per case: hb, the
workspace, and the state against wls_probe's torch fp64 iteration on the CPU on the first --check-graphs graphs.  One JSON line per
case.  No CPU fallback: without a GPU it fails.

    python tools/wls_banded_probe.py [--runs 20] [--warmup 5] [--cases ober179:1024,radial256:1024,radial300:256:2,radial1000:256]
                                     [--out profiles/wls_banded_probe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wls_probe import TorchWLS, e_of, pkg  # noqa: E402


def timed_in_turns(fns, warmup, runs):
    """[(median, min, max) ms per fn]: the functions take turns, call by call."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="ober179:1024,radial256:1024,radial300:256:2,radial1000:256")
    ap.add_argument("--check-graphs", type=int, default=4, help="graphs whose states are checked against the CPU fp64 iteration")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wls_banded_probe: needs the GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    est, syn = pkg.estimator, pkg.synthetic
    ms = lambda t: {"median": t[0], "min": t[1], "max": t[2]}
    lines = []
    for case in a.cases.split(","):
        grid, B, seed = (case.split(":") + ["1"])[:3]
        B, seed = int(B), int(seed)
        if grid.startswith("radial"):
            grid = syn.register_radial(int(grid[len("radial"):]))
        n = syn.load_grid(grid).n
        b = syn.make_batch([grid], B, seed=seed)
        d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items() if k != "stats"}
        stats = tuple(s.to(dev) for s in b["stats"])
        run = lambda entry, **kw: entry(d["x"], d["edge_index"], d["edge_attr"], *stats, n, max_iter=8, tol=0.0, **kw)
        order = est.band_order(d["edge_index"], n, num_nodes=d["x"].size(0))
        hb = order.half_bandwidth
        line = {"case": grid, "graphs": B, "seed": seed, "buses_per_graph": n, "max_iter": 8, "device": torch.cuda.get_device_name(0), "runs": a.runs,
                "warmup": a.warmup, "half_bandwidth": hb, "block_columns_kept": est.band_blocks(hb) + 1, "orderings": order.n_orderings,
                "workspace_bytes": est.band_workspace_bytes(n, hb, est.band_groups(B)), "lds_bytes": est.band_lds_bytes(n, hb)}
        # the plain banded solve, then the two answers to gross errors on the band: bad-data detection without a removal (one solve, one
        # more factorisation, the selected inverse, the measurement pass) and the Huber form (gamma = 3, the same eight iterations)
        arms = [lambda: run(est.wls_estimate_banded, order=order), lambda: run(est.wls_bad_data_banded, order=order, max_removals=0),
                lambda: run(est.wls_robust_banded, order=order, gamma=3.0)]
        dense = n <= est.max_nodes_per_graph_large()
        if dense:
            arms += [lambda: run(est.wls_estimate_large), lambda: run(est.wls_bad_data_large, max_removals=0)]
            line["dense_workspace_bytes"] = int(pkg._lib.lib().dss2_wls_large_workspace_bytes(n, min(B, 512)))
        t = timed_in_turns(arms, a.warmup, a.runs)
        line["banded_solve_ms"] = ms(t[0])
        line["banded_bad_data_ms"], line["banded_robust_ms"] = ms(t[1]), ms(t[2])
        line["bad_data_over_banded_solve"], line["robust_over_banded_solve"] = t[1][0] / t[0][0], t[2][0] / t[0][0]
        line["lds_bytes_bad_data"] = est.band_lds_bytes(n, hb, bad_data=True)
        if dense:
            line["dense_solve_ms"] = ms(t[3])
            line["dense_over_banded"] = t[3][0] / t[0][0]
            line["dense_bad_data_ms"] = ms(t[4])
            line["dense_bad_data_over_dense_solve"] = t[4][0] / t[3][0]
            line["dense_bad_data_over_banded_bad_data"] = t[4][0] / t[1][0]
        k = min(B, a.check_graphs)
        sub = dict(b, x=b["x"][:k * n], edge_attr=b["edge_attr"][:k * e_of(b, B)], edge_index=b["edge_index"][:, :k * e_of(b, B)])
        cpu = TorchWLS(sub, n, torch.device("cpu")).solve(8)
        per_graph = lambda s_: (s_[:k * n].double().cpu() - cpu).abs().reshape(k, -1).max(1).values
        summary = lambda v: {"max": v.max().item(), "median": v.median().item(), "graphs_beyond_5e-7": int((v > 5e-7).sum())}
        res = run(est.wls_estimate_banded, order=order)
        line["state_check"] = {"graphs_checked": k, "banded_vs_cpu_fp64": summary(per_graph(res.state)), "failed": int((res.status == 2).sum()),
                               "iterations_mean": res.iterations.double().mean().item()}
        if dense:
            line["state_check"]["banded_vs_dense_max"] = (res.state - run(est.wls_estimate_large).state).abs().max().item()
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
