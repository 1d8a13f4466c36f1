"""Times estimator.wls_bad_data_large (the blocked form of csrc/dss2_wls_bad_data.hip) beside estimator.wls_estimate_large on the same
batch, GPU and process -- and, where the LDS form serves the grid too (ober_sub), beside estimator.wls_bad_data and wls_estimate.

For ober179 and ober_sub at B = 1024, at max_iter = 8 and tol = 0 (every solve runs all eight iterations), device events around each
call, median of --runs calls after --warmup calls:
  (a) wls_estimate_large: the blocked solve alone;
  (b) wls_bad_data_large with max_removals = 0: the solve, one more factorisation, the inversion on the block rows, normalized
      residuals, the chi-square test;
  (c) wls_bad_data_large with max_removals = 1, threshold = 4 on the batch with one measurement per graph moved by 25 sigma
      (synthetic.corrupt_measurements): a second round for every graph that removes one;
  (d) up to 99 buses: wls_estimate and wls_bad_data (the LDS kernels) with the arguments of (a), (b) and (c).
Prints one JSON line per case.  No CPU fallback: without a GPU it fails.

    python tools/wls_bad_data_large_probe.py [--runs 20] [--warmup 5] [--cases ober179:1024,ober_sub:1024] [--out FILE]
"""
import argparse
import json
import os

import torch

from wls_probe import pkg, timed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="ober179:1024,ober_sub:1024")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wls_bad_data_large_probe: needs the GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    est = pkg.estimator
    lines = []
    for case in a.cases.split(","):
        grid, B = case.split(":")
        B = int(B)
        n = pkg.synthetic.load_grid(grid).n
        b = pkg.synthetic.make_batch([grid], B, seed=1)
        noisy, _ = pkg.synthetic.corrupt_measurements(b, per_graph=1, sigmas=25.0, seed=1)
        stats = tuple(s.to(dev) for s in b["stats"])
        on_dev = lambda bb: [bb[k].to(dev) for k in ("x", "edge_index", "edge_attr")]
        clean, bad = on_dev(b), on_dev(noisy)
        kw = dict(max_iter=8, tol=0.0)
        one = dict(threshold=4.0, max_removals=1, **kw)
        ms = lambda t: {"median": t[0], "min": t[1], "max": t[2]}
        solve = timed(lambda: est.wls_estimate_large(*clean, *stats, n, **kw), a.warmup, a.runs)
        detect = timed(lambda: est.wls_bad_data_large(*clean, *stats, n, **kw), a.warmup, a.runs)
        remove = timed(lambda: est.wls_bad_data_large(*bad, *stats, n, **one), a.warmup, a.runs)
        res = est.wls_bad_data_large(*bad, *stats, n, **one)
        line = {"case": grid, "graphs": B, "buses_per_graph": n, "max_iter": 8, "device": torch.cuda.get_device_name(0), "inversion": "blocked, 16 rows",
                "wls_estimate_large_ms": ms(solve), "wls_bad_data_large_no_removals_ms": ms(detect), "bad_data_large_over_estimate_large": detect[0] / solve[0],
                "wls_bad_data_large_one_removal_ms": ms(remove), "one_removal_over_estimate_large": remove[0] / solve[0],
                "graphs_that_removed_one": int(res.n_removed.sum()), "mean_iterations_with_removal": res.iterations.double().mean().item(),
                "runs": a.runs, "warmup": a.warmup}
        if n <= est.max_nodes_per_graph():
            lds_solve = timed(lambda: est.wls_estimate(*clean, *stats, n, **kw), a.warmup, a.runs)
            lds_detect = timed(lambda: est.wls_bad_data(*clean, *stats, n, **kw), a.warmup, a.runs)
            lds_remove = timed(lambda: est.wls_bad_data(*bad, *stats, n, **one), a.warmup, a.runs)
            lds = est.wls_bad_data(*bad, *stats, n, **one)
            line.update({"wls_estimate_ms": ms(lds_solve), "wls_bad_data_no_removals_ms": ms(lds_detect), "bad_data_over_estimate": lds_detect[0] / lds_solve[0],
                         "wls_bad_data_one_removal_ms": ms(lds_remove), "bad_data_large_over_bad_data": detect[0] / lds_detect[0],
                         "one_removal_large_over_lds": remove[0] / lds_remove[0], "both_forms_remove_the_same": bool(torch.equal(lds.removed, res.removed))})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
