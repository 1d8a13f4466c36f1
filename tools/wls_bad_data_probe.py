"""Times estimator.wls_bad_data (csrc/dss2_wls_bad_data.hip) beside estimator.wls_estimate on the same batch and GPU.

For cigre14 at B = 4096 and ober_sub at B = 1024, at max_iter = 8 and tol = 0 (every solve runs all eight iterations), device events
around each call, median of --runs calls after --warmup calls:
  (a) wls_estimate: the solve alone;
  (b) wls_bad_data with max_removals = 0: the solve, one more factorisation, the covariance, normalized residuals, the chi-square test;
  (c) wls_bad_data with max_removals = 1, threshold = 4 on the batch with one measurement per graph moved by 25 sigma
      (synthetic.corrupt_measurements): a second round for every graph that removes one.
Prints one JSON line per case.  No CPU fallback: without a GPU it fails.

    python tools/wls_bad_data_probe.py [--runs 20] [--warmup 5] [--cases cigre14:4096,ober_sub:1024] [--out FILE]
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
    ap.add_argument("--cases", default="cigre14:4096,ober_sub:1024")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wls_bad_data_probe: needs the GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
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
        ms = lambda t: {"median": t[0], "min": t[1], "max": t[2]}
        solve = timed(lambda: pkg.estimator.wls_estimate(*clean, *stats, n, **kw), a.warmup, a.runs)
        detect = timed(lambda: pkg.estimator.wls_bad_data(*clean, *stats, n, **kw), a.warmup, a.runs)
        remove = timed(lambda: pkg.estimator.wls_bad_data(*bad, *stats, n, threshold=4.0, max_removals=1, **kw), a.warmup, a.runs)
        res = pkg.estimator.wls_bad_data(*bad, *stats, n, threshold=4.0, max_removals=1, **kw)
        line = {"case": grid, "graphs": B, "buses_per_graph": n, "max_iter": 8, "device": torch.cuda.get_device_name(0),
                "wls_estimate_ms": ms(solve), "wls_bad_data_no_removals_ms": ms(detect), "bad_data_over_estimate": detect[0] / solve[0],
                "wls_bad_data_one_removal_ms": ms(remove), "graphs_that_removed_one": int(res.n_removed.sum()),
                "mean_iterations_with_removal": res.iterations.double().mean().item(), "runs": a.runs, "warmup": a.warmup}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
