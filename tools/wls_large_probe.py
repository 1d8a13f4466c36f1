"""Times estimator.wls_estimate_large (csrc/dss2_wls_large.hip: the gain matrix in global memory, blocked Cholesky) on the GPU.

The protocol of tools/wls_probe.py -- median of --runs calls after --warmup, device events around each call, max_iter = 8 and tol = 0 so
that every graph runs all eight iterations -- on ober179 at B = 1024 (358 states: no other entry serves it) and ober_sub at B = 1024
(140 states).  Beside each: wls_probe's torch fp64 iteration on the same GPU (dense batched H, cholesky_ex, cholesky_solve) and, on
ober_sub, estimator.wls_estimate (the LDS kernel) on the same batch in the same process.  The states of the HIP solves and of the torch
iteration are compared with the same torch iteration in fp64 on the CPU on the first --check-graphs graphs.  On ober179 also: iterations
to tol = 1e-6 at max_iter = 20 and the graphs that do not converge.  One JSON line per case.  No CPU fallback: without a GPU it fails.

    python tools/wls_large_probe.py [--runs 20] [--warmup 5] [--cases ober179:1024,ober_sub:1024] [--out profiles/wls_large_probe.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wls_probe import TorchWLS, e_of, pkg, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="ober179:1024,ober_sub:1024")
    ap.add_argument("--check-graphs", type=int, default=32, help="graphs whose states are checked against the CPU fp64 iteration")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wls_large_probe: needs the GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    est = pkg.estimator
    ms = lambda t: {"median": t[0], "min": t[1], "max": t[2]}
    lines = []
    for case in a.cases.split(","):
        grid, B = case.split(":")
        B = int(B)
        n = pkg.synthetic.load_grid(grid).n
        b = pkg.synthetic.make_batch([grid], B, seed=1)
        d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items() if k != "stats"}
        stats = tuple(s.to(dev) for s in b["stats"])
        run = lambda entry, **kw: entry(d["x"], d["edge_index"], d["edge_attr"], *stats, n, **kw)
        line = {"case": grid, "graphs": B, "buses_per_graph": n, "max_iter": 8, "device": torch.cuda.get_device_name(0), "runs": a.runs,
                "warmup": a.warmup}
        before = set(est._WORKSPACES)
        large = timed(lambda: run(est.wls_estimate_large, max_iter=8, tol=0.0), a.warmup, a.runs)
        line["workspace_bytes"] = sum(t.numel() for key, t in est._WORKSPACES.items() if key not in before)
        line["large_solve_ms"] = ms(large)
        k = min(B, a.check_graphs)
        sub = dict(b, x=b["x"][:k * n], edge_attr=b["edge_attr"][:k * e_of(b, B)], edge_index=b["edge_index"][:, :k * e_of(b, B)])
        cpu = TorchWLS(sub, n, torch.device("cpu")).solve(8)
        per_graph = lambda s_: (s_[:k * n].double().cpu() - cpu).abs().reshape(k, -1).max(1).values
        summary = lambda v: {"max": v.max().item(), "median": v.median().item(), "graphs_beyond_5e-7": int((v > 5e-7).sum())}
        state_large = run(est.wls_estimate_large, max_iter=8, tol=0.0).state
        line["state_check"] = {"graphs_checked": k, "large_vs_cpu_fp64": summary(per_graph(state_large))}
        if n <= est.max_nodes_per_graph():
            lds = timed(lambda: run(est.wls_estimate, max_iter=8, tol=0.0), a.warmup, a.runs)
            line["lds_solve_ms"] = ms(lds)
            line["large_over_lds"] = large[0] / lds[0]
            state_lds = run(est.wls_estimate, max_iter=8, tol=0.0).state
            line["state_check"]["lds_vs_cpu_fp64"] = summary(per_graph(state_lds))
            line["state_check"]["large_vs_lds_max"] = (state_large - state_lds).abs().max().item()
        ref = TorchWLS(b, n, dev)
        line["state_check"]["torch_gpu_vs_cpu_fp64"] = summary(per_graph(ref.solve(8)))
        tch = timed(lambda: ref.solve(8), max(2, a.warmup // 2), a.runs)
        del ref
        line["torch_fp64_ms"] = ms(tch)
        line["torch_over_large"] = tch[0] / large[0]
        if n > est.max_nodes_per_graph():
            flat = run(est.wls_estimate_large, max_iter=20, tol=1e-6)
            line["flat_start_tol_1e-6_max_iter_20"] = {"mean_iterations": flat.iterations.double().mean().item(),
                                                       "max_iterations": int(flat.iterations.max()), "not_converged": int((flat.status != 0).sum()),
                                                       "failed": int((flat.status == 2).sum()),
                                                       "max_abs_error_v_theta": (flat.state - d["y"]).abs().max(0).values.tolist()}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
