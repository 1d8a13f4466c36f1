"""Times the WLS estimator on a batch that MIXES bus counts: one launch through graph_ptr against what a user had to do before it.

The protocol of tools/wls_probe.py -- device events around each call, max_iter = 8 and tol = 0 so that every graph runs all eight
iterations, the median of --runs rounds after --warmup, the arms taking turns call by call -- on synthetic.make_batch of two grids:
cigre14 + ober_sub (15 and 70 buses: estimator.wls_estimate, the gain matrix in LDS) and ober_sub + ober179 (70 and 179 buses:
estimator.wls_estimate_large, the blocked kernel), B = 1024.  The batch is normalised with the statistics of a batch of --stats-graphs
graphs of the same grids (256, the driver's way): the statistics of 1024 graphs of cigre14 + ober_sub have a weight column whose fp32
standard deviation (1e7) rounds ober_sub's small weights away, its gain matrices are singular in the fp64 oracle too, and every such
graph ends at its first pivot -- a run that times nothing.  status_counts in the output says what the timed graphs did.  The arms:

  one_launch         the entry with graph_ptr and the largest bus count as the bound: one launch, nothing else
  split              today's way: per bus count index_select the rows and branches into a uniform batch (the index lists and the row
                     renumbering table are known on the host and uploaded before the clock starts), one call per size, the states
                     scattered back with index_copy_.  The sub-batches are new tensors every time, as they are for every new batch of
                     a loader: their graph structure is looked up by its hash, as for any fresh edge_index
  split_solves_only  the lower bound of `split`: the uniform sub-batches gathered and their structure cached before the clock starts;
                     the calls and the scatter alone

Recorded too: whether one_launch and split give the same bits (state, objective, iterations, status, last_step per graph), and the
batch's composition.  One JSON line per case, appended to --out.  No CPU fallback.

    python tools/wls_mixed_probe.py [--runs 20] [--warmup 5] [--graphs 1024] [--stats-graphs 256] [--cases cigre14+ober_sub,ober_sub+ober179]
                                    [--out profiles/wls_mixed_probe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wls_probe import pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--stats-graphs", type=int, default=256, help="the batch is normalised with the statistics of a batch of this many graphs (seed 0)")
    ap.add_argument("--cases", default="cigre14+ober_sub,ober_sub+ober179")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wls_mixed_probe: needs the GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    est = pkg.estimator
    kw = dict(max_iter=8, tol=0.0)
    for case in a.cases.split(","):
        grids = case.split("+")
        b = pkg.synthetic.make_batch(grids, a.graphs, seed=1, stats=pkg.synthetic.make_batch(grids, a.stats_graphs, seed=0)["stats"])
        d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items() if k != "stats"}
        stats = tuple(s.to(dev) for s in b["stats"])
        ptr = b["graph_ptr"]
        sizes = (ptr[1:] - ptr[:-1])
        bound = int(sizes.max())
        entry = est.wls_estimate if bound <= est.max_nodes_per_graph() else est.wls_estimate_large
        N = b["x"].shape[0]
        # the host split: per bus count the graphs, their rows and branches, and the renumbering of the rows
        groups = []
        src = b["edge_index"][0]
        graph_of_row = torch.repeat_interleave(torch.arange(a.graphs), sizes)
        for n in sorted(set(sizes.tolist())):
            which = torch.nonzero(sizes == n).flatten()
            rows = torch.nonzero(sizes[graph_of_row] == n).flatten()
            erows = torch.nonzero(sizes[graph_of_row[src]] == n).flatten()
            remap = torch.full((N,), -1, dtype=torch.int64)
            remap[rows] = torch.arange(rows.numel())
            groups.append(dict(n=n, which=which.to(dev), rows=rows.to(dev), erows=erows.to(dev), remap=remap.to(dev)))

        def gather(g):
            ei = g["remap"][d["edge_index"].index_select(1, g["erows"])]
            return d["x"].index_select(0, g["rows"]), ei, d["edge_attr"].index_select(0, g["erows"])

        def solve_parts(parts):
            state = torch.empty(N, 2, dtype=torch.float32, device=dev)
            per_graph = None
            for g, (x, ei, ea) in zip(groups, parts):
                res = entry(x, ei, ea, *stats, g["n"], **kw)
                state.index_copy_(0, g["rows"], res.state)
                if per_graph is None:
                    per_graph = [torch.empty((a.graphs,) + t.shape[1:], dtype=t.dtype, device=dev) for t in res[1:]]
                for out, t in zip(per_graph, res[1:]):
                    out.index_copy_(0, g["which"], t)
            return (state, *per_graph)

        cached = [gather(g) for g in groups]
        for g, (x, ei, ea) in zip(groups, cached):
            entry(x, ei, ea, *stats, g["n"], **kw)              # (their structure is attached to these very tensors from here on)
        arms = {"one_launch": lambda: entry(d["x"], d["edge_index"], d["edge_attr"], *stats, bound, graph_ptr=d["graph_ptr"], **kw),
                "split": lambda: solve_parts([gather(g) for g in groups]),
                "split_solves_only": lambda: solve_parts(cached)}
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.runs):
            for k, fn in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1))
        med = {k: statistics.median(v) for k, v in times.items()}
        one, split = arms["one_launch"](), arms["split"]()
        line = {"case": case, "graphs": a.graphs, "stats_graphs": a.stats_graphs, "composition": {str(g["n"]): int(g["which"].numel()) for g in groups}, "bound": bound,
                "kernel": "lds" if entry is est.wls_estimate else "blocked", "max_iter": 8, "device": torch.cuda.get_device_name(0),
                "runs": a.runs, "warmup": a.warmup, "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                "one_launch_over_split": med["one_launch"] / med["split"],
                "one_launch_over_split_solves_only": med["one_launch"] / med["split_solves_only"],
                "one_launch_equals_split_bitwise": all(torch.equal(p, q) for p, q in zip(one, split)),
                "status_counts": {str(s): int((one.status == s).sum()) for s in (0, 1, 2)}}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
