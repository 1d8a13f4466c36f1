#!/usr/bin/env python3
"""Times one training step of MultiConvNet (forward, the backward of a fixed output gradient, fused Adamax) on the 64 real CIGRE-14
graphs of tests/golden/case_multiconv_real64.npz (dim_hid 32, 3 layers, K = 2), three ways: eager, replayed from a launch plan
(graphs.PlannedStep) and replayed from a hipGraph (graphs.GraphedStep).  Median over 5 repeats of (device-event time of `steps`
calls) / steps.  One JSON line.

    python tools/multiconvbench.py [--steps 200] [--warmup 20] [--dropout 0.0]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("deep-statistical-solver-for-distribution-system-state-estimation_amd")
import cheb_oracle as cor  # noqa: E402
DEV = "cuda:0"


def timed(fn, steps, warmup, repeats=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out)


def make(p):
    t, sd, grads, keys, args = cor.load_golden("multiconv_real64")
    net = pkg.MultiConvNet(*args[:-1], p).to(DEV)
    net.load_state_dict({k: v.float() for k, v in sd.items()})
    data = types.SimpleNamespace(x=t["x"].float().to(DEV), edge_index=t["edge_index"].to(DEV), edge_attr=t["edge_attr"].float().to(DEV))
    gout = t["gout"].float().to(DEV)
    params = list(net.parameters())
    opt = pkg.optim.FusedAdamax(params, lr=3e-3, capturable=True)

    def step():
        for q in params:
            q.grad = None
        out = net(data)
        out.backward(gout)
        opt.step()
        return out
    return step, data, args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dropout", type=float, default=0.0)
    a = ap.parse_args()
    step, data, args = make(a.dropout)
    eager = timed(step, a.steps, a.warmup)
    step_p, _, _ = make(a.dropout)
    plan = pkg.graphs.PlannedStep(step_p, warmup=2)
    planned = timed(plan.replay, a.steps, a.warmup)
    step_g, _, _ = make(a.dropout)
    graph = pkg.graphs.GraphedStep(step_g, warmup=2)
    graphed = timed(graph.replay, a.steps, a.warmup)
    print(json.dumps({"model": "MultiConvNet", "args": list(args[:-1]) + [a.dropout], "batch": "cigre14_real64 (64 graphs)",
                      "nodes": int(data.x.size(0)), "edges": int(data.edge_index.size(1)), "launches_per_step": plan.n_launches,
                      "eager_ms": round(eager, 4), "plan_replay_ms": round(planned, 4), "graph_replay_ms": round(graphed, 4),
                      "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
