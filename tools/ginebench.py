#!/usr/bin/env python3
"""Times the GIN model on the reference driver's line (dss2_run.py:86 with GINE_DSSE(8, 32, 2, num_layers=8, edge_dim=6),
gsp_wls_edge, backward, Adamax lr 3e-3) on one GPU, three ways per configuration, and GAT_DSSE (the driver's default) the same way
in the same run, for a same-box comparison:

    eager   runner.train_epoch on one resident batch (Python + autograd around every launch)
    graph   runner.GraphedTrainer: the step captured once into a hipGraph, replayed on copied inputs
    plan    runner.EpochTrainer(mode="plan"): an epoch of replays of one recorded step (collation first, optimizer last); time per step

and reports the launches of one step: the model's forward and backward (counted by recording them into a launch plan) and the whole
recorded training step of the EpochTrainer.  GINE lines also carry the algorithmic bytes of one forward + backward
(algo_bytes_step: every array a pass reads or writes counted once per pass, the per-edge gathers of h and dz once per edge; the loss
and the optimizer are not included).  One JSON line per model and configuration.

    python tools/ginebench.py [--configs cigre14:64,cigre14:4096,ober_sub:1024] [--steps 50] [--warmup 10] [--models GINE_DSSE,GAT_DSSE]

``GAT_DSSE:H`` in --models is the driver's GAT model with H attention heads (their mean, as runner.build_model builds it).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("deep-statistical-solver-for-distribution-system-state-estimation_amd")
REG = pkg.runner.REG_COEFS
DEV = "cuda:0"


def timed(fn, steps, warmup, repeats=5):
    """Median over `repeats` of (elapsed / steps) in ms, by device events around `steps` calls."""
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


def count_launches(fn):
    L = pkg._lib
    h = C.c_void_p()
    L.check(L.lib().dss2_plan_begin(C.byref(h)), "dss2_plan_begin")
    try:
        r = fn()
    finally:
        L.check(L.lib().dss2_plan_end(h), "dss2_plan_end")
    n = int(L.lib().dss2_plan_size(h))
    L.lib().dss2_plan_destroy(h)
    return n, r


def describe(name):
    """The constructor call runner.build_model makes for a --models entry."""
    base, _, kind = name.partition(":")
    if base == "GAT_DSSE" and kind:          # GAT_DSSE:4 -- four heads, averaged (runner.build_model passes concat=False)
        return f"GAT_DSSE(8, 32, 2, 8, 6, heads={int(kind)}, concat={int(kind) == 1})"
    if base in ("GINE_DSSE", "GAT_DSSE"):
        return f"{base}(8, 32, 2, 8, 6)"
    if base == "gnn_dsse":
        return f"gnn_dsse(8, 32, 2, 8, K=2, model='{kind or 'gcn2'}', cached=False)"
    return base


def model_and_opt(name, capturable, seed=0):
    torch.manual_seed(seed)
    base, _, kind = name.partition(":")       # gnn_dsse:gcn2 / gnn_dsse:fagcn / gnn_dsse:tagcn; GAT_DSSE:<heads>
    if base == "GAT_DSSE":
        m = pkg.runner.build_model(base, {**pkg.runner.HYPER, "heads": int(kind or 1)}).to(DEV)
    else:
        m = pkg.runner.build_model(base, pkg.runner.HYPER, gnn_model=kind or "gcn2").to(DEV)
    return m, pkg.FusedAdamax(m.parameters(), lr=3e-3, capturable=capturable)


def gine_algo_bytes(N, E, C=8, ed=6, dense=32, nout=2, n_convs=7):
    """fp32 / int32 bytes one GINE_DSSE forward + backward moves at the algorithmic minimum of the fused route."""
    csr = 2 * E                                                               # col + edge id per CSR entry
    fwd = n_convs * (N * C + E * C + E * ed + csr + 2 * N * C) + N * dense + N * nout          # h, h_j gathers, ea, CSR, y + z
    bwd = n_convs * (2 * N * C + E * C + E * ed + csr + 2 * N * C + N * C)                    # h + dz, dz_i gathers, ea, CSR, y + z, dz
    bwd += N * nout + N * dense + N * C + (N * dense + N * C) + (N * nout + N * dense)        # head backward, its weight gradients
    return 4 * (fwd + bwd)


def bench(name, grid, B, steps, warmup):
    full = pkg.synthetic.make_batch([grid], B, seed=7)
    st = tuple(s.to(DEV) for s in full["stats"])
    x, ei, ea = full["x"].to(DEV), full["edge_index"].to(DEV), full["edge_attr"].to(DEV)
    batch = {"x": x, "edge_index": ei, "edge_attr": ea, "num_graphs": B}
    res = {"model": name, "config": f"{grid} B={B}", "nodes": int(x.size(0)), "edges": int(ei.size(1))}
    if name == "GINE_DSSE":
        res["algo_bytes_step"] = gine_algo_bytes(int(x.size(0)), int(ei.size(1)))

    m, o = model_and_opt(name, False)
    res["eager_ms"] = timed(lambda: pkg.runner.train_epoch(m, o, [batch], st, REG), steps, warmup)
    out = pkg.runner.run_model(m, x[:, :8], ei, ea[:, :6])
    g = torch.ones_like(out)
    out.backward(g)
    torch.cuda.synchronize()
    res["launches_forward"], out = count_launches(lambda: pkg.runner.run_model(m, x[:, :8], ei, ea[:, :6]))
    res["launches_backward"], _ = count_launches(lambda: out.backward(g))

    m, o = model_and_opt(name, True)
    tr = pkg.runner.GraphedTrainer(m, o, st, REG)
    tr.step(x, ei, ea)
    res["graph_ms"] = timed(lambda: tr.step(x, ei, ea), steps, warmup)

    ds = pkg.dataset.DeviceDataset.from_batch(full, device=DEV)
    m, o = model_and_opt(name, True)
    et = pkg.runner.EpochTrainer(m, o, st, REG, ds, B, shuffle=False, mode="plan")
    res["plan_ms"] = timed(lambda: et.steps[B][0].replay(), steps, warmup)     # (the device cursor wraps at the epoch's end)
    res["launches_plan_step"] = int(et.steps[B][0].n_launches)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="cigre14:64,cigre14:4096,ober_sub:1024")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--models", default="GINE_DSSE,GAT_DSSE")
    a = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "models": ", ".join(describe(m) for m in a.models.split(",")),
                      "steps": a.steps, "warmup": a.warmup, "repeats": 5, "statistic": "median of per-step means"}), flush=True)
    for cfg in a.configs.split(","):
        grid, B = cfg.split(":")
        for name in a.models.split(","):
            print(json.dumps(bench(name, grid, int(B), a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
