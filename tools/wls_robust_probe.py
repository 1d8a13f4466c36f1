"""Times estimator.wls_robust (csrc/dss2_wls_robust.hip: the Huber M-estimator on the WLS kernels) against the plain estimator on the GPU.

The protocol of tools/wls_probe.py -- device events around each call, max_iter = 8 and tol = 0 so that every graph runs all eight
iterations -- at B = 1024 on cigre14 and ober_sub (the LDS kernel: wls_estimate) and on ober179 (the blocked kernel: wls_estimate_large).
The arms -- the plain solve, wls_robust at gamma = 3 with plain_iters = 1, wls_bad_data with max_removals = 1 (graphs of at most 99
buses) and, with --parent-lib, a parent_ twin of each that runs every dss2_wls_* entry and query of a library built from another
commit -- take turns call by call, --runs rounds after --warmup, and the medians are compared: other work shares the machine, and an
arm measured alone in its own block would carry that block's weather.  Also recorded: whether gamma = inf reproduces the plain
result to the bit, per arm whether the parent library's result equals this one's in every field bit for bit, and how many
measurements the clean batch has down-weighted at the end.  With --parent-lib at a COPY of this build both arms of a pair are the
same code: |ratio - 1| is then the noise of the comparison.  One JSON line per case, appended to --out.  No CPU fallback.

    python tools/wls_robust_probe.py [--runs 20] [--warmup 5] [--cases cigre14:1024,ober_sub:1024,ober179:1024] [--parent-lib libdss2_hip.so]
                                     [--out profiles/wls_robust_probe.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wls_probe import pkg  # noqa: E402

BAD_DATA_MAX_BUSES = 99          # wls_bad_data inverts the gain matrix in LDS


def _parent_names(lib):
    """Every entry and query of the classical estimator (not the training loss's dss2_wls_loss_*), and the error text that goes with them."""
    return tuple(k for k in lib._SIGNATURES if k.startswith("dss2_wls_") and not k.startswith("dss2_wls_loss_")) + ("dss2_last_error",)


class _WithParent:
    """The loaded library with the estimator's entries and queries taken from another build."""

    def __init__(self, real, path):
        self._real, self._parent, self._names = real, C.CDLL(path), _parent_names(pkg._lib)
        for name in self._names:
            fn = getattr(self._parent, name)
            fn.restype, fn.argtypes = pkg._lib._SIGNATURES[name]

    def __getattr__(self, name):
        return getattr(self._parent if name in self._names else self._real, name)


def _same_bits(p, q):
    """Every field of two results equal bit for bit (a NaN equals the same NaN)."""
    return len(p) == len(q) and all(s.shape == t.shape and s.dtype == t.dtype and
                                    torch.equal(s.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)) for s, t in zip(p, q))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="cigre14:1024,ober_sub:1024,ober179:1024")
    ap.add_argument("--parent-lib", default="", help="libdss2_hip.so of another commit: each arm gets a parent_ twin on its estimator entries")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wls_robust_probe: needs the GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    est, lib = pkg.estimator, pkg._lib
    real = lib.lib()
    swapped = _WithParent(real, a.parent_lib) if a.parent_lib else None
    kw = dict(max_iter=8, tol=0.0)
    for case in a.cases.split(","):
        grid, B = case.split(":")
        B = int(B)
        n = pkg.synthetic.load_grid(grid).n
        b = pkg.synthetic.make_batch([grid], B, seed=1)
        d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items() if k != "stats"}
        stats = tuple(s.to(dev) for s in b["stats"])
        large = n > est.max_nodes_per_graph()
        plain_entry = est.wls_estimate_large if large else est.wls_estimate
        run = lambda entry, **more: entry(d["x"], d["edge_index"], d["edge_attr"], *stats, n, **kw, **more)

        def with_parent(fn):
            def call():
                lib._lib = swapped
                try:
                    return fn()
                finally:
                    lib._lib = real
            return call

        arms = {"plain": lambda: run(plain_entry), "robust": lambda: run(est.wls_robust, gamma=3.0, plain_iters=1)}
        if n <= BAD_DATA_MAX_BUSES:
            arms["bad_data"] = lambda: run(est.wls_bad_data, max_removals=1)
        if swapped is not None:
            arms.update({"parent_" + k: with_parent(fn) for k, fn in list(arms.items())})
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
        line = {"case": grid, "graphs": B, "buses_per_graph": n, "kernel": "blocked" if large else "lds", "max_iter": 8, "gamma": 3.0, "plain_iters": 1,
                "device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup,
                "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                "robust_over_plain": med["robust"] / med["plain"]}
        plain, robust = run(plain_entry), run(est.wls_robust, gamma=3.0, plain_iters=1)
        anchor = run(est.wls_robust, gamma=float("inf"))
        line["gamma_inf_equals_plain_bitwise"] = all(torch.equal(p, q) for p, q in zip(plain, anchor[:5]))
        line["downweighted_on_clean_data"] = int(robust.n_downweighted.sum())
        line["state_robust_minus_plain_max"] = (robust.state - plain.state).abs().max().item()
        if swapped is not None:
            line["parent_lib"] = os.path.basename(a.parent_lib)
            line["robust_over_parent_plain"] = med["robust"] / med["parent_plain"]
            for k in [k for k in arms if not k.startswith("parent_")]:
                line[f"{k}_over_parent_{k}"] = med[k] / med["parent_" + k]
                line[f"parent_{k}_equals_{k}_bitwise"] = _same_bits(arms[k](), arms["parent_" + k]())
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
