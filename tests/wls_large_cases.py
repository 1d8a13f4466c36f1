"""Batches for the large-graph WLS estimator (estimator.wls_estimate_large, csrc/dss2_wls_large.hip), shared by
tests/test_wls_large_cpu.py (which measures the bounds in the fp64 oracle) and tests/test_gpu_wls_large.py.

Radial trees out of tests/wls_cases.py's generator (`graph(..., shape=...)`, 3 kV level) with tests/wls_edge_cases.py's `_tree`: a chain
with the laterals {18: 1, 40: 5, 52: 30, 60: 44, 90: 70}, flows measured on every sixth branch, V at buses 0, n // 2 and n - 1; three
graphs per batch, every one converging in the oracle in 4 iterations from a flat start:
  n100     the first size the LDS kernel refuses: 200 states, not a multiple of 16 or 32
  n128     256 states, a multiple of every block size (one more lateral, {110: 3})
  n179t    358 states, ober179's size as a tree (and {150: 100})
  cap      ONE graph of CAP = 256 buses, the largest the kernel serves: 512 states, 513 rows with the right-hand side
and `ober179`: synthetic.make_batch(["ober179"], 3, seed=0), the project's own large grid (gain matrix of condition number 2.4e13).
"""
import functools

import wls_cases as wc
import wls_edge_cases as we
import wls_oracle as wo

CAP = 256
_LATERALS = {18: 1, 40: 5, 52: 30, 60: 44, 90: 70}


def _shape(n, more=()):
    lat = dict(_LATERALS)
    lat.update(more)
    return dict(shape=(n, we._tree(n, lat), list(range(0, n - 1, 6))), v_at=(0, n // 2, n - 1))


TREES = {"n100": _shape(100), "n128": _shape(128, {110: 3}), "n179t": _shape(179, {110: 3, 150: 100}),
         "cap": _shape(CAP, {110: 3, 150: 100})}
GRAPHS = {"n100": (0, 1, 2), "n128": (0, 1, 2), "n179t": (0, 1, 2), "cap": (0,)}
SIZES = ["n100", "n128", "n179t"]
ALL = SIZES + ["ober179", "cap"]


@functools.lru_cache(maxsize=None)
def batch(name):
    """The host batch of a case of this module, or of wls_cases (any of its names)."""
    if name in TREES:
        return wc.collate([wc.graph(name, k, **TREES[name]) for k in GRAPHS[name]], TREES[name]["shape"][0])
    if name == "ober179":
        from conftest import load_pkg
        b = load_pkg().synthetic.make_batch(["ober179"], 3, seed=0)
        b["nodes_per_graph"] = 179
        return b
    return wc.any_batch(name)


@functools.lru_cache(maxsize=None)
def oracle(name, max_iter, tol, perm_seed=None):
    """tests/wls_oracle.py's solve of a batch: computed once, shared, never modified."""
    return wo.solve(*we.args(batch(name)), max_iter=max_iter, tol=tol, perm_seed=perm_seed)


def state_bound(spread):
    """The state bound from the oracle's spread over summation orders: the project's margin of 8 (tests/test_gpu_wls_solve.py), and
    never below the 5e-7 every other WLS test uses."""
    return max(5e-7, 8.0 * spread)
