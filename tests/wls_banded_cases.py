"""Batches, orderings and bounds for the banded WLS estimator (estimator.band_order, estimator.wls_estimate_banded,
csrc/dss2_wls_banded.hpp), shared by tests/test_wls_banded_cpu.py and tests/test_gpu_wls_banded.py.

  n257        tests/wls_large_cases.py's tree (chain, its seven laterals) at 257 buses, the first size the dense blocked kernel refuses; 2 graphs
  n320        the same style at 320 buses (one more lateral, {300: 200}); 2 graphs
  radial300   synthetic.register_radial(300): the project's random feeder, 2-hop bandwidth 34 buses, hb = 69 states; 2 graphs
  relabelled257   n257 with its buses renumbered at random (a fixed draw): the numbering a caller may arrive with
  star41      a hub with 40 leaves: every bus is within two branches of every other, hb = 81 = dense; 2 graphs
  path12      a chain of 12 buses: 2-hop bandwidth 2
  guard41     a chain of 41, the star of 41 in the caller's numbering (hub 0: its last leaf's rows reach column 0 from block row 5), a
              chain of 41: the batch whose middle graph does not fit a band of four blocks
  ober70      ONE graph of ober_sub (70 buses), the band-edge case
  mixed8      synthetic.make_batch(["cigre14", "cigre14_reswitched"], 8): two topologies in one batch
and every name of tests/wls_large_cases.py (n100, ober179, cap, cigre14, ober_sub, ...).

Bounds are the project's: the state within wls_large_cases.state_bound(spread), spread = the worst, over four random summation orders
of the ORACLE, of |fp32(oracle state) - permuted-order state|; the objective within 1e-6 relative; iterations and statuses equal.
"""
import functools

import numpy as np
import torch

import wls_cases as wc
import wls_edge_cases as we
import wls_large_cases as lc
import wls_oracle as wo

OBJ_BOUND = 1e-6
_MORE = {110: 3, 150: 100}
TREES = {"n257": lc._shape(257, _MORE), "n320": lc._shape(320, {**_MORE, 300: 200})}
_STAR41 = dict(shape=(41, [((0, k) if k % 2 else (k, 0)) for k in range(1, 41)], [0, 7, 20]), v_at=(0, 13, 40))
_PATH12 = dict(shape=(12, [(k - 1, k) for k in range(1, 12)], [0, 5]), v_at=(0, 11))
_PATH41 = dict(shape=(41, [(k - 1, k) for k in range(1, 41)], [0, 9, 30]), v_at=(0, 20, 40))
SHAPES = dict(TREES, star41=_STAR41, path12=_PATH12, path41=_PATH41)
SEEDS = (1, 2, 3, 4)


def load_pkg():
    from conftest import load_pkg as lp
    return lp()


def relabel(b, new_of_old):
    """The batch with global bus i renamed new_of_old[i]: rows of x and y move, edge endpoints are renamed, edge_attr stays."""
    new_of_old = torch.as_tensor(new_of_old, dtype=torch.long)
    old_of_new = torch.empty_like(new_of_old)
    old_of_new[new_of_old] = torch.arange(new_of_old.numel())
    return dict(b, x=b["x"][old_of_new].contiguous(), y=b["y"][old_of_new].contiguous(), edge_index=new_of_old[b["edge_index"]].contiguous())


@functools.lru_cache(maxsize=None)
def batch(name):
    if name in SHAPES:
        kw = SHAPES[name]
        return wc.collate([wc.graph(name, k, **kw) for k in (0, 1)], kw["shape"][0])
    if name == "guard41":
        return wc.collate([wc.graph("path41", 0, **_PATH41), wc.graph("star41", 0, **_STAR41), wc.graph("path41", 1, **_PATH41)], 41)
    if name == "radial300":
        syn = load_pkg().synthetic
        b = syn.make_batch([syn.register_radial(300)], 2, seed=0)
        b["nodes_per_graph"] = 300
        return b
    if name == "ober70":
        b = load_pkg().synthetic.make_batch(["ober_sub"], 1, seed=2)
        b["nodes_per_graph"] = 70
        return b
    if name == "mixed8":
        b = load_pkg().synthetic.make_batch(["cigre14", "cigre14_reswitched"], 8, seed=13)
        b["nodes_per_graph"] = 15
        return b
    if name == "relabelled257":
        b = batch("n257")
        rng = np.random.default_rng(257)
        return relabel(b, np.concatenate([g * 257 + rng.permutation(257) for g in range(2)]))
    return lc.batch(name)


@functools.lru_cache(maxsize=None)
def oracle(name, max_iter, tol, perm_seed=None):
    """tests/wls_oracle.py's dense solve of a batch: computed once, shared, never modified."""
    return wo.solve(*we.args(batch(name)), max_iter=max_iter, tol=tol, perm_seed=perm_seed)


@functools.lru_cache(maxsize=None)
def spread(name, max_iter, tol):
    ref = oracle(name, max_iter, tol)
    return max((ref["state"].float().double() - oracle(name, max_iter, tol, s)["state"]).abs().max().item() for s in SEEDS)


def bound(name, max_iter, tol):
    return lc.state_bound(spread(name, max_iter, tol))


def brute_force_half_bandwidth(edge_index, n, num_nodes):
    """max (r - c) over the non-zeros of the 2-hop pattern in states, from a dense adjacency matrix per graph."""
    ei = edge_index.cpu().numpy()
    hb = 0
    for g in range(num_nodes // n):
        A = np.eye(n, dtype=np.int64)
        sel = (ei[0] >= g * n) & (ei[0] < (g + 1) * n)
        A[ei[0, sel] - g * n, ei[1, sel] - g * n] = 1
        A[ei[1, sel] - g * n, ei[0, sel] - g * n] = 1
        i, j = np.nonzero(A @ A)
        hb = max(hb, 2 * int((i - j).max()) + 1)
    return hb
