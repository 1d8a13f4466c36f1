"""The build's own runner for the hot path: what /root/reference/dss2_run.py does around it.

Reproduces the training loop (dss2_run.py:131-147) and the per-epoch evaluation
(dss2_run.py:165-224) with the reference's knobs as arguments and its defaults:
feature slicing ``x[:, :8] / edge_attr[:, :6] / x[:, 8:] / edge_attr[:, 6:]`` (:138,140),
``reg_coefs`` (:104-112), Adamax lr 3e-3 (:91-92), batch_size 64, the hyper-parameter dict (:72-82).
The model: the driver's default ``GAT_DSSE`` (:85-86, ``--model GAT_DSSE``), the GIN model ``GINE_DSSE`` (same line, ``--model GINE_DSSE``) or the MPN / SkipMPN / PFN / SkipPFN line (:88).
Data: either a folder in the reference's layout (``--data-folder``: ``dataset.data_from_pickles`` ->
shuffle -> 0.9 split -> ``dataset.DataLoader``, dss2_run.py:56-69, measurement model / z-score / collation
on the device) or synthetic batches from ``synthetic.make_batch`` (same layout), collated once and kept
resident on the GPU (re-used tensors take the no-sync topology fast path).

    python tools/train.py --case cigre14 --model SkipPFN --epochs 5
    python tools/train.py --data-folder /path/to/data/cigre14/ --model SkipPFN --epochs 5
"""
from __future__ import annotations

import argparse
import time
from typing import Dict, List, Optional

import torch

from . import data as dss2_data
from . import networks, synthetic
from . import optim as dss2_optim

REG_COEFS = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
OPTIMIZERS = {"Adamax": dss2_optim.FusedAdamax, "Adam": dss2_optim.FusedAdam, "AdamW": dss2_optim.FusedAdamW,
              "RMSprop": dss2_optim.FusedRMSprop, "SGD": dss2_optim.FusedSGD}      # the names of dss2_run.py:91's getattr(optim, NAME)
HYPER = {"dim_nodes": 8, "dim_lines": 6, "dim_out": 2, "dim_hid": 32, "gnn_layers": 8, "K": 2, "dropout_rate": 0.3, "L": 5, "heads": 1}


def build_model(name: str, hp: Dict, gnn_model: str = "gcn2") -> torch.nn.Module:
    cls = getattr(networks, name)
    if name == "gnn_dsse":     # dss2_run.py:86 with the third model family; cached=False so a short last batch works
        return cls(dim_feat=hp["dim_nodes"], dim_dense=hp["dim_hid"], dim_out=hp["dim_out"], num_layers=hp["gnn_layers"],
                   K=hp["K"], model=gnn_model, cached=False)
    if name == "GAT_DSSE":     # dss2_run.py:86; several heads as their mean (concat=False): the only multi-head GAT_DSSE that runs
        return cls(dim_feat=hp["dim_nodes"], dim_dense=hp["dim_hid"], dim_out=hp["dim_out"], heads=hp["heads"],
                   num_layers=hp["gnn_layers"], edge_dim=hp["dim_lines"], concat=(hp["heads"] == 1))
    if name == "GINE_DSSE":    # dss2_run.py:86 with the GIN model (no heads argument)
        return cls(dim_feat=hp["dim_nodes"], dim_dense=hp["dim_hid"], dim_out=hp["dim_out"], num_layers=hp["gnn_layers"],
                   edge_dim=hp["dim_lines"])
    a = (hp["dim_nodes"], hp["dim_lines"], hp["dim_out"], hp["dim_hid"], hp["gnn_layers"], hp["K"], hp["dropout_rate"])
    return cls(*a, hp["L"]) if name in ("PFN", "SkipPFN") else cls(*a)


def run_model(model, x, ei, ea):
    """The model's forward on a batch: gnn_dsse takes (x, edge_index), every other model (x, edge_index, edge_attr)."""
    if isinstance(model, networks.gnn_dsse):
        return model(x, ei)
    return model(x, ei, ea)


def make_loaders(case: str, n_graphs: int, batch_size: int, device, seed: int = 0, split: float = 0.9):
    """Pre-collated, device-resident batches (train / test) with one set of normalisation statistics."""
    full = synthetic.make_batch([case], n_graphs, seed=seed)
    stats = tuple(s.to(device) for s in full["stats"])
    n_train = int(split * n_graphs)

    def batches(g0, g1, seed_off):
        out = []
        for b0 in range(g0, g1, batch_size):
            nb = min(batch_size, g1 - b0)
            b = synthetic.make_batch([case], nb, seed=seed + 1 + seed_off + b0, stats=full["stats"])
            out.append({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in b.items() if k != "stats"})
        return out

    return batches(0, n_train, 0), batches(n_train, n_graphs, 10_000), stats


def _fields(data):
    """A batch is a dict (synthetic loaders) or a dataset.Batch (device loader): (x, edge_index, edge_attr, y, B)."""
    if isinstance(data, dict):
        return data["x"], data["edge_index"], data["edge_attr"], data.get("y"), data["num_graphs"]
    return data.x, data.edge_index, data.edge_attr, data.y, data.num_graphs


def train_epoch(model, opt, loader, stats, reg_coefs, group=None, max_grad_norm=None) -> float:
    """``max_grad_norm``: clip the gradients' global 2-norm between backward and the optimizer step (optim.clip_grad_norm_)."""
    model.train()
    params = list(model.parameters()) if max_grad_norm is not None else None
    total = torch.zeros((), device=stats[0].device)
    for data in loader:                                              # dss2_run.py:134-144
        opt.zero_grad()
        x, ei, ea, _, num_graphs = _fields(data)
        out = run_model(model, x[:, :8], ei, ea[:, :6])
        loss = dss2_data.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=stats[0], x_std=stats[1],
                                      edge_mean=stats[2], edge_std=stats[3], edge_index=ei, reg_coefs=reg_coefs,
                                      num_samples=num_graphs, node_param=x[:, 8:], edge_param=ea[:, 6:], group=group)
        loss.backward(dss2_data.unit_grad(loss))                      # (= loss.backward(), without autograd's ones_like fill kernel)
        if max_grad_norm is not None:
            dss2_optim.clip_grad_norm_(params, max_grad_norm)
        opt.step()
        total += loss.detach()
    return float(total / len(loader))                                # one host sync per epoch (:147)


class GraphedTrainer:
    """The training step of ``train_epoch`` -- zero_grad, forward, gsp_wls_edge, backward, optimizer step -- captured ONCE per
    batch shape into a hipGraph (graphs.GraphedStep) and replayed on static input buffers: at the driver's batch size the eager
    step is host-bound (~2.4 ms of Python / autograd dispatch around 0.33 ms of kernels for the SkipPFN line), the replay is
    not.  Valid when every batch of a shape has the SAME graph structure (one topology per dataset, e.g. the reference's
    cigre14 folder): the structure is part of the captured launches, so only x and edge_attr are copied per step.  In-kernel
    dropout draws new masks on every replay; the optimizer must be a fused one with ``capturable=True`` (``FusedAdamax`` or any other
    class of optim.py).  ``max_grad_norm``: gradient clipping inside the captured step, between backward and the optimizer."""

    def __init__(self, model, opt, stats, reg_coefs, group=None, max_grad_norm=None):
        if not getattr(opt, "capturable", False):
            raise ValueError("GraphedTrainer needs FusedAdamax(capturable=True): the step count must live on the device")
        self.model, self.opt, self.stats, self.reg, self.group = model, opt, stats, reg_coefs, group
        self.max_grad_norm = max_grad_norm
        self.graphs = {}
        self.params = list(model.parameters())

    def _build(self, x, ei, ea):
        from .graphs import GraphedStep
        sx, sea, sei = x.clone(), ea.clone(), ei.clone()
        st, reg, model, opt, params, group = self.stats, self.reg, self.model, self.opt, self.params, self.group
        max_grad_norm = self.max_grad_norm
        eager_losses = []

        def step_fn():
            for p in params:
                p.grad = None
            out = run_model(model, sx[:, :8], sei, sea[:, :6])
            loss = dss2_data.gsp_wls_edge(input=sx[:, :8], edge_input=sea[:, :6], output=out, x_mean=st[0], x_std=st[1],
                                          edge_mean=st[2], edge_std=st[3], edge_index=sei, reg_coefs=reg, num_samples=None,
                                          node_param=sx[:, 8:], edge_param=sea[:, 6:], group=group)
            loss.backward(dss2_data.unit_grad(loss))
            if max_grad_norm is not None:
                dss2_optim.clip_grad_norm_(params, max_grad_norm)
            opt.step()
            if not torch.cuda.is_current_stream_capturing():
                eager_losses.append(loss.detach().clone())
            return loss
        # the warm-up step of the capture is a REAL training step on this batch (it advances the weights and the optimizer); the
        # capture runs on the caller's current stream when that is not the default one (the autograd state of earlier eager
        # steps belongs to it), else on a stream of its own
        cur = torch.cuda.current_stream()
        g = GraphedStep(step_fn, warmup=1, capture_error_mode=("thread_local" if group is not None else "global"),
                        stream=(cur if cur != torch.cuda.default_stream() else None))
        return g, sx, sea, eager_losses[-1]

    def step(self, x, ei, ea) -> torch.Tensor:
        key = (tuple(x.shape), tuple(ea.shape), tuple(ei.shape))
        hit = self.graphs.get(key)
        if hit is None:
            g, sx, sea, first_loss = self._build(x, ei, ea)
            self.graphs[key] = (g, sx, sea)
            return first_loss           # (the capture's warm-up step has trained on this batch)
        g, sx, sea = hit
        sx.copy_(x)
        sea.copy_(ea)
        return g.replay().detach()


def train_epoch_graphed(trainer: GraphedTrainer, loader) -> float:
    total = torch.zeros((), device=trainer.stats[0].device)
    for data in loader:
        x, ei, ea, _, _ = _fields(data)
        total += trainer.step(x, ei, ea)
    return float(total / len(loader))


class EpochTrainer:
    """The training loop of dss2_run.py:131-147 -- ``for data in loader: zero_grad; forward; gsp_wls_edge; backward; step`` -- with NO host
    work per batch beyond one C call: the loader's collation writes straight into the step's static input buffers as the FIRST launch of
    the recorded step (``dss2_collate_cursor``: the batch's position in the epoch's sample permutation lives on the device and is moved
    forward by the launch behind the gather), the optimizer step and the running loss sum (``dss2_accum_scalar``) are its last ones.  An
    epoch is ``len(dataset) // batch_size`` replays of one recorded step (+ one replay of a second, smaller step for the last
    batch, ``drop_last=False`` as torch_geometric's loader at dss2_run.py:68-69); the only per-epoch host work is drawing the
    permutation (on the device) and resetting two words.  Nothing is read back until the caller asks for the epoch's mean loss.

    ``mode``: "plan" (graphs.PlannedStep: the library's own launch list, one ``dss2_plan_run`` per step; also at world > 1, where the
    step's collectives cut it into segments) or "graph" (graphs.GraphedStep: a hipGraph).  Needs ``FusedAdamax(capturable=True)`` (or
    another fused optimizer of optim.py, capturable; ``max_grad_norm`` puts optim.clip_grad_norm_ between backward and its step) and
    either a single-topology ``DeviceDataset`` (the graph structure is then built once, outside the step) or a
    ``dataset.PaddedMixedDataset`` (``MixedDataset.padded()``: samples of several topologies on one bus count, BASELINE config C5 --
    the collation also gathers every slot's edge list and edge count, and the step's second entry is ``Topology.rebuild()``: the
    structure of THIS batch, built on the device inside the step; the loss divides by the batch's real edge count, read on the
    device.  The permutation runs over the union of the parts, the reference loader's uniform shuffle.  Models: MPN, SkipMPN, PFN,
    SkipPFN).  Recording a step runs it (plans:
    three times, graphs: once), so the model, the optimizer state (every state tensor, the step counts, a tensor ``lr``) and the epoch
    position are saved before and restored after: the first
    ``train_epoch()`` starts from exactly the state the trainer was given."""

    def __init__(self, model, opt, stats, reg_coefs, dataset, batch_size: int, shuffle: bool = True, mode: str = "plan", group=None,
                 generator=None, max_grad_norm=None):
        from . import _lib
        from . import dataset as dss2_dataset
        self.padded = isinstance(dataset, dss2_dataset.PaddedMixedDataset)
        if not isinstance(dataset, dss2_dataset.DeviceDataset) or not (dataset.shared_topology or self.padded):
            raise ValueError("EpochTrainer needs a single-topology DeviceDataset (per-batch structures: DataLoader / PrefetchLoader + train_epoch)")
        if self.padded and type(model) not in (networks.MPN, networks.SkipMPN, networks.PFN, networks.SkipPFN):
            # (the lane-group models -- GAT_DSSE, GINE_DSSE, gnn_dsse -- and the Multi* variants build structures of their own kind from
            #  edge_index (as given / without flip flags / with self loops), which would list the padding edges as branches)
            raise ValueError(f"EpochTrainer on a padded mixed store supports MPN, SkipMPN, PFN and SkipPFN, not {type(model).__name__}: "
                             "its graph structure is not rebuilt from the per-slot edge counts")
        if not getattr(opt, "capturable", False):
            raise ValueError("EpochTrainer needs FusedAdamax(capturable=True): the step count must live on the device")
        if mode not in ("plan", "graph"):
            raise ValueError("mode: 'plan' or 'graph'")
        self._lib = _lib
        self.model, self.opt, self.stats, self.reg, self.group = model, opt, stats, reg_coefs, group
        self.ds, self.B, self.shuffle, self.mode, self.generator = dataset, int(batch_size), bool(shuffle), mode, generator
        self.max_grad_norm = max_grad_norm
        self.params = list(model.parameters())
        dev = dataset.device
        n = len(dataset)
        if n < 1 or self.B < 1:
            raise ValueError("empty dataset / batch")
        self.n_full, self.rem = divmod(n, self.B)
        self.base_ids = dataset.ids.contiguous()
        self.ids = self.base_ids.clone()                                   # this epoch's order (static: the recorded steps read it)
        self.cursor = torch.tensor([0, n], dtype=torch.int64, device=dev)  # {position, epoch length}
        self._cursor0 = self.cursor.clone()
        self.acc = torch.zeros(2, dtype=torch.float64, device=dev)         # {sum of the step losses, steps}
        self.steps = {}
        opt.init_state()
        saved = self._snapshot()
        for nb in ([self.B] if self.n_full else []) + ([self.rem] if self.rem else []):
            self.steps[nb] = self._record(nb)
        self._restore(saved)

    # ---- state that recording a step consumes
    def _state_tensors(self):
        ts = list(self.params)
        seen = set()

        def add(v):      # (the parameters of a group share one step tensor: once)
            if torch.is_tensor(v) and id(v) not in seen:
                seen.add(id(v))
                ts.append(v)
        for g in self.opt.param_groups:
            add(g.get("_step"))
            add(g.get("lr"))
            for p in g["params"]:
                for v in self.opt.state.get(p, {}).values():
                    add(v)
        return ts

    def _snapshot(self):
        return [t.detach().clone() for t in self._state_tensors()]

    @torch.no_grad()
    def _restore(self, saved):
        for t, s in zip(self._state_tensors(), saved):
            t.copy_(s)
        self.cursor.copy_(self._cursor0)
        self.acc.zero_()

    def _record(self, nb: int):
        from . import graphs
        ds, st, reg, model, opt, params, group = self.ds, self.stats, self.reg, self.model, self.opt, self.params, self.group
        dev = ds.device
        sx = torch.empty(nb * ds.n, ds.x.size(2), dtype=torch.float32, device=dev)
        sea = torch.empty(nb * ds.e, ds.edge_attr.size(2), dtype=torch.float32, device=dev)
        ids, cursor, acc, L, max_grad_norm = self.ids, self.cursor, self.acc, self._lib, self.max_grad_norm
        if self.padded:
            # static edge lists and per-slot edge counts, gathered with the features; the structure follows them inside the step
            ei = torch.empty(2, nb * ds.e, dtype=torch.int64, device=dev)
            cnt = torch.empty(nb, dtype=torch.int32, device=dev)
            descs = ds.collate_descs(sx, sea, edge_index=ei, e_count=cnt)
            ds.collate_into(descs, ids, nb, cursor=cursor, advance=False)      # (real content for the first build)
            topo = ds.padded_topology(ei, cnt)
        else:
            ei, _ = ds.batch_structure(nb)
            descs = ds.collate_descs(sx, sea)
            topo, cnt = None, None

        def step_fn():
            ds.collate_into(descs, ids, nb, cursor=cursor, advance=True)
            if topo is not None:
                topo.rebuild()
            for p in params:
                p.grad = None
            out = run_model(model, sx[:, :8], ei, sea[:, :6])
            loss = dss2_data.gsp_wls_edge(input=sx[:, :8], edge_input=sea[:, :6], output=out, x_mean=st[0], x_std=st[1],
                                          edge_mean=st[2], edge_std=st[3], edge_index=ei, reg_coefs=reg, num_samples=None,
                                          node_param=sx[:, 8:], edge_param=sea[:, 6:], group=group)
            loss.backward(dss2_data.unit_grad(loss))
            if max_grad_norm is not None:
                dss2_optim.clip_grad_norm_(params, max_grad_norm)
            opt.step()
            L.check(L.lib().dss2_accum_scalar(acc.data_ptr(), loss.data_ptr(), L.stream_ptr(dev)), "dss2_accum_scalar")
            return loss
        cur = torch.cuda.current_stream(dev)
        if self.mode == "plan":
            rec = graphs.PlannedStep(step_fn, stream=cur)
        else:
            rec = graphs.GraphedStep(step_fn, warmup=1, capture_error_mode=("thread_local" if group is not None else "global"),
                                     stream=(cur if cur != torch.cuda.default_stream(dev) else None))
        return rec, sx, sea, descs, ei, cnt, topo

    def train_epoch(self) -> torch.Tensor:
        """One pass over the dataset.  Returns the DEVICE tensor {sum of the step losses, steps} of this epoch (``mean_loss()`` reads
        it: the epoch's single host synchronisation, dss2_run.py:147)."""
        if self.shuffle:
            perm = torch.randperm(self.base_ids.numel(), device=self.base_ids.device, generator=self.generator)
            torch.index_select(self.base_ids, 0, perm, out=self.ids)
        self.cursor.copy_(self._cursor0)
        self.acc.zero_()
        if self.n_full:
            replay = self.steps[self.B][0].replay
            for _ in range(self.n_full):
                replay()
        if self.rem:
            self.steps[self.rem][0].replay()
        return self.acc

    def mean_loss(self) -> float:
        s, k = self.acc.tolist()
        return s / max(k, 1.0)


@torch.no_grad()
def evaluate(model, loader, stats) -> Dict[str, float]:
    """dss2_run.py:165-224: RMSE / MAE of V and theta and of the line / trafo loadings from get_pflow, and the
    std ratios, averaged over the test batches.  The ten per-batch quantities are accumulated on the device
    (``data.eval_batch``); one device-to-host copy per evaluation."""
    model.eval()                                                     # dropout stays active, as in the reference
    acc = torch.zeros(10, dtype=torch.float64, device=stats[0].device)
    n = 0
    for data in loader:
        x, ei, ea, y, _ = _fields(data)
        out = run_model(model, x[:, :8], ei, ea[:, :6])
        dss2_data.eval_batch(out, y, x, ei, ea, stats[0], stats[1], acc)
        n += 1
    vals = (acc / max(n, 1)).cpu().tolist()
    return dict(zip(dss2_data.EVAL_METRICS, vals))


@torch.no_grad()
def evaluate_wls(loader, stats, nodes_per_graph: Optional[int] = None, model=None, bad_data=None, **solver_kw) -> Dict[str, float]:
    """The classical WLS estimator (``estimator.wls_estimate``; ``wls_estimate_large`` above its bus count) over a loader, scored like ``evaluate``: the ten EVAL_METRICS of its
    state, averaged over the batches, plus ``wls_mean_iterations`` (Gauss-Newton updates per graph) and ``wls_not_converged`` (graphs
    that did not end with status 0).  ``model`` None: a flat start, the baseline a learned estimator is compared with; a model: its
    de-normalised output is the start, the hybrid.  ``solver_kw``: max_iter, tol, weights.  ``bad_data`` = dict(threshold=...,
    max_removals=..., [confidence, s_min]): the solve is ``estimator.wls_bad_data`` with these, and the metrics gain ``wls_suspect``
    (graphs that fail the chi-square test after the removals) and ``wls_removed`` (measurements removed).  The dict may also carry
    ``large``, taken off before the call: False or absent -- ``wls_bad_data``, which refuses above ``estimator.max_nodes_per_graph()``
    buses; True -- ``estimator.wls_bad_data_large``, the blocked form, up to ``estimator.max_nodes_per_graph_large()`` buses; "auto" -- chosen
    by the batch's bound as the plain solve is (what ``--wls-bad-data`` passes).  The keyword ``robust`` = dict(gamma=..., [plain_iters]) (taken out of
    ``solver_kw``): the solve is ``estimator.wls_robust`` with these, the Huber M-estimator, for every bus count up to
    ``estimator.max_nodes_per_graph_large()``, and the metrics gain ``wls_downweighted`` (measurements with a weight factor below 1 at the
    solution); not together with ``bad_data``.  A batch that carries a ``graph_ptr`` (a dict key or an attribute: ``synthetic.make_batch``,
    ``dataset.MixedDataset`` on parts of different bus counts) is solved with it and with its ``max_nodes`` -- else ``nodes_per_graph``,
    which may be None where every batch says its own -- as the bound on a graph's bus count: a data list may mix grids.  The kernel
    (LDS or blocked) is chosen by that bound.  One device-to-host copy.
    The keyword ``banded`` (taken out of ``solver_kw`` like ``robust``; default False): True -- the plain solve is ``estimator.wls_estimate_banded`` (no cap of 256 buses; equal-size graphs -- a ``graph_ptr`` that mixes bus counts is
    refused); "auto" -- only above ``estimator.max_nodes_per_graph_large()`` buses; False, the default --
    never: above 256 buses the call is refused as before.  With ``bad_data`` or ``robust``, True and "auto" alike: up to 256 buses their dense
    solves as without it, above 256 ``estimator.wls_bad_data_banded`` / ``estimator.wls_robust_banded`` (``bad_data['large']`` has nothing to choose there).  The banded solve orders each distinct edge list once (``estimator.band_order``
    reads it back: one more copy per structure) and keeps the order for the batches that share the tensor."""
    from . import estimator
    banded = solver_kw.pop("banded", False)
    if not (banded is True or banded is False or banded == "auto"):
        raise ValueError(f"evaluate_wls: banded must be False, True or 'auto', got {banded!r}")
    orders = {}                  # id(edge_index) -> (edge_index, BandOrder): a loader that reuses its structure tensor is ordered once
    robust = solver_kw.pop("robust", None)
    if bad_data is not None and robust is not None:
        raise ValueError("evaluate_wls: bad_data and robust are two answers to gross errors: give one of them")
    bad_large = False
    if bad_data is not None:
        bad_data = dict(bad_data)
        bad_large = bad_data.pop("large", False)
        if not (bad_large is True or bad_large is False or bad_large == "auto"):
            raise ValueError(f"evaluate_wls: bad_data['large'] must be False, True or 'auto', got {bad_large!r}")
    dev = stats[0].device
    acc = torch.zeros(10, dtype=torch.float64, device=dev)
    tally = torch.zeros(5, dtype=torch.float64, device=dev)          # updates, graphs, graphs not converged, suspect graphs, removals (robust: down-weighted measurements)
    n = 0
    if model is not None:
        model.eval()
    for data in loader:
        x, ei, ea, y, _ = _fields(data)
        init = None
        if model is not None:
            out = run_model(model, x[:, :8], ei, ea[:, :6])
            init = torch.stack([out[:, 0] * stats[1][0] + stats[0][0], out[:, 1]], 1)
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        get = data.get if isinstance(data, dict) else lambda k: getattr(data, k, None)
        graph_ptr, bound, kw = get("graph_ptr"), nodes_per_graph, solver_kw
        if graph_ptr is not None:
            kw = dict(solver_kw, graph_ptr=graph_ptr)
            bound = get("max_nodes") or nodes_per_graph
        if bound is None:
            raise ValueError("evaluate_wls: nodes_per_graph is None and the batch carries no graph_ptr with max_nodes")
        beyond = bound > estimator.max_nodes_per_graph_large()
        # (banded=True moves the PLAIN solve onto the band at every bus count; bad_data and robust keep their dense solves up to 256 buses)
        if (banded is True and (beyond or (bad_data is None and robust is None))) or (banded == "auto" and beyond):
            # (a graph_ptr whose graphs all reach the bound describes equal-size graphs: known on the host from the two lengths)
            if graph_ptr is not None and x.size(0) != (graph_ptr.numel() - 1) * bound:
                raise NotImplementedError("evaluate_wls: the banded solve serves equal-size graphs; this batch's graph_ptr mixes bus counts")
            if id(ei) not in orders:
                orders[id(ei)] = (ei, estimator.band_order(ei, bound, num_nodes=x.size(0)))
            band_kw = dict(solver_kw, init=init, order=orders[id(ei)][1])
            suspect, removed = zero, zero
            if robust is not None:
                res = estimator.wls_robust_banded(x, ei, ea, stats[0], stats[1], stats[2], stats[3], bound, **band_kw, **robust)
                removed = res.n_downweighted.sum()
            elif bad_data is not None:       # (`large` chooses between the two dense forms: nothing to choose here)
                res = estimator.wls_bad_data_banded(x, ei, ea, stats[0], stats[1], stats[2], stats[3], bound, **band_kw, **bad_data)
                suspect, removed = res.suspect.sum(), res.n_removed.sum()
            else:
                res = estimator.wls_estimate_banded(x, ei, ea, stats[0], stats[1], stats[2], stats[3], bound, **band_kw)
        elif robust is not None:
            res = estimator.wls_robust(x, ei, ea, stats[0], stats[1], stats[2], stats[3], bound, init=init, **kw, **robust)
            suspect, removed = zero, res.n_downweighted.sum()
        elif bad_data is None:
            solve = estimator.wls_estimate if bound <= estimator.max_nodes_per_graph() else estimator.wls_estimate_large
            res = solve(x, ei, ea, stats[0], stats[1], stats[2], stats[3], bound, init=init, **kw)
            suspect, removed = zero, zero
        else:
            large = bound > estimator.max_nodes_per_graph() if bad_large == "auto" else bad_large
            solve = estimator.wls_bad_data_large if large else estimator.wls_bad_data
            res = solve(x, ei, ea, stats[0], stats[1], stats[2], stats[3], bound, init=init, **kw, **bad_data)
            suspect, removed = res.suspect.sum(), res.n_removed.sum()
        dss2_data._eval_state_batch(res.state, y, x, ei, ea, acc)
        tally += torch.stack([res.iterations.sum(), torch.tensor(res.iterations.numel(), device=dev), (res.status != 0).sum(),
                              suspect, removed]).double()
        n += 1
    vals = (acc / max(n, 1)).cpu().tolist()
    its, graphs, bad, n_suspect, n_removed = tally.cpu().tolist()
    m = dict(zip(dss2_data.EVAL_METRICS, vals))
    m["wls_mean_iterations"] = its / max(graphs, 1.0)
    m["wls_not_converged"] = int(bad)
    if bad_data is not None:
        m["wls_suspect"] = int(n_suspect)
        m["wls_removed"] = int(n_removed)
    if robust is not None:
        m["wls_downweighted"] = int(n_removed)
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="cigre14", help="cigre14, cigre14_reswitched, ober_sub or ober179; or a comma-separated list of cases on one "
                    "bus count (cigre14,cigre14_reswitched: BASELINE config C5), trained as one shuffled data list on a padded store (EpochTrainer)")
    ap.add_argument("--model", default="SkipPFN", choices=["MPN", "SkipMPN", "PFN", "SkipPFN", "GAT_DSSE", "GINE_DSSE"] + ["gnn_dsse"])
    ap.add_argument("--gnn-model", default="gcn2", choices=["gcn2", "fagcn", "tagcn"], help="gnn_dsse's conv kind")
    ap.add_argument("--graphs", type=int, default=720)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=600)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--optimizer", default="Adamax", choices=list(OPTIMIZERS), help="the fused counterpart of torch.optim's class of this name")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the gradients' global 2-norm before every optimizer step")
    hyper_help = {"heads": "GAT_DSSE: attention heads per conv (heads * dim_nodes rounded up to a power of two <= 32: 1 to 4 at 8 "
                           "channels).  Above 1 the model is built with concat=False, the mean over the heads: the only multi-head "
                           "GAT_DSSE the reference can train (its concatenated output fits neither the next conv nor the Linear)"}
    for k, v in HYPER.items():
        ap.add_argument("--" + k.replace("_", "-"), type=type(v), default=v, help=hyper_help.get(k))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default="")
    ap.add_argument("--data-folder", default="", help="folder with the reference's pickles (nodes, edges, labels, noise_param)")
    ap.add_argument("--graph", type=int, default=-1, help="1: replay the training step as a hipGraph (GraphedTrainer; needs ONE graph "
                    "structure per batch shape), 0: eager, -1 (default): graph when the data has a single topology")
    ap.add_argument("--wls-baseline", action="store_true", help="after training, print the evaluation metrics of the classical WLS "
                    "estimator on the test split, from a flat start and from the trained model's output (evaluate_wls); a data list may mix bus counts")
    ap.add_argument("--wls-bad-data", type=float, default=None, metavar="THRESHOLD", help="the --wls-baseline lines (implied) through "
                    "estimator.wls_bad_data (above 99 buses per graph: wls_bad_data_large): up to 5 measurements per graph are removed while the "
                    "largest normalized residual exceeds THRESHOLD")
    ap.add_argument("--wls-robust", type=float, default=None, metavar="GAMMA", help="the --wls-baseline lines (implied) through "
                    "estimator.wls_robust, the Huber M-estimator with threshold GAMMA (3.0 is the usual choice); any bus count up to 256; "
                    "not together with --wls-bad-data")
    ap.add_argument("--wls-banded", action="store_true", help="the --wls-baseline lines (implied) on grids above 256 buses per graph through "
                    "estimator.wls_estimate_banded (the buses are ordered for a small bandwidth once per structure); up to 256 buses as without it.  "
                    "Combines with --wls-bad-data and --wls-robust: above 256 buses through wls_bad_data_banded and wls_robust_banded")
    a = ap.parse_args(argv)
    if a.wls_robust is not None and a.wls_bad_data is not None:
        ap.error("--wls-robust and --wls-bad-data are exclusive")
    hp = {k: getattr(a, k) for k in HYPER}
    if a.model == "SkipMPN":
        hp["dim_out"] = hp["dim_nodes"]
    dev = torch.device("cuda")
    torch.manual_seed(a.seed)
    import numpy as np
    mixed_train = None
    if a.data_folder:                                                # dss2_run.py:47-69
        from . import dataset as dss2_dataset
        cigre = "cigre" in a.data_folder
        meas_v = np.array([0, 1, 12, 7, 11, 14] if cigre else [35, 16, 52, 47, 6, 48, 59, 27, 37, 56])
        meas_pf = np.array([0, 10] if cigre else [40, 43, 11, 21, 54, 57])
        ds, *stats = dss2_dataset.data_from_pickles(a.data_folder, 8, 6, 4, 2, meas_v, meas_pf, device=dev)
        ds = ds.shuffled()
        n_train = int(0.9 * len(ds))
        train_loader = dss2_dataset.DataLoader(ds[0:n_train], batch_size=a.batch_size, shuffle=True)
        test_loader = dss2_dataset.DataLoader(ds[n_train:], batch_size=a.batch_size, shuffle=False)
        stats = tuple(stats)
    elif "," in a.case:                                              # a mixed data list: one padded device store, whole epochs recorded
        from . import dataset as dss2_dataset
        cases = [c.strip() for c in a.case.split(",")]
        full = synthetic.make_batch(cases, min(a.graphs, 256), seed=a.seed)
        stats = tuple(s.to(dev) for s in full["stats"])
        per = -(-a.graphs // len(cases))
        parts = [dss2_dataset.DeviceDataset.from_batch(synthetic.make_batch([c], per, seed=a.seed + 1 + k, stats=full["stats"]), device=dev)
                 for k, c in enumerate(cases)]
        mixed = dss2_dataset.MixedDataset(parts).shuffled(np.random.default_rng(a.seed))
        n_train = int(0.9 * len(mixed))
        mixed_train = mixed[0:n_train]
        train_loader = dss2_dataset.DataLoader(mixed_train, batch_size=a.batch_size, shuffle=True)
        test_loader = dss2_dataset.DataLoader(mixed[n_train:], batch_size=a.batch_size, shuffle=False)
    else:
        train_loader, test_loader, stats = make_loaders(a.case, a.graphs, a.batch_size, dev, a.seed)
    model = build_model(a.model, hp, gnn_model=a.gnn_model).to(dev)
    single_topology = (not a.data_folder and mixed_train is None) or bool(getattr(train_loader.dataset, "shared_topology", False))
    use_graph = (a.graph == 1) or (a.graph == -1 and single_topology and hp["dim_out"] == 2)
    make_opt, clip = OPTIMIZERS[a.optimizer], a.max_grad_norm
    opt = make_opt(model.parameters(), lr=a.lr, capturable=use_graph)
    # a device-resident data folder with ONE graph structure: whole epochs without the interpreter (EpochTrainer: the loader's collation is the
    # first launch of the recorded step); pre-collated synthetic batches: the step replayed on copied inputs (GraphedTrainer); else eager
    epoch_trainer = None
    if mixed_train is not None and a.graph != 0 and mixed_train.n is not None and type(model) in (networks.MPN, networks.PFN, networks.SkipPFN):
        use_graph = True
        opt = make_opt(model.parameters(), lr=a.lr, capturable=True)
        epoch_trainer = EpochTrainer(model, opt, stats, REG_COEFS, mixed_train.padded(), a.batch_size, shuffle=True, mode="graph", max_grad_norm=clip)
    elif mixed_train is not None:
        use_graph = False                                            # (other models / mixed bus counts: the eager loader, a structure per batch)
        opt = make_opt(model.parameters(), lr=a.lr)
    elif use_graph and a.data_folder and single_topology:
        epoch_trainer = EpochTrainer(model, opt, stats, REG_COEFS, train_loader.dataset, a.batch_size, shuffle=True, mode="graph", max_grad_norm=clip)
    trainer = GraphedTrainer(model, opt, stats, REG_COEFS, max_grad_norm=clip) if (use_graph and epoch_trainer is None) else None
    how = "whole epochs as replays of one recorded step (EpochTrainer)" if epoch_trainer is not None else ("hipGraph replay" if use_graph else "eager")
    print(f"device:{dev}  train batches {len(train_loader)}  test batches {len(test_loader)}  model {a.model} {hp}  step: {how}")
    for epoch in range(a.epochs):
        t0 = time.perf_counter()
        if epoch_trainer is not None:
            epoch_trainer.train_epoch()
            tl = epoch_trainer.mean_loss()
        else:
            tl = train_epoch_graphed(trainer, train_loader) if use_graph else train_epoch(model, opt, train_loader, stats, REG_COEFS, max_grad_norm=clip)
        m = evaluate(model, test_loader, stats) if hp["dim_out"] == 2 else {}
        torch.cuda.synchronize()
        print(f"epoch {epoch:4d}  train_loss {tl:.6g}  " + "  ".join(f"{k} {v:.4g}" for k, v in m.items()) +
              f"  ({time.perf_counter() - t0:.2f} s)", flush=True)
    if a.wls_baseline or a.wls_bad_data is not None or a.wls_robust is not None or a.wls_banded:
        ds = getattr(test_loader, "dataset", None)
        n_bus = getattr(ds, "n", None) if ds is not None else synthetic.load_grid(a.case).n
        if n_bus is None:                                            # a data list that mixes bus counts: its batches carry graph_ptr; the bound is the largest part's
            n_bus = max(p.n for p in ds.parts)
        for label, start in [("flat start", None)] + ([(f"start = {a.model}'s output", model)] if hp["dim_out"] == 2 else []):
            bad_data = dict(threshold=a.wls_bad_data, max_removals=5, large="auto") if a.wls_bad_data is not None else None
            robust = dict(gamma=a.wls_robust) if a.wls_robust is not None else None
            m = evaluate_wls(test_loader, stats, n_bus, model=start, bad_data=bad_data, robust=robust, banded="auto" if a.wls_banded else False)
            print(f"wls baseline ({label})  " + "  ".join(f"{k} {v:.4g}" for k, v in m.items()), flush=True)
    if a.save:                                                       # dss2_run.py:240-247
        torch.save({"epoch": a.epochs - 1, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict()},
                   a.save)


if __name__ == "__main__":
    main()
