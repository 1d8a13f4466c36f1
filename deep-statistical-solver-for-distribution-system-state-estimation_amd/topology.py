"""Per-topology graph structure for the HIP kernels, built ON THE DEVICE (``dss2_csr_build`` and friends,
csrc/dss2_topology.hip) once per distinct edge_index and cached.

Replaces, per forward call of the reference: ``MPN.is_directed`` / ``undirect_graph``
(/root/reference/networks.py:236-258: host sync + 3 cats), PyG ``gcn_norm`` (degree, pow,
masked_fill, 2 gathers per TAGConv call) and PyG's per-call scatter index handling.

Two parts, built separately:

* the CSR part (always): CSR by target / by source of the (doubled) directed edge list, incidence CSR of the stored
  edges, int32 endpoints, in-degrees, gcn_norm weights -- all the loss kernels, ``MessagePassing.propagate`` and
  ``segment_sum`` need; asynchronous, any graph size;
* the tile part (lazily, when a tile kernel asks for it): whole-graph tiles of <= 32*nrb rows and the per-tile ELL
  slices the tile kernels stage in LDS.  A connected component above 192 rows has no graph-aligned tiles:
  ``global_only`` is set, the plain GEMMs run on uniform 64-row tiles and the propagation in global memory
  (networks._tagconv_forward_global).

Host synchronisation: none when the caller passes a :class:`TopologyHint` (the device data loader does: it knows
its samples' sizes and degrees); otherwise one 24-byte copy for the cache key + directedness and one 64-byte copy of
the build statistics on a cache miss.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib

_FLIP = 1 << 31
_NRB_CHOICES = (2, 4, 3, 1, 6)   # preference order on utilisation ties (32*nrb rows per tile)
LDS_LIMIT = 160 * 1024
_ELL_MAX = 8


@dataclass(slots=True)
class Tiling:
    """One tile set of a batch: whole-graph tiles of 32 * nrb rows and the per-tile ELL slices the tile kernels stage in LDS.  A
    Topology owns a primary one (``Topology.tiling``) and alternates of a forced height (``Topology.tiles_for``); the CSR arrays
    every tiling indexes stay on the Topology."""
    global_only: bool            # no graph-aligned tiles (a component above 192 rows): uniform 64-row tiles, no ELL slices
    nrb: int
    ntiles: int
    tile_start: torch.Tensor     # int32 [ntiles + 1]
    utilisation: float
    max_segment: int
    max_tile_rows: int           # rows a tile really holds where every graph has the same size, else 0
    max_nnz: int
    max_nnzT: int
    ell: int                     # ELL width by target / by source (0: a row above 8 entries, CSR staging)
    ellT: int
    ell_tiles: Optional[torch.Tensor]          # int32 [ntiles, width, 32 * nrb, 2] (column, weight); None at width 0
    ellT_tiles: Optional[torch.Tensor]
    ell_ent_tiles: Optional[torch.Tensor]      # ... (column, edge entry)
    ellT_ent_tiles: Optional[torch.Tensor]
    gain_bits: Dict[int, int] = field(default_factory=dict)                 # ops._wgrad_mode: nmat -> headroom bits of this tile set


_TILING_FIELDS = frozenset(Tiling.__slots__) - {"gain_bits"}


@dataclass(frozen=True)
class TopologyHint:
    """What a caller that assembled the batch itself knows without looking at the device (dataset.DataLoader does):
    with it the whole structure is built without a single device-to-host copy."""
    directed: bool               # MPN.is_directed of the batch: its first edge has no reverse edge (networks.py:236-238)
    nodes_per_graph: int         # every graph of the batch has this many nodes, in consecutive rows
    max_degree: int              # upper bound of the in- and out-degree on the directed (doubled) list
    max_edges_per_graph: int     # upper bound of the stored edges of one graph
    # round 6: where the graphs' ranges in the stored edge list are known too, the whole CSR part (and the folded-bias row scales) is ONE
    # launch, a wave per graph (dss2_csr_build_graphs): edges_per_graph (every graph has this many, in graph order) or edge_ptr (device int64
    # [G + 1], the batch's own prefix sum of the graphs' edge counts); neither: the general build (global scans)
    edges_per_graph: int = 0
    edge_ptr: Optional[torch.Tensor] = None


# ---- the 16 statistic words of a build (int32, device: include/dss2_hip.h, csrc/dss2_topology.hip:67) ----------------
# name -> index; ``ntiles_cand`` is the first of the 8 words a walk fills, one per candidate height
_WORDS = dict(max_deg=0, max_degT=1, max_segment=2, n_segments=3, min_segment=4, error=5, max_nnz=6, max_nnzT=7, ntiles_cand=8)
_PER_TILING = slice(_WORDS["error"], _WORDS["ntiles_cand"])      # what an ELL launch writes: the error flag and the per-tile entry maxima
_ERRORS = {1: "edge_index holds node ids outside [0, num_nodes)",
           2: "TopologyHint.max_degree is smaller than a row of the batch",
           3: "edge_count holds a value outside [0, edges_per_graph]"}


# ---- tile selection: pure functions (no torch, no library call) -------------------------------------------------------
NNZ_HINT, NNZ_ELL, NNZ_READBACK = "hint", "ell", "readback"      # where a tiling's per-tile entry counts (max_nnz / max_nnzT) come from


class TileSpec(NamedTuple):
    """Everything known about a tiling before any launch.  ``nnz`` names the policy of the per-tile entry counts: NNZ_HINT, a bound
    from the hint; NNZ_ELL, max_deg * tm (ELL slices both ways: no kernel uses the figure); NNZ_READBACK, hub graphs without a hint,
    whose kernels stage CSR slices and need the exact sizes: read back after the ELL launch (0 here)."""
    nrb: int
    ntiles: int
    utilisation: float
    max_segment: int
    max_tile_rows: int
    ell: int
    ellT: int
    uniform_rows: int            # > 0: tile_start in closed form, tile t starts at row t * uniform_rows; 0: the walk's candidate ``walk_index``
    walk_index: Optional[int]
    nnz: str
    max_nnz: int
    max_nnzT: int


def best_height(N: int, choices, ntiles_of) -> Optional[Tuple[float, int, int]]:
    """THE height rule: (utilisation, nrb, ntiles) of the candidate that fills its tiles best; one later in ``choices`` has to be better
    by more than 0.03, so that ``choices`` is the preference order on ties.  ``ntiles_of(nrb)`` <= 0: no tiling of that height.  None: of none."""
    best = None
    for cand in choices:
        nt = ntiles_of(cand)
        if nt <= 0:
            continue
        util = N / float(nt * 32 * cand)
        if best is None or util > best[0] + 0.03:
            best = (util, cand, nt)
    return best


def _ell_width(max_deg: int) -> int:
    return max_deg if max_deg <= _ELL_MAX else 0       # (0: a row above 8 entries, CSR staging)


def spec_from_hint(hint: TopologyHint, N: int, directed: bool, choices) -> Optional[TileSpec]:
    """Closed form: G = N / n graphs of n rows each, (32 * nrb) // n of them per tile; degrees and the entry bound from the hint."""
    n = hint.nodes_per_graph
    G = N // n
    best = best_height(N, choices, lambda c: -(-G // ((32 * c) // n)) if 32 * c >= n else 0)
    if best is None:
        return None
    util, nrb, nt = best
    per = (32 * nrb) // n
    width = _ell_width(int(hint.max_degree))
    bound = per * hint.max_edges_per_graph * (2 if directed else 1)
    return TileSpec(nrb=nrb, ntiles=nt, utilisation=util, max_segment=n, max_tile_rows=per * n, ell=width, ellT=width,
                    uniform_rows=per * n, walk_index=None, nnz=NNZ_HINT, max_nnz=bound, max_nnzT=bound)


def spec_from_stats(s: Dict[str, object], N: int, choices) -> Optional[TileSpec]:
    """From the statistics of a walk over ``choices`` (``s["ntiles_cand"][i]``: the tiles of choices[i], <= 0 where a segment does not fit)."""
    best = best_height(N, choices, dict(zip(choices, s["ntiles_cand"])).__getitem__)
    if best is None:
        return None
    util, nrb, nt = best
    tm, seg = 32 * nrb, s["max_segment"]
    ell, ellT = _ell_width(s["max_deg"]), _ell_width(s["max_degT"])
    nnz = NNZ_ELL if ell and ellT else NNZ_READBACK
    # (max_tile_rows is known without another copy only where every graph has the same size: whole graphs per tile)
    return TileSpec(nrb=nrb, ntiles=nt, utilisation=util, max_segment=seg, max_tile_rows=(tm // seg) * seg if s["min_segment"] == seg else 0,
                    ell=ell, ellT=ellT, uniform_rows=0, walk_index=list(choices).index(nrb), nnz=nnz,
                    max_nnz=s["max_deg"] * tm if nnz == NNZ_ELL else 0, max_nnzT=s["max_degT"] * tm if nnz == NNZ_ELL else 0)


def stat_words(primary: bool, closed_form: bool, has_ell: bool) -> Optional[str]:
    """Which 16 statistic words the launches of a tiling write: "own" (the Topology's), "copy" (a private copy, error flag and per-tile
    maxima zeroed) or None (there is no ELL launch).  The Topology's words describe the PRIMARY tiling and nothing else:
    * the primary writes them, whatever it is (a hinted hub primary too: its launch has no slices, but posts the primary's entry maxima);
    * a walked alternate writes candidate counts (the walk) and entry maxima (the ELL launch), with or without slices: a copy;
    * a closed-form alternate with slices posts no statistic (uniform_rows > 0), only the error flag, which is about the hint the
      primary was built from as well: the Topology's words, no clone and no fill on the fresh-batch path;
    * a closed-form alternate WITHOUT slices (hub graphs) has nothing to write -- tile_start comes from dss2_tiles_uniform, the entry
      bound from the hint -- and its launch would post its own maxima where the primary's stand: it is not issued."""
    if primary:
        return "own"
    if not closed_form:
        return "copy"
    return "own" if has_ell else None


def _stream(dev) -> int:
    return _lib.stream_ptr(dev)


def probe(edge_index: torch.Tensor) -> Tuple[int, int, bool]:
    """(hash1, hash2, is_directed) of edge_index in one kernel + one 24-byte device-to-host copy."""
    ei = edge_index if edge_index.is_contiguous() else edge_index.contiguous()
    out = torch.zeros(3, dtype=torch.int64, device=ei.device)
    _lib.check(_lib.lib().dss2_topology_probe(ei.data_ptr(), ei.size(1), out.data_ptr(), _stream(ei.device)), "dss2_topology_probe")
    h1, h2, rev = out.tolist()
    return h1, h2, rev == 0


def reference_is_directed(edge_index: torch.Tensor) -> bool:
    """/root/reference/networks.py:236-238: looks only at the first edge of the batch:
    is there NO edge (v0 -> u0) among the edges leaving v0?  (One host sync; cached per topology.)"""
    if edge_index.is_cuda:
        return probe(edge_index)[2]
    u0, v0 = edge_index[0, 0], edge_index[1, 0]
    cand = edge_index[1, edge_index[0, :] == v0]
    return not bool((cand == u0).any().item())


class Topology:
    """Frozen device-side structure of one batched graph.  See include/dss2_hip.h."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, nrb: Optional[int] = None,
                 double: Optional[bool] = None, hint: Optional[TopologyHint] = None, flip: bool = True,
                 edge_count: Optional[torch.Tensor] = None):
        """double=None: the reference's rule (MPN.is_directed on the first edge; from the hint when given); False: use
        the edge list exactly as given (standalone EdgeAggregation / TAGConv / propagate); True: always double.
        flip=False: reverse edges carry no sign-flip flag (the Multi* / MaskEmbd* variants duplicate edge_attr unchanged,
        /root/reference/networks.py:440-444, where MPN negates columns 0 and 2, :250-254).
        edge_count (device int32 [G], with a hint of uniform graphs): a PADDED batch -- graph g owns ``hint.edges_per_graph`` stored edge
        slots of which the first edge_count[g] are branches and the rest padding edges the structure never lists.  Every buffer is then
        sized by the slots and stays where it is; ``rebuild()`` rebuilds the content from edge_index / edge_count as they are on the
        device at that moment, with launches that are part of a recorded training step (dss2_csr_build_padded).  ``E`` counts the
        slots; ``edge_total`` (device int32 [1]) is the real edge count of the batch that was last built."""
        ei = self._checked(edge_index, num_nodes)
        self.N, self.E, self.device = int(num_nodes), int(ei.size(1)), ei.device
        self.hint, self._nrb_forced, self.flip = hint, nrb, bool(flip)
        if double is not None:
            self.directed = bool(double)
        elif hint is not None:
            self.directed = bool(hint.directed)
        else:
            self.directed = probe(ei)[2]
        self.E2 = 2 * self.E if self.directed else self.E
        # (padded batches: the entries behind rowptr[N] are never written -- zeros once, so that nothing indeterminate sits there)
        self._arena(torch.zeros if edge_count is not None else torch.empty)
        a = self._csr_args(ei)
        self._deg_pows = None
        self._padded = None
        self.edge_count = self.edge_total = None                 # (padded batches only)
        self._ell_jobs: List[_lib.EllBuildArgs] = []       # padded batches: the ELL launch of every tiling, in build order (rebuild())
        self._stats = None
        self._tiling: Optional[Tiling] = None               # the primary tiling, built on first use
        self._alt_tilings: Dict[int, Optional[Tiling]] = {}
        self._gnn_structures: Dict[int, object] = {}        # gnn._structure: normalisation mode -> the lane-group models' structure
        per_graph = self._per_graph_build_fits()
        if edge_count is not None:
            self._build_padded(a, ei, edge_count, double)
        elif per_graph:
            self._build_per_graph(a, ei)
        else:
            self._build_general(a, ei)

    @staticmethod
    def _checked(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
        """The argument checks; edge_index, contiguous."""
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        N, E = int(num_nodes), int(edge_index.size(1))
        if E == 0 or N == 0:
            raise ValueError("empty graph batch")
        if N >= 2 ** 31 - 4 or 2 * E >= 2 ** 31 - 4:
            raise ValueError("graph too large for the int32 CSR")
        if not edge_index.is_cuda:
            raise RuntimeError("DSS2 HIP path: edge_index must live on the GPU (there is no CPU fallback)")
        return edge_index if edge_index.is_contiguous() else edge_index.contiguous()

    def _arena(self, alloc) -> None:
        """One int32 arena for every array, 16-byte aligned slices, as attributes; ``_addr``: name -> device address of each slice, what
        the argument records of the builds are filled from."""
        N, E, E2 = self.N, self.E, self.E2
        sizes = [("rowptr", N + 1), ("col", E2), ("ent", E2), ("perm", E2), ("w", E2), ("rowptrT", N + 1), ("colT", E2),
                 ("entT", E2), ("permT", E2), ("wT", E2), ("inc_rowptr", N + 1), ("inc_ent", 2 * E), ("efrom", E), ("eto", E),
                 ("deg", N), ("_lastcut", N + 1), ("_meta", 16)]
        padded = [(n + 3) // 4 * 4 for _, n in sizes]
        arena = alloc(sum(padded), dtype=torch.int32, device=self.device)
        d, where, addr = self.__dict__, {}, arena.data_ptr()
        for (name, n), pn, chunk in zip(sizes, padded, arena.split(padded)):       # one split call: 17 views (16-byte aligned)
            d[name] = chunk[:n] if n != pn else chunk
            where[name] = addr
            addr += 4 * pn
        for name in ("w", "wT", "deg"):
            d[name] = d[name].view(torch.float32)
        self._addr = where

    def _csr_args(self, ei: torch.Tensor) -> "_lib.CsrBuildArgs":
        a = _lib.CsrBuildArgs()
        a.edge_index, a.n_edges, a.n_nodes, a.doubled, a.no_flip = ei.data_ptr(), self.E, self.N, int(self.directed), int(not self.flip)
        for name, addr in self._addr.items():
            setattr(a, name.lstrip("_"), addr)
        return a

    def _per_graph_build_fits(self) -> bool:
        """Are the graphs' ranges in the stored edge list known (round 6), and the graphs small enough for a wave each?"""
        hint = self.hint
        return (hint is not None and (hint.edges_per_graph > 0 or hint.edge_ptr is not None) and self.N % hint.nodes_per_graph == 0
                and os.environ.get("DSS2_TOPO_GRAPHS", "1") != "0"
                and bool(_lib.lib().dss2_csr_build_graphs_supported(hint.nodes_per_graph, hint.max_edges_per_graph)))

    # ---- the three builds of the CSR part.  Each leaves ``_keep`` (what its asynchronous launches read) and says what else
    def _build_general(self, a, ei) -> None:
        """dss2_csr_build, global scans, any batch.  Leaves: ``_keep``; ``_deg_pows`` None (built on first use, ``deg_pows``)."""
        L = _lib.lib()
        work = torch.empty(int(L.dss2_csr_build_work_ints(self.N, self.E, int(self.directed))), dtype=torch.int32, device=self.device)
        a.work = work.data_ptr()
        _lib.check(L.dss2_csr_build(C.byref(a), _stream(self.device)), "dss2_csr_build")
        self._keep = (ei,)

    def _build_per_graph(self, a, ei) -> None:
        """dss2_csr_build_graphs, one wave per graph: every array AND the [N, 4] folded-bias row scales in one launch.  Leaves: ``_keep``,
        ``_deg_pows``."""
        hint, ep = self.hint, self.hint.edge_ptr
        self._deg_pows = torch.empty(self.N, 4, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().dss2_csr_build_graphs(C.byref(a), hint.nodes_per_graph, (ep.data_ptr() if ep is not None else None),
                                                    int(hint.edges_per_graph), int(hint.max_edges_per_graph), self._deg_pows.data_ptr(),
                                                    _stream(self.device)), "dss2_csr_build_graphs")
        self._keep = (ei, ep)

    def _build_padded(self, a, ei, edge_count: torch.Tensor, double) -> None:
        """dss2_csr_build_padded, through ``rebuild()``.  Leaves: ``_keep``, ``_deg_pows``, ``edge_count``, ``edge_total``, ``_csr_ptr``
        and ``_padded``, the argument record every later ``rebuild()`` re-issues."""
        hint, N, dev = self.hint, self.N, self.device
        n = hint.nodes_per_graph if hint is not None else 0
        if double is not None or hint is None or n <= 0 or N % n or hint.edges_per_graph <= 0 or hint.edges_per_graph * (N // n) != self.E:
            raise ValueError("a padded Topology needs a TopologyHint of uniform graphs: edges_per_graph slots for each of N / nodes_per_graph graphs")
        if edge_count.dtype != torch.int32 or edge_count.device != dev or not edge_count.is_contiguous() or edge_count.numel() != N // n:
            raise ValueError("edge_count: a contiguous int32 device tensor with one entry per graph")
        if not _lib.lib().dss2_csr_build_graphs_supported(n, hint.edges_per_graph):
            raise NotImplementedError(f"padded batches of {n}-node graphs with {hint.edges_per_graph} edge slots are beyond the per-graph build")
        q = _lib.PaddedBuildArgs()
        q.csr = a
        q.nodes_per_graph, q.edge_stride = n, int(hint.edges_per_graph)
        self.edge_count, self.edge_total = edge_count, torch.zeros(1, dtype=torch.int32, device=dev)
        self._csr_ptr = torch.empty(N // n + 1, dtype=torch.int64, device=dev)
        self._deg_pows = torch.empty(N, 4, dtype=torch.float32, device=dev)
        q.edge_count, q.csr_ptr, q.edge_total, q.deg_pows = edge_count.data_ptr(), self._csr_ptr.data_ptr(), self.edge_total.data_ptr(), self._deg_pows.data_ptr()
        self._padded = q
        self._keep = (ei, edge_count)
        self.rebuild()

    def rebuild(self) -> None:
        """Padded batches: the CSR part, the folded-bias row scales and every tiling built so far, again, from what edge_index and
        edge_count hold on the device NOW -- into the same buffers, by launches a launch plan records and a hipGraph captures.  (A
        tiling is built lazily on first use; one first asked for while a step is being recorded is refused like every structure
        build outside a step: run the step once before recording it.)"""
        q = self._padded
        if q is None:
            raise ValueError("rebuild(): not a padded Topology (pass edge_count)")
        q.n_ell = len(self._ell_jobs)
        for i, b in enumerate(self._ell_jobs):
            q.ell[i] = b
        self._stats = None
        _lib.check(_lib.lib().dss2_csr_build_padded(C.byref(q), _stream(self.device)), "dss2_csr_build_padded")

    # ---- lazily built tile part -------------------------------------------------------------------------------
    @property
    def tiling(self) -> Tiling:
        """The primary tiling (built on first use)."""
        ts = self._tiling
        if ts is None:
            ts = self._tiling = self._build_tiles()
        return ts

    def __getattr__(self, name):
        # the tile fields read on the Topology (benchmark, tests, tools): those of the primary tiling.  Package code on the step path
        # takes ``topo.tiling`` once and reads the record
        if name in _TILING_FIELDS:
            return getattr(self.tiling, name)
        raise AttributeError(name)

    @staticmethod
    def _read_stats(meta: torch.Tensor) -> Dict[str, int]:
        m = meta.tolist()
        if m[_WORDS["error"]] in _ERRORS:
            raise ValueError(_ERRORS[m[_WORDS["error"]]])
        s = {name: m[i] for name, i in _WORDS.items()}
        s["ntiles_cand"] = m[_WORDS["ntiles_cand"]:]
        return s

    def stats(self) -> Dict[str, int]:
        """Exact build statistics of the PRIMARY tiling (one 64-byte device-to-host copy, cached): degrees, segments, error
        flag.  An alternate tiling (``tiles_for``) never shows up here: ``stat_words`` says what its launches write instead."""
        if self._stats is None:
            self._stats = self._read_stats(self._meta)
        return self._stats

    def tiles_for(self, nrb: int) -> Optional[Tiling]:
        """The Tiling with a FORCED tile height of 32 * nrb rows: the primary one itself (``self.tiling``) when that is its height,
        else an alternate built beside it (cached per height).  Used by the whole-stack kernels, which are latency-bound per tile
        (at small batches twice as many 32-row tiles put twice as many CUs to work), and by the weight gradient.  None when no
        whole-graph tiling of that height exists."""
        ts = self.tiling
        if ts.global_only:
            return None
        if nrb == ts.nrb:
            return ts
        if nrb not in self._alt_tilings:
            self._alt_tilings[nrb] = self._build_tiles(choices=(int(nrb),), primary=False)
        return self._alt_tilings[nrb]

    def _build_tiles(self, choices=None, primary=True) -> Optional[Tiling]:
        """primary: the best tiling of ``choices`` (its statistics are the Topology's own), uniform 64-row tiles where no graph fits
        a tile.  Else an alternate one, None where no graph fits a tile of the heights in ``choices``."""
        if choices is None:
            env = os.environ.get("DSS2_NRB")
            choices = (int(self._nrb_forced),) if self._nrb_forced else ((int(env),) if env else _NRB_CHOICES)
        hint = self.hint
        if hint is not None and self.N % hint.nodes_per_graph == 0:
            # ---- no device-to-host copy: uniform graphs => closed-form tiles, degrees from the hint
            spec, max_segment, tile_start = spec_from_hint(hint, self.N, self.directed, choices), hint.nodes_per_graph, None
            meta = self._meta if stat_words(primary, True, bool(spec and (spec.ell or spec.ellT))) == "own" else None
        else:
            # ---- general batch: greedy packing for every candidate row budget in one launch, then ONE copy of the statistics
            # (the rule's answer is needed before the walk, and with a walk it does not depend on the ELL widths the walk finds)
            meta = self._meta
            if stat_words(primary, False, False) == "copy":
                meta = meta.clone()
                meta[_PER_TILING].zero_()
            spec, max_segment, tile_start = self._walk(choices, meta, primary)
        if spec is None:
            return self._global_tiles(max_segment) if primary else None
        return self._launch_tiles(spec, tile_start, meta, primary)

    def _walk(self, choices, meta: torch.Tensor, primary: bool):
        """dss2_tiles_walk over ``choices`` and the copy of the statistics: (spec or None, longest segment, the chosen candidate's tile_start)."""
        N, dev = self.N, self.device
        cands = [torch.empty(N + 1, dtype=torch.int32, device=dev) for _ in choices]
        tm_host = (C.c_int32 * len(choices))(*[32 * c for c in choices])
        ptrs = (C.c_void_p * len(choices))(*[t.data_ptr() for t in cands])
        _lib.check(_lib.lib().dss2_tiles_walk(self._lastcut.data_ptr(), N, tm_host, len(choices), ptrs, N,
                                              meta[_WORDS["ntiles_cand"]:].data_ptr(), _stream(dev)), "dss2_tiles_walk")
        s = self._read_stats(meta)
        if primary:
            self._stats = s            # (what ``stats()`` returns where no tiling follows; one that follows adds its entry counts)
        spec = spec_from_stats(s, N, choices)
        return spec, s["max_segment"], (cands[spec.walk_index][:spec.ntiles + 1].clone() if spec is not None else None)

    def _launch_tiles(self, spec: TileSpec, tile_start: Optional[torch.Tensor], meta: Optional[torch.Tensor], primary: bool) -> Tiling:
        """From a spec to a Tiling.  tile_start None: closed form, written by the ELL launch along with its slices, by dss2_tiles_uniform
        where there are none (hub graphs).  meta: the statistic words the ELL launch writes, None: no ELL launch (``stat_words``)."""
        L, dev, st, N = _lib.lib(), self.device, _stream(self.device), self.N
        nt, tm, ell, ellT = spec.ntiles, 32 * spec.nrb, spec.ell, spec.ellT
        if self._padded is not None:
            # rebuild() re-issues the ELL launch with the step: it has to be the closed-form, ELL-staged kind, and there is room for a few
            if not (spec.uniform_rows and ell and ellT):
                raise NotImplementedError("padded batches: graphs with a bus of more than 8 branches have no ELL slices to rebuild")
            if len(self._ell_jobs) >= _lib.PADDED_MAX_TILINGS:
                raise NotImplementedError(f"padded batches: more than {_lib.PADDED_MAX_TILINGS} tilings of one batch")
        if tile_start is None:
            tile_start = torch.empty(nt + 1, dtype=torch.int32, device=dev)

        def slab(width):
            return torch.empty(nt, width, tm, 2, dtype=torch.int32, device=dev) if width > 0 else None
        ell_tiles, ell_ent_tiles, ellT_tiles, ellT_ent_tiles = slab(ell), slab(ell), slab(ellT), slab(ellT)
        b, at = _lib.EllBuildArgs(), self._addr
        b.rowptr, b.col, b.ent, b.w, b.rowptrT, b.colT, b.entT, b.wT = (at["rowptr"], at["col"], at["ent"], at["w"], at["rowptrT"], at["colT"],
                                                                        at["entT"], at["wT"])
        b.tile_start, b.ntiles, b.tm, b.ell_width, b.ellT_width = tile_start.data_ptr(), nt, tm, ell, ellT
        b.ell_tiles, b.ell_ent_tiles = (ell_tiles.data_ptr() if ell else None), (ell_ent_tiles.data_ptr() if ell else None)
        b.ellT_tiles, b.ellT_ent_tiles = (ellT_tiles.data_ptr() if ellT else None), (ellT_ent_tiles.data_ptr() if ellT else None)
        b.uniform_rows, b.n_nodes = (spec.uniform_rows if (ell or ellT) else 0), N
        if spec.uniform_rows and not b.uniform_rows:
            _lib.check(L.dss2_tiles_uniform(tile_start.data_ptr(), nt, spec.uniform_rows, N, st), "dss2_tiles_uniform")
        if meta is not None:
            b.meta = meta.data_ptr()
            _lib.check(L.dss2_ell_tiles_build(C.byref(b), st), "dss2_ell_tiles_build")
            if self._padded is not None:
                self._ell_jobs.append(b)
            if spec.uniform_rows and os.environ.get("DSS2_CHECK", "0") == "1":
                self._read_stats(meta)      # debugging aid: the closed-form path reads nothing back; this reads the error flag after all (ONE host sync)
        max_nnz, max_nnzT = spec.max_nnz, spec.max_nnzT
        if spec.nnz == NNZ_READBACK:
            s = self._read_stats(meta)
            max_nnz, max_nnzT = s["max_nnz"], s["max_nnzT"]
        if primary:
            self._stats = None            # (the ELL build added the per-tile entry counts to the statistics)
        return Tiling(global_only=False, nrb=spec.nrb, ntiles=nt, tile_start=tile_start, utilisation=spec.utilisation,
                      max_segment=spec.max_segment, max_tile_rows=spec.max_tile_rows, max_nnz=max_nnz, max_nnzT=max_nnzT, ell=ell, ellT=ellT,
                      ell_tiles=ell_tiles, ellT_tiles=ellT_tiles, ell_ent_tiles=ell_ent_tiles, ellT_ent_tiles=ellT_ent_tiles)

    def _global_tiles(self, max_segment: int) -> Tiling:
        """A connected component exceeds the largest LDS-resident tile (192 rows): no graph-aligned tiles exist.  The
        plain GEMMs still run on uniform 64-row tiles; the propagation hops run in global memory on the CSR
        (dss2_csr_axpy) and the edge MLP on the row-per-wave CSR kernels (networks._tagconv_forward_global)."""
        nt = -(-self.N // 64)
        tile_start = torch.empty(nt + 1, dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().dss2_tiles_uniform(tile_start.data_ptr(), nt, 64, self.N, _stream(self.device)), "dss2_tiles_uniform")
        return Tiling(global_only=True, nrb=2, ntiles=nt, tile_start=tile_start, utilisation=self.N / float(nt * 64), max_segment=max_segment,
                      max_tile_rows=0, max_nnz=0, max_nnzT=0, ell=0, ellT=0, ell_tiles=None, ellT_tiles=None,
                      ell_ent_tiles=None, ellT_ent_tiles=None)

    @property
    def deg_pows(self) -> torch.Tensor:
        """[N, 4] fp32, column m = A_hat^m deg (A_hat = the gcn_norm propagation matrix): the row scales of
        a bias folded through m propagations (networks._FoldPlan).  Built once per topology, in fp64."""
        if self._deg_pows is None:
            out = torch.empty(self.N, 4, dtype=torch.float32, device=self.device)
            work = torch.empty(2 * self.N, dtype=torch.float64, device=self.device)
            _lib.check(_lib.lib().dss2_deg_pows(self.rowptr.data_ptr(), self.col.data_ptr(), self.w.data_ptr(),
                                                self.deg.data_ptr(), self.N, out.data_ptr(), work.data_ptr(),
                                                _stream(self.device)), "dss2_deg_pows")
            self._deg_pows = out
        return self._deg_pows

    def lds_check(self, nmat: int, kpad: int, ncg: int) -> None:
        from .ops import gemm_plan      # (ops imports this module)
        ts = self.tiling
        if ts.global_only:     # plain GEMMs only: forward K=kpad -> nmat*hout columns, data-gradient K=nmat*hout -> kpad
            need = max(gemm_plan(ts, 1, kpad, nmat * ncg * 32, graph=(0, 0)).sizing_lds, gemm_plan(ts, 1, nmat * ncg * 32, kpad, graph=(0, 0)).sizing_lds)
            if need > LDS_LIMIT:
                raise NotImplementedError(f"global-memory path: a 64-row tile x K={nmat * ncg * 32} needs {need} B of LDS (> 160 KiB)")
            return
        need = gemm_plan(ts, nmat, kpad, ncg * 32, graph=(max(ts.max_nnz, ts.max_nnzT), min(ts.ell, ts.ellT))).sizing_lds
        if need > LDS_LIMIT:
            raise NotImplementedError(f"tile of {32 * ts.nrb} rows x K={kpad} needs {need} B of LDS (> 160 KiB)")


# ------------------------------------------------------------------------------------------
# cache: identity fast path (same tensor object, unmodified) -> no sync; otherwise content hash
# ------------------------------------------------------------------------------------------
_by_hash: Dict[Tuple, Topology] = {}
_last: Dict[Tuple[int, str], Tuple] = {}   # (id(tensor), mode) -> (weakref, version, data_ptr, num_nodes, topo)
_MAX_CACHE = 64


def _mode(double: Optional[bool], flip: bool = True) -> str:
    return ("ref" if double is None else ("dbl" if double else "asis")) + ("" if flip else "-noflip")


def register_topology(edge_index: torch.Tensor, num_nodes: int, topo: Topology, double: Optional[bool] = None,
                      flip: bool = True) -> Topology:
    """Attach an already built structure to this very tensor object: the next ``get_topology(edge_index, ...)`` (the
    model's forward, the loss) returns it without hashing or synchronising.  Used by dataset.DataLoader."""
    if len(_last) >= _MAX_CACHE:
        _last.pop(next(iter(_last)))
    key = (id(edge_index), _mode(double, flip))

    def _drop(ref, key=key, table=_last):   # the tensor died: release its structure (device arrays) with it
        hit = table.get(key)
        if hit is not None and hit[0] is ref:
            table.pop(key, None)
    _last[key] = (weakref.ref(edge_index, _drop), edge_index._version, edge_index.data_ptr(), int(num_nodes), topo)
    return topo


def attached_topology(edge_index: torch.Tensor, num_nodes: int, double: Optional[bool] = None, flip: bool = True) -> Optional[Topology]:
    """The structure attached to this very tensor object (``register_topology``) if the tensor is unmodified since, else None:
    the identity fast path, no hashing and no synchronisation."""
    hit = _last.get((id(edge_index), _mode(double, flip)))
    if hit is not None:
        ref, ver, ptr, nn, topo = hit
        if ref() is edge_index and ver == edge_index._version and ptr == edge_index.data_ptr() and nn == num_nodes:
            return topo
    return None


def get_topology(edge_index: torch.Tensor, num_nodes: int, double: Optional[bool] = None, flip: bool = True) -> Topology:
    """The cached structure of this batch.  double=None: the reference's doubling rule (MPN / the loss);
    False: the edge list exactly as given (standalone EdgeAggregation / TAGConv / MessagePassing.propagate)."""
    if not edge_index.is_cuda:
        raise RuntimeError("DSS2 HIP path: edge_index must live on the GPU (there is no CPU fallback)")
    topo = attached_topology(edge_index, num_nodes, double, flip)
    if topo is not None:
        return topo
    h1, h2, directed = probe(edge_index)
    key = (edge_index.device.index, int(num_nodes), int(edge_index.size(1)), h1, h2, _mode(double, flip))
    topo = _by_hash.get(key)
    if topo is None:
        topo = Topology(edge_index, num_nodes, double=(directed if double is None else double), flip=flip)
        if len(_by_hash) >= _MAX_CACHE:
            _by_hash.pop(next(iter(_by_hash)))
        _by_hash[key] = topo
    return register_topology(edge_index, num_nodes, topo, double, flip)


def clear_cache() -> None:
    _by_hash.clear()
    _last.clear()
