"""Which kernels an MPN / SkipMPN block runs, decided ONCE per forward call.

``block_route`` reads ``flags`` and the library's chain record (``ops.chain_plan``, once per direction) when the forward starts
and returns every decision of the block, forward and backward, as one immutable record.  ``networks._ensure_plans`` and
``networks._mpn_forward`` follow it, and the forward hands it to ``networks._mpn_backward``, which evaluates no predicate of its
own: the two chains of a block (the forward chain writes ``S`` and the gate bits that the data-gradient chain reads) cannot
disagree.  A new fused form registers its condition HERE, once, as a field.  Nothing is cached: a flag flipped between two calls
takes effect at the next forward (not between a forward and its own backward)."""
from __future__ import annotations

from typing import NamedTuple, Tuple

from . import flags as FL
from .ops import (_tiles, chain16_supported, chain_edge_supported, chain_f16_supported, chain_gate_words, chain_head_supported,
                  chain_head_wgrad_supported, chain_plan, chain_supported, gemm16_supported, is_narrow)
from .topology import Topology


def use_global_path(topo: Topology, nmat: int) -> bool:
    """A TAGConv runs as ONE plain tile GEMM + K propagation hops in global memory when the graphs exceed the LDS-resident
    tiles (> 192 nodes) or when K > 3 (the fused tile kernels are instantiated for K + 1 <= 4 matrices)."""
    return bool(_tiles(topo).global_only or nmat > 4)


class BlockRoute(NamedTuple):
    """Per-layer tuples have one entry per conv (False for a layer that a chained launch covers)."""
    # weight space (what the module's _PackPlan / _FoldPlan hold)
    glob: bool                  # graphs beyond the LDS-resident tiles, or K > 3: plain GEMMs + propagation hops in global memory
    fold: bool                  # the edge MLP's second Linear folded into conv 0 (_FoldPlan)
    b16: Tuple[int, ...]        # pack groups (1 + layer) that also get bf16x3 packs -- or, with f16, f16x2 packs
    f16: bool
    # forward
    n_chain: int                # hid -> hid layers 0 .. n_chain-1 as ONE chained launch (0: none)
    use16: bool                 # ... its tile GEMM on the bf16 / f16 matrix pipe (b_format 1, or 2 with f16)
    gw: int                     # ... writing gw sign-bit words per tile and layer for the data-gradient chain (0: no bit words)
    head: bool                  # the narrow last layer inside the same launch (dss2_gemm_prop_chain_head, mode 1)
    edge: bool                  # ... and the edge MLP's first Linear in its staging (dss2_chain_edge, mode 1)
    g16: Tuple[bool, ...]       # per remaining layer: the bf16x6 single-layer form of the tall tiles
    # backward
    bwd_chain: bool             # last layer on its own, then the data gradients of layers L-2 .. 0 as ONE chained launch
    bwd_use16: bool
    bwd_head: bool              # the head's data gradient inside that launch (mode 2)
    bwd_head_wgrad: bool        # ... and its weight gradient from the same staging, one slab per tile
    bwd_edge: bool              # ... and the edge MLP's backward behind the chain's last layer (dss2_chain_edge, mode 2)
    bwd_join: bool              # the folded conv 0 rides in the batched weight-gradient launch of the plain layers
    bwd_g16: Tuple[bool, ...]   # per-layer route: the bf16x6 single-layer data gradient
    bwd_defer: Tuple[bool, ...]  # layers whose weight gradients wait for a batched launch (up to 8 consecutive layers each)


def block_route(mod, topo: Topology, need_dx: bool, in_stack: bool) -> BlockRoute:
    """The route of one forward call of ``mod`` (MPN / SkipMPN dimensions) on ``topo``.  ``need_dx``: the backward will be asked
    for the input gradient; ``in_stack``: the block runs inside a PFN / SkipPFN node (_PFNFn)."""
    L, nmat, hid, nout = mod.n_gnn_layers, mod.K + 1, mod.dim_hid, mod.dim_out
    houts = [nout if l == L - 1 else hid for l in range(L)]
    glob = use_global_path(topo, nmat)
    pf, pb = chain_plan(topo, nmat, hid, nout, False), chain_plan(topo, nmat, hid, nout, True)      # what the chain kernels say, per direction
    fold = bool(FL.FOLD_W2 and not is_narrow(nmat, houts[0]) and not glob)
    b16 = tuple(range(1, L)) if (FL.CHAIN_BF16 and not glob and hid % 4 == 0 and hid <= 256 and not is_narrow(nmat, hid) and L >= 2
                                 and (L >= 3 or gemm16_supported(topo, nmat, hid, False))) else ()
    # ... as f16x3 where both chains of the block have the form (64-row tiles; csrc/dss2_gemm_chain_sp.hip MS = 2) and the backward
    # takes the chained route
    f16 = bool(b16 and L >= 3 and FL.WGRAD_BATCH and chain_f16_supported(topo, nmat, hid, (pf, pb)))
    narrow_head = is_narrow(nmat, nout)
    # the edge MLP inside the chains: what both directions ask for besides their own fused head and shape query
    edge_ok = fold and f16 and not in_stack and not need_dx

    n_chain = L - 1 if (L - 1 >= 2 and chain_supported(topo, nmat, hid, False, bool(b16), pf)) else 0
    use16 = bool(n_chain and b16 and chain16_supported(topo, nmat, hid, False, pf))
    gw = chain_gate_words(topo, nmat, hid, (pf, pb)) if use16 else 0
    head = bool(use16 and FL.CHAIN_HEAD_FWD and n_chain <= FL.CHAIN_MAX and not glob and narrow_head
                and chain_head_supported(topo, nmat, hid, nout, False, pf))
    edge = bool(head and edge_ok and chain_edge_supported(topo, nmat, hid, False, pf))

    def tall16(l, transposed):      # a single hid -> hid layer with bf16x3 weights (b16 is empty on the global path)
        return bool(houts[l] == hid and (1 + l) in b16 and not f16 and gemm16_supported(topo, nmat, hid, transposed))
    first = L if head else n_chain
    g16 = tuple(first <= l < L - 1 and tall16(l, False) for l in range(L))

    bwd_chain = bool(L >= 3 and FL.WGRAD_BATCH and chain_supported(topo, nmat, hid, True, bool(b16), pb))
    bwd_use16 = bool(bwd_chain and b16 and chain16_supported(topo, nmat, hid, True, pb))
    # (tall tiles: only the direction-specialised data-gradient chain has the head form -- its layers gate with the forward's bit words)
    bwd_head = bool(bwd_use16 and L - 1 <= FL.CHAIN_MAX and narrow_head and chain_head_supported(topo, nmat, hid, nout, True, pb)
                    and (_tiles(topo).nrb <= 2 or gw > 0))
    bwd_head_wgrad = bool(bwd_head and chain_head_wgrad_supported(topo, nmat, hid, nout, pb))
    bwd_edge = bool(bwd_head and edge_ok and chain_edge_supported(topo, nmat, hid, True, pb))
    # The folded conv 0 joins the batched launch of the plain layers (round 4; flags.WGRAD_JOIN_FOLDED = False: its own launch).
    # Round 3 kept it apart because three layers x 85 workgroups leave a 13-vs-12-tile tail at C2; measured now, the
    # joined launch is 141 us against 93 + 57, and -- what matters more -- the step writes and re-reads half the slabs
    # (255 x 197 KB instead of 128 x 2 + 256): reduction 24.7 -> 17.8 us, C2 step 0.537 -> 0.509 ms on one box.
    bwd_join = bool(bwd_chain and fold and L - 1 <= 8 and (FL.WGRAD_JOIN_FOLDED is None or FL.WGRAD_JOIN_FOLDED))
    if bwd_chain:
        bwd_g16 = (False,) * L
        bwd_defer = tuple(not bwd_join and (1 if fold else 0) <= l < L - 1 for l in range(L))
    else:
        bwd_g16 = tuple(tall16(l, True) for l in range(L))
        bwd_defer = tuple(bool(FL.WGRAD_BATCH and not glob and not (l == 0 and fold) and houts[l] == hid and not is_narrow(nmat, hid))
                          for l in range(L))
    return BlockRoute(glob, fold, b16, f16, n_chain, use16, gw, head, edge, g16,
                      bwd_chain, bwd_use16, bwd_head, bwd_head_wgrad, bwd_edge, bwd_join, bwd_g16, bwd_defer)
