"""The case table of the MPN path at hidden widths, head widths, K and depths that no other test runs, shared by
tests/test_mpn_width_cases_cpu.py (structure, route, coverage and conditioning of every case, no GPU) and tests/test_gpu_mpn_widths.py
(the kernels against the fp64 oracle model of every case).

tests/mpn_shape_cases.py moves the graph's numbers (ELL width, tile height, rows per tile); the cases here keep its graphs and move the
model's: dim_hid off the 32 grid (a partly filled last column group, kpad > kreal), dim_out 1 .. 11, K 1 .. 3 and up to 11 layers.  A case
repeats the graph fields of its base case exactly, so edge list, x, edge_attr and STRUCTURE are the base's (``mpn_shape_cases.batch`` is
keyed by those fields); gout is drawn behind them for the case's own dim_out and the weights are the oracle model's own initialisation.

ROUTE pins what each case is there for, in the form of mpn_shape_cases.ROUTE with one entry more: per block the layer chain's record
(dss2_chain_plan_t) in both directions.  VARIANTS pins what each flag of the format reruns moves.  All literals were read off the library
BEFORE these tests existed, on the stand-in topology, never from a run of changed code."""
import contextlib

import mpn_shape_cases as mc
from mpn_shape_cases import E_BF16X6, E_VALU, WG_BF16_64, WG_F16_32, WG_F16_TALL, WG_FP32

WG_NONE, WG_BF16_TALL = 0, 6                             # dss2_wgrad_kernel (the others: mpn_shape_cases)
NONE, FP32, BF16X6, SP, SP6 = range(5)                   # dss2_chain_family: none, fp32 and bf16x6 multi-wave, split-plane 64-row, split-plane tall


def _on(base, name, args, purpose, cls="MPN"):
    b = mc.BY_NAME[base]
    return mc.Case(name, b.counts, b.cap, cls, args, purpose, tail=b.tail, full=b.full, dup3=b.dup3, seed=b.seed)


def _mpn(nout, hid, layers, K):
    return (8, 6, nout, hid, layers, K, 0.0)


# name -> the case of mpn_shape_cases whose graphs it runs on
BASE = {
    "w36_rs2": "full64_ell5", "w44_k1": "full64_ell5", "w40_k3": "full64_ell5", "w72_head": "full64_ell5", "w100_out3": "full64_ell5",
    "w136_w8": "full64_ell5", "w252": "full64_ell5", "w160_out5": "full64_ell5", "out11_wide_head": "full64_ell5",
    "w260_nochain": "full64_ell5", "w70_scalar": "full64_ell5", "d10_split": "full64_ell5",
    "t96_w44": "n65_ell6", "t96_w100_out4_k1": "n65_ell6", "t96_w136_fp32": "n65_ell6", "t96_d11": "n65_ell6",
    "t192_w72_out1": "full192_ell8", "t32_w200": "nrb1_ell8", "c2g_w96": "c2_ell8_head_edge",
    "stack_w40": "stack_full64_ell4",
}

CASES = [
    _on("full64_ell5", "w36_rs2", _mpn(2, 36, 4, 2),
        "bf16x6 multi-wave chain, row split 2, 4 waves, kpad 48 > 36, no gate words, no head; bf16x6 64-row weight gradient; VALU edge kernels"),
    _on("full64_ell5", "w44_k1", _mpn(2, 44, 4, 1), "the same family at nmat 2, last column group of 12"),
    _on("full64_ell5", "w40_k3", _mpn(2, 40, 4, 3), "nmat 4: the bf16x6 chain with the fp32 weight gradient"),
    _on("full64_ell5", "w72_head", _mpn(2, 72, 4, 2),
        "split-plane bf16x6 chain, 96 gate words, fused head forward and backward with its weight gradient; no f16x3 form"),
    _on("full64_ell5", "w100_out3", _mpn(3, 100, 4, 2),
        "4 column groups, the last holding 4 columns; fused head without its weight gradient (nout 3)"),
    _on("full64_ell5", "w136_w8", _mpn(2, 136, 4, 2), "5 column groups, 8 waves, 160 gate words"),
    _on("full64_ell5", "w252", _mpn(2, 252, 4, 2), "last width under the cap, 256 gate words"),
    _on("full64_ell5", "w160_out5", _mpn(5, 160, 4, 2), "f16x3 at 8 waves; nout 5: no fused head, the head still a narrow layer (15 columns)"),
    _on("full64_ell5", "out11_wide_head", _mpn(11, 128, 4, 2), "3 * 11 = 33 > 32: the head is no longer a narrow layer"),
    _on("full64_ell5", "w260_nochain", _mpn(2, 260, 3, 2),
        "above 256: MPN.forward leaves the fused block for the per-layer autograd nodes (general edge aggregation, one TAGConv node per layer)"),
    _on("full64_ell5", "w70_scalar", _mpn(2, 70, 3, 2), "hid % 4 != 0: no chain, scalar loads and epilogues, fp32 weight gradient"),
    _on("full64_ell5", "d10_split", _mpn(2, 64, 10, 2),
        "9 chained layers > CHAIN_MAX: two launches per direction, the second reading the first's last Y"),
    _on("n65_ell6", "t96_w44", _mpn(2, 44, 4, 2),
        "96-row split-plane f16x3, 2 waves, backward head with its weight gradient; tall f16x3 weight gradient"),
    _on("n65_ell6", "t96_w100_out4_k1", _mpn(4, 100, 4, 1), "96-row split-plane f16x3, 4 waves, nmat 2, backward head at nout 4"),
    _on("n65_ell6", "t96_w136_fp32", _mpn(2, 136, 4, 2), "the fp32 chain (8 waves) as the default route: no 16-bit form"),
    _on("n65_ell6", "t96_d11", _mpn(2, 64, 11, 2), "10 chained f16x3 layers on tall tiles, heads dropped"),
    _on("full192_ell8", "t192_w72_out1", _mpn(1, 72, 4, 2), "192-row split-plane f16x3 with 3 waves, no fp32 chain at all; backward head at nout 1"),
    _on("nrb1_ell8", "t32_w200", _mpn(2, 200, 4, 2),
        "32-row tiling: bf16x6 chain at 8 waves; 32-row f16x3 weight gradient at a width off the 32 grid"),
    _on("c2_ell8_head_edge", "c2g_w96", _mpn(2, 96, 4, 2),
        "64-row f16x3 split-plane chain with 3 column groups, fused heads, no edge phase (hid != 128); 32-row f16x3 weight gradient"),
]
# the one stack: SkipPFN at a width the whole-stack kernels (hid 32) decline
STACK_CASE = _on("stack_full64_ell4", "stack_w40", (8, 6, 2, 40, 3, 2, 0.0, 2),
    "the whole-stack kernels decline hid != 32; the per-block bf16x6 chains of two layers inside the stack node", cls="SkipPFN")
ALL_CASES = CASES + [STACK_CASE]
# dim_hid > 256 (networks.EdgeAggregation.fused_dims): the model runs MPN._forward_general and stores no block route; ROUTE pins for it what
# the route predicates and the plans say of the shape (no chain in either direction, no tile family for the edge MLP)
GENERAL_PATH = ("w260_nochain",)
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES) and set(BY_NAME) == set(BASE) and not set(BY_NAME) & set(mc.BY_NAME)


def _row(f16, n_chain, use16, gw, head=False, bwd_head=False, bwd_head_wgrad=False, bwd_chain=True):
    """A block route in the order of mpn_shape_cases.ROUTE_FIELDS (no case here has an edge phase in a chain or takes the global path)."""
    return (f16, n_chain, use16, gw, head, False, bwd_chain, bwd_head, bwd_head_wgrad, False, False)


def _plan(fp32, b16, f16, gate_words=(0, 0), head_modes=(0, 0), head_wgrad=(0, 0)):
    """A chain record: (family, row_split, waves) of the three weight formats, then what the two 16-bit formats carry.  Every case has
    the same record in both directions."""
    return ((fp32, b16, f16), gate_words, head_modes, head_wgrad)


_NO = (NONE, 0, 0)
_P_RS2 = _plan((FP32, 2, 4), (BF16X6, 2, 4), _NO)                                         # <= 2 column groups on 64-row tiles: two waves each
_P_NONE = _plan(_NO, _NO, _NO)
_P_T96_2W = _plan((FP32, 1, 4), (SP6, 1, 2), (SP6, 1, 2), (128, 128), (2, 2), (1, 1))      # 96-row tiles, 2 column groups


def _entry(row, wg, edge, plan, edge_dx=None, blocks=1, stack=False):
    """need_dx -> the ROUTE entry; the input gradient only changes the edge families."""
    chains = ((plan, plan),) * blocks
    return {False: (stack, (row,) * blocks, wg, edge, chains),
            True: (stack, (row,) * blocks, wg, (edge[0], edge[1], edge[0]) if edge_dx is None else edge_dx, chains)}


_VALU, _MFMA = (E_VALU, E_VALU, 0), (E_BF16X6, E_BF16X6, 0)        # hid off the 32 grid: the VALU tile kernels
# name -> need_dx -> (whole-stack kernels take the model, ROUTE_FIELDS of every block, (tile rows, dss2_wgrad_kernel) of the hid -> hid
# weight gradients, dss2_edge_family (forward, backward by target, backward by source), per block (forward, transposed) chain record)
ROUTE = {
    "w36_rs2": _entry(mc._BF16X6_3, (64, WG_BF16_64), _VALU, _P_RS2),
    "w44_k1": _entry(mc._BF16X6_3, (64, WG_BF16_64), _VALU, _P_RS2),
    "w40_k3": _entry(mc._BF16X6_3, (64, WG_FP32), _VALU, _P_RS2),
    "w72_head": _entry(_row(False, 3, True, 96, True, True, True), (64, WG_BF16_64), _VALU,
                       _plan((FP32, 1, 4), (SP, 1, 4), _NO, (96, 0), (3, 0), (1, 0))),
    "w100_out3": _entry(_row(False, 3, True, 128, True, True, False), (64, WG_BF16_64), _VALU,
                        _plan((FP32, 1, 4), (SP, 1, 4), _NO, (128, 0), (3, 0), (0, 0))),
    "w136_w8": _entry(_row(False, 3, True, 160, True, True, True), (64, WG_BF16_64), _VALU,
                      _plan((FP32, 1, 8), (SP, 1, 8), _NO, (160, 0), (3, 0), (1, 0))),
    "w252": _entry(_row(False, 3, True, 256, True, True, True), (64, WG_BF16_64), _VALU,
                   _plan((FP32, 1, 8), (SP, 1, 8), _NO, (256, 0), (3, 0), (1, 0))),
    "w160_out5": _entry(_row(True, 3, True, 160), (64, WG_BF16_64), _MFMA, _plan((FP32, 1, 8), (SP, 1, 8), (SP, 1, 8), (160, 160)),
                        edge_dx=(E_BF16X6, E_BF16X6, E_VALU)),
    "out11_wide_head": _entry(_row(True, 3, True, 128), (64, WG_BF16_64), _MFMA, _plan((FP32, 1, 4), (SP, 1, 4), (SP, 1, 4), (128, 128)),
                              edge_dx=(E_BF16X6, E_BF16X6, E_VALU)),
    "w260_nochain": _entry(mc._LAYERS, (64, WG_BF16_64), (0, 0, 0), _P_NONE),
    "w70_scalar": _entry(mc._LAYERS, (64, WG_FP32), _VALU, _P_NONE),
    "d10_split": _entry(_row(False, 9, True, 0), (64, WG_BF16_64), _MFMA, _P_RS2, edge_dx=(E_BF16X6, E_BF16X6, E_VALU)),
    "t96_w44": _entry(_row(True, 3, True, 128, False, True, True), (96, WG_F16_TALL), _VALU, _P_T96_2W),
    "t96_w100_out4_k1": _entry(_row(True, 3, True, 256, False, True, False), (96, WG_F16_TALL), _VALU,
                               _plan((FP32, 1, 4), (SP6, 1, 4), (SP6, 1, 4), (256, 256), (2, 2), (0, 0))),
    "t96_w136_fp32": _entry(_row(False, 3, False, 0), (96, WG_F16_TALL), _VALU, _plan((FP32, 1, 8), _NO, _NO)),
    "t96_d11": _entry(_row(True, 10, True, 128), (96, WG_F16_TALL), _MFMA, _P_T96_2W, edge_dx=(E_VALU, E_VALU, E_VALU)),
    "t192_w72_out1": _entry(_row(True, 3, True, 288, False, True, True), (192, WG_F16_TALL), _VALU,
                            _plan(_NO, (SP6, 1, 3), (SP6, 1, 3), (288, 288), (2, 2), (1, 1))),
    "t32_w200": _entry(mc._BF16X6_3, (32, WG_F16_32), _VALU, _plan((FP32, 1, 8), (BF16X6, 1, 8), _NO)),
    "c2g_w96": _entry(_row(True, 3, True, 96, True, True, True), (32, WG_F16_32), _MFMA,
                      _plan((FP32, 1, 4), (SP, 1, 4), (SP, 1, 4), (96, 96), (3, 3), (1, 1)), edge_dx=(E_BF16X6, E_BF16X6, E_VALU)),
    "stack_w40": _entry(mc._BF16X6_2, (64, WG_BF16_64), _VALU, _P_RS2, blocks=2),
}

# The format reruns (VARIANT_FLAGS below), without an input gradient: name -> variant -> ({BlockRoute field: value} where the route under
# the flag differs from the default one, (tile rows, dss2_wgrad_kernel), edge families).  A weight-gradient flag moves no route field.
_NO_CHAIN = dict(n_chain=0, use16=False, bwd_chain=False, bwd_use16=False, bwd_join=False, bwd_defer=(False, True, True, False))
_NO_GW_HEAD = dict(gw=0, bwd_head=False, bwd_head_wgrad=False)
VARIANTS = {
    "w36_rs2": {
        "chain_f16_off": ({}, (64, WG_BF16_64), _VALU),                      # (no f16x3 form here: the default run again)
        "chain_bf16_off": (dict(b16=(), use16=False, bwd_use16=False), (64, WG_BF16_64), _VALU),         # the fp32 chain, row split 2
        "chain_layers_off": (_NO_CHAIN, (64, WG_BF16_64), _VALU),
        "wgrad_f16_off": ({}, (64, WG_BF16_64), _VALU),                      # (64-row tiles: bf16x6 already)
        "wgrad_bf16_off": ({}, (64, WG_FP32), _VALU),
    },
    "w72_head": {
        "chain_f16_off": ({}, (64, WG_BF16_64), _VALU),
        "chain_bf16_off": (dict(b16=(), use16=False, bwd_use16=False, head=False, **_NO_GW_HEAD), (64, WG_BF16_64), _VALU),
        "chain_layers_off": (dict(_NO_CHAIN, head=False, **_NO_GW_HEAD), (64, WG_BF16_64), _VALU),
        "wgrad_f16_off": ({}, (64, WG_BF16_64), _VALU),
        "wgrad_bf16_off": ({}, (64, WG_FP32), _VALU),
    },
    "t96_w44": {
        "chain_f16_off": (dict(f16=False), (96, WG_F16_TALL), _VALU),
        "chain_bf16_off": (dict(b16=(), f16=False, use16=False, bwd_use16=False, **_NO_GW_HEAD), (96, WG_F16_TALL), _VALU),
        "chain_layers_off": (dict(_NO_CHAIN, f16=False, **_NO_GW_HEAD), (96, WG_F16_TALL), _VALU),
        "wgrad_f16_off": ({}, (96, WG_BF16_TALL), _VALU),
        "wgrad_bf16_off": ({}, (96, WG_FP32), _VALU),
    },
    "t192_w72_out1": {
        "chain_f16_off": (dict(f16=False), (192, WG_F16_TALL), _VALU),
        "chain_bf16_off": (dict(_NO_CHAIN, b16=(), f16=False, **_NO_GW_HEAD), (192, WG_F16_TALL), _VALU),      # no fp32 chain: layer by layer
        "chain_layers_off": (dict(_NO_CHAIN, f16=False, **_NO_GW_HEAD), (192, WG_F16_TALL), _VALU),
        "wgrad_f16_off": ({}, (192, WG_BF16_TALL), _VALU),
        # 192-row tiles have an fp32 weight gradient only where hid % 128 == 0 (csrc/dss2_wgrad.hip wgrad_w8): the library refuses the launch
        "wgrad_bf16_off": ({}, (192, WG_NONE), _VALU),
    },
}


# ------------------------------------------------------------------------------------------
# what a case's numbers mean to the kernels
# ------------------------------------------------------------------------------------------
def dims(case):
    """(dim_out, hid, layers, nmat) of a case."""
    return case.args[2], case.args[3], case.args[4], case.args[5] + 1


def kpad16(hid):
    """K of the tile GEMM as the 16-bit chains pad it (csrc/dss2_gemm_chain.hip chain_select)."""
    return (hid + 15) // 16 * 16


def last_group(hid):
    """First column of the partly filled last column group, None where hid fills its groups."""
    return None if hid % 32 == 0 else 32 * (hid // 32)


def pad_sensitive(case):
    hid = dims(case)[1]
    return hid % 32 != 0 or kpad16(hid) > hid


def hid_slices(case, name, tensor):
    """[(label, the tensor's slice of the last column group along one hid-sized axis)] of a parameter (gradient) named ``name``."""
    hid = dims(case)[1]
    c0 = last_group(hid)
    if c0 is None:
        return []
    return [(f"{name}[axis {ax}, {c0}:]", tensor.narrow(ax, c0, hid - c0)) for ax in range(tensor.dim()) if tensor.size(ax) == hid]


def kind_of(case, name):
    """The tensor kind a parameter's error is recorded under: the edge MLP's, the head's (a block's last conv) or a hid -> hid conv's."""
    if "edge_aggr" in name:
        return "edge-MLP weight"
    return "head weight" if f"convs.{dims(case)[2] - 1}." in name else "conv weight"


def heads_apart(flag):
    """The fields of a BlockRoute that flags.CHAIN_HEAD (both chains) or flags.CHAIN_HEAD_FWD (the forward chain) = False clears."""
    return dict(head=False) if flag == "CHAIN_HEAD_FWD" else dict(head=False, bwd_head=False, bwd_head_wgrad=False)


# ------------------------------------------------------------------------------------------
# the route with the chain's record
# ------------------------------------------------------------------------------------------
CHAIN_FIELDS = ("family", "row_split", "waves")


def _plan_literal(p):
    """dss2_chain_plan_t as a literal: ((family, row_split, waves) of fp32 / bf16x3 / f16x2 weights, gate_words, head_modes and head_wgrad
    of the two 16-bit formats)."""
    k = p.fmt
    return (tuple(tuple(getattr(k[f], n) for n in CHAIN_FIELDS) for f in range(3)), (k[1].gate_words, k[2].gate_words),
            (k[1].head_modes, k[2].head_modes), (k[1].head_wgrad, k[2].head_wgrad))


def chain_literal(case, topo=None):
    """Per block: (the chain's record forward, transposed) on the stand-in topology or on the device's."""
    P = mc.pkg()
    ts = (mc.stub_topology(case) if topo is None else topo).tiling
    return tuple(tuple(_plan_literal(P.ops.chain_plan(ts, m.K + 1, m.dim_hid, m.dim_out, tr)) for tr in (False, True)) for m in mc.blocks_of(case))


def route_literal(case, need_dx, block_routes=None, topo=None):
    """mpn_shape_cases.route_literal with the chain records behind it."""
    return mc.route_literal(case, need_dx, block_routes=block_routes, topo=topo) + (chain_literal(case, topo),)


@contextlib.contextmanager
def flags_set(**values):
    """``flags.NAME = value`` for every pair, restored on the way out."""
    FL = mc.pkg().flags
    keep = {k: getattr(FL, k) for k in values}
    for k, v in values.items():
        setattr(FL, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(FL, k, v)


# the format reruns: name -> the flags it switches off
VARIANT_FLAGS = {
    "chain_f16_off": ("CHAIN_F16",),            # f16x3 -> bf16x6 chains
    "chain_bf16_off": ("CHAIN_BF16",),          # -> the fp32 chain where one exists
    "chain_layers_off": ("CHAIN_LAYERS",),      # -> dss2_gemm_prop layer by layer
    "wgrad_f16_off": ("WGRAD_F16",),            # -> the bf16x6 weight gradient
    "wgrad_bf16_off": ("WGRAD_BF16",),          # -> the fp32 weight gradient
}
VARIANT_CASES = ("w36_rs2", "w72_head", "t96_w44", "t192_w72_out1")
HEAD_CASES = ("w72_head", "w100_out3", "w252", "t96_w100_out4_k1", "t192_w72_out1", "c2g_w96")
SPLIT_CASES = ("d10_split", "t96_d11")


def variant_literal(case, variant, default=None, block_route=None, topo=None):
    """What a format rerun moves, without an input gradient: ({BlockRoute field: value} where the route under the variant's flags differs
    from the default one, (tile rows, dss2_wgrad_kernel), the edge families).  ``default`` / ``block_route``: the routes two forwards
    stored (else route.block_route on the stand-in topology); ``topo``: the device Topology."""
    P = mc.pkg()
    stub = mc.stub_topology(case) if topo is None else topo
    if default is None:
        default = P.route.block_route(mc.blocks_of(case)[0], stub.tiling, False, False)
    with flags_set(**{f: False for f in VARIANT_FLAGS[variant]}):
        if block_route is None:
            block_route = P.route.block_route(mc.blocks_of(case)[0], stub.tiling, False, False)
        _, _, wg, edge = mc.route_literal(case, False, block_routes=[block_route], topo=topo)
    moved = {f: getattr(block_route, f) for f in block_route._fields if getattr(block_route, f) != getattr(default, f)}
    return moved, wg, edge
