"""ctypes binding of libdss2_hip.so (the C ABI declared in include/dss2_hip.h).

There is NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
The kernels only exist for gfx950; CPU tensors are rejected by the callers.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSS2_LIB", os.path.join(_HERE, "libdss2_hip.so"))   # DSS2_LIB: diagnostic builds only

c_f32p = C.c_void_p   # all device pointers travel as integers (tensor.data_ptr())
c_i32p = C.c_void_p


class PackDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32),
                ("ld", C.c_int32), ("transpose", C.c_int32), ("koff", C.c_int32), ("kpad", C.c_int32),
                ("ncg", C.c_int32), ("joff", C.c_int32)]


class GemmPropArgs(C.Structure):
    _fields_ = [("X", C.c_void_p), ("ldx", C.c_int64), ("kreal", C.c_int32), ("kpad", C.c_int32),
                ("Bp", C.c_void_p), ("bias", C.c_void_p), ("rowscale", C.c_void_p),
                ("relu_src", C.c_void_p), ("ld_relu", C.c_int64),
                ("dmask", C.c_void_p), ("ld_dmask", C.c_int64),
                ("add_src", C.c_void_p), ("ld_add", C.c_int64),
                ("Y", C.c_void_p), ("ldy", C.c_int64), ("hout", C.c_int32), ("ncg", C.c_int32),
                ("relu", C.c_int32), ("nmat", C.c_int32), ("nrb", C.c_int32), ("ntiles", C.c_int32),
                ("tile_start", C.c_void_p),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("w", C.c_void_p),
                ("max_nnz", C.c_int32), ("ell_width", C.c_int32),
                ("prop_in", C.c_int32), ("narrow_h", C.c_int32),
                ("prebias", C.c_void_p), ("pre_rowscale", C.c_void_p), ("ell_tiles", C.c_void_p),
                ("drop_state", C.c_void_p), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float), ("drop_id", C.c_int32),
                ("b_format", C.c_int32), ("max_tile_rows", C.c_int32)]


class ChainEdge(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ea", C.c_void_p), ("W1", C.c_void_p), ("b1", C.c_void_p), ("ell_ent", C.c_void_p),
                ("S", C.c_void_p), ("slab", C.c_void_p), ("ldx", C.c_int64), ("ldea", C.c_int64), ("width", C.c_int32), ("pad", C.c_int32)]


class ChainHead(C.Structure):
    _fields_ = [("W", C.c_void_p * 4), ("bias", C.c_void_p), ("add_src", C.c_void_p), ("Y", C.c_void_p),
                ("G", C.c_void_p), ("gate", C.c_void_p), ("Xout", C.c_void_p),
                ("ld_add", C.c_int64), ("ldy", C.c_int64), ("ldg", C.c_int64), ("ld_gate", C.c_int64), ("ldxo", C.c_int64),
                ("nout", C.c_int32), ("mode", C.c_int32), ("drop_id", C.c_int32), ("pad", C.c_int32), ("wg_slab", C.c_void_p),
                ("edge", ChainEdge)]


class WgradArgs(C.Structure):
    _fields_ = [("G", C.c_void_p), ("ldg", C.c_int64), ("hout", C.c_int32),
                ("X", C.c_void_p), ("ldx", C.c_int64), ("hin", C.c_int32),
                ("rowscale", C.c_void_p),
                ("slab", C.c_void_p), ("n_split", C.c_int32), ("nmat", C.c_int32), ("nrb", C.c_int32),
                ("ntiles", C.c_int32),
                ("tile_start", C.c_void_p),
                ("rowptrT", C.c_void_p), ("colT", C.c_void_p), ("wT", C.c_void_p),
                ("max_nnz", C.c_int32), ("ell_width", C.c_int32), ("ell_tiles", C.c_void_p), ("rowscale2", C.c_void_p),
                ("narrow", C.c_int32), ("mfma_bf16", C.c_int32)]


class WgradPlan(C.Structure):
    """dss2_wgrad_plan_t: the kernel a weight-gradient launch runs and its geometry (include/dss2_hip.h)."""
    _fields_ = [("kernel", C.c_int32), ("reason", C.c_int32), ("nb", C.c_int32), ("w8", C.c_int32),
                ("grid_y", C.c_int32), ("z_groups", C.c_int32), ("y_slices", C.c_int32), ("f16x3_covers", C.c_int32),
                ("launch_lds", C.c_uint64), ("sizing_lds", C.c_uint64)]


class GemmPlan(C.Structure):
    """dss2_gemm_prop_plan_t: the kernel a single-layer tile GEMM + propagation launch runs and its geometry (include/dss2_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "reason", "row_split", "waves", "block", "pad_")] + [("lds_bytes", C.c_uint64), ("sizing_lds", C.c_uint64)]


GEMM_NONE, GEMM_NARROW_STREAM, GEMM_NARROW, GEMM_FP32, GEMM_FP32_KHALF, GEMM_BF16X6_KHALF = range(6)      # dss2_gemm_kernel


class ChainKernel(C.Structure):
    """dss2_chain_kernel_t: the layer chain's kernel for one weight format, its geometry and what it carries (include/dss2_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("family", "row_split", "waves", "block", "lds_bytes", "gate_words", "head_modes", "head_wgrad", "edge_modes")]


class ChainPlan(C.Structure):
    _fields_ = [("fmt", ChainKernel * 3)]      # by args.b_format: fp32, bf16x3, f16x2 weights


CHAIN_NONE, CHAIN_FP32, CHAIN_BF16X6, CHAIN_SP, CHAIN_SP6 = range(5)      # dss2_chain_family

# dss2_wgrad_kernel
(WGRAD_NONE, WGRAD_NARROW_STREAM, WGRAD_FP32_NARROW, WGRAD_FP32, WGRAD_BF16_64, WGRAD_BF16_32, WGRAD_BF16_TALL,
 WGRAD_F16_32, WGRAD_F16_TALL, WGRAD_F16_TALL_PAIR) = range(10)


class EdgeArgs(C.Structure):
    """dss2_edge_args: the operands of the edge MLP's forward / backward and the graph, as tiles with an entry table or as the CSR."""
    _fields_ = ([(n, C.c_void_p if t == "p" else C.c_int64) for n, t in zip(("x", "ldx", "ea", "ldea", "W1", "b1", "dS", "tile_start", "ell_ent"), "plplppppp")] +
                [(n, C.c_int32) for n in ("ell_width", "nrb", "ntiles", "pad_")] + [("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p),
                ("n_nodes", C.c_int64), ("S", C.c_void_p), ("slab", C.c_void_p), ("U", C.c_void_p), ("ldu", C.c_int64)] +
                [(n, C.c_int32) for n in ("n_slabs", "h", "fn", "fe", "bwd_with_u", "by_source")])


class EdgePass(C.Structure):
    """dss2_edge_pass_t: the kernel one pass of the edge MLP runs and its launch geometry (include/dss2_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("family", "nrb", "parts", "block", "wg_per_tile", "lds_bytes")]


class EdgePlan(C.Structure):
    _fields_ = [("fwd", EdgePass), ("bwd", EdgePass), ("bwd_src", EdgePass), ("pair_exact", C.c_int32), ("pad_", C.c_int32)]


EDGE_NONE, EDGE_CSR, EDGE_VALU, EDGE_VALU_HALF, EDGE_FP32_MFMA, EDGE_BF16X6 = range(6)      # dss2_edge_family


class CsrBuildArgs(C.Structure):
    _fields_ = [("edge_index", C.c_void_p), ("n_edges", C.c_int64), ("n_nodes", C.c_int64), ("doubled", C.c_int32), ("no_flip", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p), ("perm", C.c_void_p), ("w", C.c_void_p),
                ("rowptrT", C.c_void_p), ("colT", C.c_void_p), ("entT", C.c_void_p), ("permT", C.c_void_p), ("wT", C.c_void_p),
                ("inc_rowptr", C.c_void_p), ("inc_ent", C.c_void_p), ("efrom", C.c_void_p), ("eto", C.c_void_p),
                ("deg", C.c_void_p), ("lastcut", C.c_void_p), ("meta", C.c_void_p), ("work", C.c_void_p)]


class EllBuildArgs(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p), ("w", C.c_void_p),
                ("rowptrT", C.c_void_p), ("colT", C.c_void_p), ("entT", C.c_void_p), ("wT", C.c_void_p),
                ("tile_start", C.c_void_p), ("ntiles", C.c_int32), ("tm", C.c_int32), ("ell_width", C.c_int32),
                ("ellT_width", C.c_int32),
                ("ell_tiles", C.c_void_p), ("ell_ent_tiles", C.c_void_p), ("ellT_tiles", C.c_void_p),
                ("ellT_ent_tiles", C.c_void_p), ("meta", C.c_void_p), ("uniform_rows", C.c_int32), ("n_nodes", C.c_int64)]


PADDED_MAX_TILINGS = 4


class PaddedBuildArgs(C.Structure):
    _fields_ = [("csr", CsrBuildArgs), ("nodes_per_graph", C.c_int32), ("edge_stride", C.c_int32), ("edge_count", C.c_void_p),
                ("csr_ptr", C.c_void_p), ("edge_total", C.c_void_p), ("deg_pows", C.c_void_p), ("n_ell", C.c_int32), ("pad_", C.c_int32),
                ("ell", EllBuildArgs * PADDED_MAX_TILINGS)]


class CsrAxpyArgs(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("w", C.c_void_p), ("T", C.c_void_p), ("ldt", C.c_int64),
                ("add", C.c_void_p), ("ld_add", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64), ("bias", C.c_void_p),
                ("relu_src", C.c_void_p), ("ld_relu", C.c_int64), ("add_src", C.c_void_p), ("ld_src", C.c_int64),
                ("drop_state", C.c_void_p), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float), ("drop_id", C.c_int32),
                ("relu", C.c_int32), ("n_rows", C.c_int64), ("h", C.c_int32), ("pad_", C.c_int32)]


class ReduceDesc(C.Structure):
    _fields_ = [("slab", C.c_void_p), ("out", C.c_void_p), ("stride", C.c_int64), ("len", C.c_int64),
                ("n_slabs", C.c_int32), ("pad_", C.c_int32)]


class ChainLayer(C.Structure):
    _fields_ = [("Bp", C.c_void_p), ("bias", C.c_void_p), ("relu_src", C.c_void_p), ("dmask", C.c_void_p),
                ("add_src", C.c_void_p), ("prebias", C.c_void_p), ("Y", C.c_void_p), ("relu", C.c_int32), ("drop_id", C.c_int32),
                ("gate_bits", C.c_void_p), ("y_bits", C.c_void_p)]


class AdamaxDesc(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_inf", C.c_void_p), ("n", C.c_int64)]


class OptimHyper(C.Structure):
    """dss2_optim_hyper: rule, flags and hyper-parameters of one optimizer launch; lr_dev overrides lr when set (include/dss2_hip.h)."""
    _fields_ = ([("rule", C.c_int32), ("flags", C.c_int32)] +
                [(n, C.c_float) for n in ("lr", "beta1", "beta2", "omb1", "omb2", "eps", "weight_decay", "momentum", "omdamp")] +
                [("pad_", C.c_int32), ("lr_dev", C.c_void_p)])


OPT_ADAM, OPT_RMSPROP, OPT_SGD, OPT_ADAMAX = range(4)                                                   # dss2_optim_rule
OPT_AMSGRAD, OPT_DECOUPLED_WD, OPT_CENTERED, OPT_MOMENTUM, OPT_NESTEROV = 1, 2, 4, 8, 16          # dss2_optim_flag
OPTIM_GRAD_CHUNK, OPTIM_MAX_PARTIALS = 192, 256                                                         # dss2_grad_sqsum_partials


class OptimDesc(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("s0", C.c_void_p), ("s1", C.c_void_p), ("s2", C.c_void_p), ("n", C.c_int64)]


class OptimFlatDesc(C.Structure):
    """dss2_optim_flat_desc: a row of the DEVICE table of dss2_optim_step_flat (optim.py builds it through numpy)."""
    _fields_ = [("param", C.c_void_p), ("grad_off", C.c_int64), ("s0", C.c_void_p), ("s1", C.c_void_p), ("s2", C.c_void_p), ("n", C.c_int64)]


class AdamaxFlatDesc(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad_off", C.c_int64), ("exp_avg", C.c_void_p), ("exp_inf", C.c_void_p), ("n", C.c_int64)]


class GradDesc(C.Structure):
    _fields_ = [("grad", C.c_void_p), ("n", C.c_int64)]


class GradFlatDesc(C.Structure):
    _fields_ = [("grad_off", C.c_int64), ("n", C.c_int64)]


class CollateDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("chunk", C.c_int32), ("kind", C.c_int32),
                ("shared", C.c_int32), ("pad_", C.c_int32), ("nodes_per_sample", C.c_int64)]


class SgemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p * 4), ("B", C.c_void_p * 4), ("C", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("c_off", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32),
                ("ldc", C.c_int32), ("transA", C.c_int32), ("transB", C.c_int32), ("nbatch", C.c_int32),
                ("accumulate", C.c_int32)]


class WlsSolveArgs(C.Structure):
    """dss2_wls_solve_args (include/dss2_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("edge_attr", C.c_void_p), ("ldea", C.c_int64),
                ("x_mean", C.c_void_p), ("x_std", C.c_void_p), ("edge_mean", C.c_void_p), ("edge_std", C.c_void_p),
                ("efrom", C.c_void_p), ("eto", C.c_void_p), ("inc_rowptr", C.c_void_p), ("inc_ent", C.c_void_p),
                ("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("nodes_per_graph", C.c_int32), ("max_iter", C.c_int32),
                ("tol", C.c_double), ("w_v", C.c_double), ("w_p", C.c_double), ("w_pf", C.c_double),
                ("init", C.c_void_p), ("ld_init", C.c_int64), ("state", C.c_void_p), ("objective", C.c_void_p),
                ("iterations", C.c_void_p), ("status", C.c_void_p), ("last_step", C.c_void_p), ("vminmax", C.c_void_p),
                ("max_groups", C.c_int32), ("half_bandwidth", C.c_int32), ("graph_ptr", C.c_void_p), ("n_graphs", C.c_int64)]


class WlsBadDataArgs(C.Structure):
    """dss2_wls_bad_data_args (include/dss2_hip.h)."""
    _fields_ = [("solve", WlsSolveArgs), ("threshold", C.c_double), ("z_p", C.c_double), ("s_min", C.c_double),
                ("max_removals", C.c_int32), ("pad_", C.c_int32), ("bus_label", C.c_void_p), ("dof", C.c_void_p), ("chi2_limit", C.c_void_p),
                ("suspect", C.c_void_p), ("removed", C.c_void_p), ("removed_rn", C.c_void_p), ("n_removed", C.c_void_p),
                ("bus_rn", C.c_void_p), ("bus_sens", C.c_void_p), ("edge_rn", C.c_void_p), ("edge_sens", C.c_void_p),
                ("state_std", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


class WlsLargeArgs(C.Structure):
    """dss2_wls_large_args (include/dss2_hip.h)."""
    _fields_ = [("solve", WlsSolveArgs), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


WLS_BAND_BLOCK, WLS_BAND_GROUPS, WLS_BAND_LDS_BYTES = 16, 512, 160 * 1024      # the banded form of dss2_wls_solve_large
WLS_BAND_BAD_DATA_BYTES = 320                                                  # ... of dss2_wls_bad_data: its fixed LDS block behind the solve's


class WlsRobustArgs(C.Structure):
    """dss2_wls_robust_args (include/dss2_hip.h)."""
    _fields_ = [("solve", WlsSolveArgs), ("gamma", C.c_double), ("plain_iters", C.c_int32), ("pad_", C.c_int32),
                ("bus_q", C.c_void_p), ("edge_q", C.c_void_p), ("n_downweighted", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


class WlsArgs(C.Structure):
    _fields_ = [("input", C.c_void_p), ("ld_in", C.c_int64),
                ("edge_input", C.c_void_p), ("ld_ein", C.c_int64),
                ("output", C.c_void_p), ("ld_out", C.c_int64),
                ("node_param", C.c_void_p), ("ld_np", C.c_int64),
                ("edge_param", C.c_void_p), ("ld_ep", C.c_int64),
                ("x_mean", C.c_void_p), ("x_std", C.c_void_p),
                ("edge_mean", C.c_void_p), ("edge_std", C.c_void_p),
                ("efrom", C.c_void_p), ("eto", C.c_void_p),
                ("inc_rowptr", C.c_void_p), ("inc_ent", C.c_void_p),
                ("n_nodes", C.c_int64), ("n_edges", C.c_int64),
                ("lam_v", C.c_float), ("lam_p", C.c_float), ("lam_pf", C.c_float), ("lam_reg", C.c_float),
                ("sums", C.c_void_p), ("partials", C.c_void_p), ("vminmax", C.c_void_p),
                ("apq", C.c_void_p), ("loss", C.c_void_p), ("grad_output", C.c_void_p), ("pflow", C.c_void_p),
                ("flags", C.c_int32), ("counter", C.c_void_p), ("gscale", C.c_void_p), ("edge_count", C.c_void_p)]


WLS_VMM_CACHED, WLS_FUSED_FINISH, WLS_NO_LOSS_WRITE = 1, 2, 4


class StackDims(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_hh", C.c_int32), ("dout_inner", C.c_int32), ("dout_last", C.c_int32),
                ("skip_inner", C.c_int32), ("skip_last", C.c_int32)]


class StackArgs(C.Structure):
    _fields_ = [("dims", StackDims),
                ("x", C.c_void_p), ("ldx", C.c_int64), ("ea", C.c_void_p), ("ldea", C.c_int64), ("wpack", C.c_void_p),
                ("tile_start", C.c_void_p), ("ntiles", C.c_int32), ("tm", C.c_int32),
                ("ell_w", C.c_void_p), ("ell_e", C.c_void_p), ("ell_width", C.c_int32),
                ("ellT_w", C.c_void_p), ("ellT_e", C.c_void_p), ("ellT_width", C.c_int32),
                ("deg_pows", C.c_void_p), ("eacache", C.c_void_p), ("xs", C.c_void_p), ("acts", C.c_void_p),
                ("out", C.c_void_p), ("ldo", C.c_int64), ("gout", C.c_void_p), ("ldg", C.c_int64),
                ("dxbuf", C.c_void_p), ("dx_out", C.c_void_p),
                ("slab", C.c_void_p), ("slab_stride", C.c_int64), ("n_wg", C.c_int32),
                ("drop_state", C.c_void_p), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float), ("drop_stride", C.c_int32),
                ("n_nodes", C.c_int64)]


class LanegroupHead(C.Structure):
    _fields_ = [("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p), ("hin", C.c_void_p),
                ("ldhin", C.c_int64), ("z1", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int64), ("gout", C.c_void_p),
                ("ldgo", C.c_int64), ("dz1", C.c_void_p), ("c", C.c_int32), ("dense", C.c_int32), ("nout", C.c_int32),
                ("pad_", C.c_int32)]


LANEGROUP_WGRAD_MAX_JOBS = 16


class LanegroupWgradJob(C.Structure):
    _fields_ = [("G", C.c_void_p), ("ldg", C.c_int64), ("X", C.c_void_p), ("ldx", C.c_int64), ("gw", C.c_int32),
                ("xw", C.c_int32), ("col", C.c_int32), ("pad_", C.c_int32)]


class LanegroupWgradArgs(C.Structure):
    _fields_ = [("jobs", LanegroupWgradJob * LANEGROUP_WGRAD_MAX_JOBS), ("slab", C.c_void_p), ("n_nodes", C.c_int64),
                ("n_slabs", C.c_int32), ("slab_len", C.c_int32), ("n_jobs", C.c_int32), ("pad_", C.c_int32)]


class GatGraph(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p), ("rowptrT", C.c_void_p), ("colT", C.c_void_p),
                ("entT", C.c_void_p), ("ea", C.c_void_p), ("ldea", C.c_int64), ("n_nodes", C.c_int64), ("ed", C.c_int32),
                ("add_self_loops", C.c_int32), ("slope", C.c_float), ("nonlin", C.c_int32), ("slab", C.c_void_p),
                ("n_slabs", C.c_int32), ("slab_len", C.c_int32)]


class GatConv(C.Structure):
    _fields_ = [("att", C.c_void_p), ("bias", C.c_void_p), ("Wl", C.c_void_p), ("bl", C.c_void_p), ("Wr", C.c_void_p),
                ("br", C.c_void_p), ("We", C.c_void_p), ("h", C.c_void_p), ("ldh", C.c_int64), ("y", C.c_void_p),
                ("m", C.c_void_p), ("s", C.c_void_p), ("dxl", C.c_void_p), ("dxr", C.c_void_p), ("dedge", C.c_void_p),
                ("dself", C.c_void_p), ("cin", C.c_int32), ("cout", C.c_int32), ("slab_off", C.c_int32), ("heads", C.c_int32),
                ("concat", C.c_int32), ("pad_", C.c_int32)]


class GatArgs(C.Structure):
    _fields_ = [("g", GatGraph), ("up", GatConv), ("lo", GatConv), ("head", LanegroupHead), ("has_up", C.c_int32),
                ("has_lo", C.c_int32), ("has_head", C.c_int32), ("group", C.c_int32), ("gy", C.c_void_p), ("ldgy", C.c_int64),
                ("dh", C.c_void_p), ("dh_cols", C.c_int32), ("pad_", C.c_int32)]


class GineGraph(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p), ("rowptrT", C.c_void_p), ("colT", C.c_void_p),
                ("entT", C.c_void_p), ("ea", C.c_void_p), ("ldea", C.c_int64), ("n_nodes", C.c_int64), ("ed", C.c_int32),
                ("nonlin", C.c_int32), ("slab", C.c_void_p), ("n_slabs", C.c_int32), ("slab_len", C.c_int32),
                ("nslab", C.c_void_p), ("nslab_len", C.c_int32), ("pad_", C.c_int32)]


class GineConv(C.Structure):
    _fields_ = [("eps", C.c_void_p), ("Wn", C.c_void_p), ("bn", C.c_void_p), ("We", C.c_void_p), ("be", C.c_void_p),
                ("h", C.c_void_p), ("ldh", C.c_int64), ("y", C.c_void_p), ("z", C.c_void_p), ("dz", C.c_void_p),
                ("cin", C.c_int32), ("cout", C.c_int32), ("slab_off", C.c_int32), ("nn_off", C.c_int32)]


class GineArgs(C.Structure):
    _fields_ = [("g", GineGraph), ("up", GineConv), ("lo", GineConv), ("head", LanegroupHead), ("has_up", C.c_int32),
                ("has_lo", C.c_int32), ("has_head", C.c_int32), ("group", C.c_int32), ("gy", C.c_void_p), ("ldgy", C.c_int64),
                ("dh", C.c_void_p), ("dh_cols", C.c_int32), ("pad_", C.c_int32)]


GNN_GCN2, GNN_FA, GNN_TAG = 1, 2, 3
GNN_MAX_K = 4


class GnnGraph(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p), ("rowptrT", C.c_void_p), ("colT", C.c_void_p),
                ("entT", C.c_void_p), ("dis", C.c_void_p), ("n_nodes", C.c_int64), ("ed", C.c_int32), ("loops", C.c_int32),
                ("nonlin", C.c_int32), ("pad_", C.c_int32), ("slab", C.c_void_p), ("n_slabs", C.c_int32), ("slab_len", C.c_int32)]


class GnnConv(C.Structure):
    _fields_ = [("kind", C.c_int32), ("K", C.c_int32), ("W", C.c_void_p * (GNN_MAX_K + 1)), ("bias", C.c_void_p),
                ("h", C.c_void_p), ("ldh", C.c_int64), ("x0", C.c_void_p), ("ldx0", C.c_int64), ("param", C.c_float),
                ("c", C.c_int32), ("y", C.c_void_p), ("u", C.c_void_p), ("d", C.c_void_p), ("se", C.c_void_p), ("sn", C.c_void_p),
                ("part", C.c_void_p), ("slab_off", C.c_int32), ("pad_", C.c_int32)]


class GnnArgs(C.Structure):
    _fields_ = [("g", GnnGraph), ("up", GnnConv), ("lo", GnnConv), ("head", LanegroupHead), ("has_up", C.c_int32),
                ("has_lo", C.c_int32), ("has_head", C.c_int32), ("group", C.c_int32), ("hop", C.c_int32), ("dx0_first", C.c_int32),
                ("rin", C.c_void_p), ("rout", C.c_void_p), ("gy", C.c_void_p), ("ldgy", C.c_int64), ("dh", C.c_void_p),
                ("dh_cols", C.c_int32), ("pad_", C.c_int32), ("dx0", C.c_void_p)]


CHEB_MAX_K, CHEB_MAX_CONVS = 4, 4


class ChebGraph(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("ent", C.c_void_p), ("perm", C.c_void_p), ("rowptrT", C.c_void_p),
                ("colT", C.c_void_p), ("entT", C.c_void_p), ("permT", C.c_void_p), ("efrom", C.c_void_p), ("eto", C.c_void_p),
                ("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("n_rows", C.c_int64), ("ed", C.c_int32), ("n_convs", C.c_int32),
                ("w", C.c_void_p), ("what", C.c_void_p), ("dn", C.c_void_p), ("lam", C.c_void_p), ("arg", C.c_void_p),
                ("slab", C.c_void_p), ("n_slabs", C.c_int32), ("slab_len", C.c_int32)]


class ChebLayer(C.Structure):
    _fields_ = [("W", (C.c_void_p * CHEB_MAX_K) * CHEB_MAX_CONVS), ("bias", C.c_void_p * CHEB_MAX_CONVS), ("h", C.c_void_p),
                ("ldh", C.c_int64), ("y", C.c_void_p), ("T", C.c_void_p), ("dv", C.c_void_p), ("r", C.c_void_p * 2),
                ("cin", C.c_int32), ("cout", C.c_int32), ("K", C.c_int32), ("relu", C.c_int32), ("drop_id", C.c_int32),
                ("pad_", C.c_int32)]


class ChebArgs(C.Structure):
    _fields_ = [("g", ChebGraph), ("up", ChebLayer), ("lo", ChebLayer), ("head", LanegroupHead), ("has_up", C.c_int32),
                ("has_lo", C.c_int32), ("has_head", C.c_int32), ("group", C.c_int32), ("hop", C.c_int32), ("acc_first", C.c_int32),
                ("gy", C.c_void_p), ("ldgy", C.c_int64), ("dh", C.c_void_p), ("dh_cols", C.c_int32), ("pad_", C.c_int32),
                ("dwh", C.c_void_p), ("ddn", C.c_void_p), ("drop_state", C.c_void_p), ("drop_thr", C.c_uint32),
                ("drop_scale", C.c_float)]


class ChebEdgeArgs(C.Structure):
    _fields_ = [("g", ChebGraph), ("ea", C.c_void_p), ("ldea", C.c_int64), ("W1", C.c_void_p), ("b1", C.c_void_p),
                ("W2", C.c_void_p), ("b2", C.c_void_p), ("w_in", C.c_void_p), ("ldw", C.c_int64), ("has_mlp", C.c_int32),
                ("hid", C.c_int32), ("lambda_given", C.c_int32), ("lambda_", C.c_float), ("n_wg", C.c_int32), ("zero_in", C.c_int32),
                ("pmax", C.c_void_p), ("parg", C.c_void_p), ("psum", C.c_void_p), ("dwh", C.c_void_p), ("ddn", C.c_void_p),
                ("dw", C.c_void_p), ("dz1", C.c_void_p), ("a1", C.c_void_p)]


# Every struct type of include/dss2_hip.h (the opaque dss2_plan aside) and its mirror.  A field carries the C member's name (lambda_:
# `lambda` is a Python keyword) and every upper-case integer constant X of this module is the header's DSS2_X: tests/test_abi_cpu.py
# compiles the header and holds layouts, field types, the signatures below and the constants to it.
C_STRUCTS = {
    "dss2_csr_build_args": CsrBuildArgs, "dss2_ell_build_args": EllBuildArgs, "dss2_padded_build_args": PaddedBuildArgs,
    "dss2_pack_desc": PackDesc, "dss2_edge_args": EdgeArgs, "dss2_edge_pass_t": EdgePass, "dss2_edge_plan_t": EdgePlan,
    "dss2_gemm_prop_args": GemmPropArgs, "dss2_gemm_prop_plan_t": GemmPlan, "dss2_chain_layer": ChainLayer,
    "dss2_chain_edge": ChainEdge, "dss2_chain_head": ChainHead, "dss2_chain_kernel_t": ChainKernel, "dss2_chain_plan_t": ChainPlan,
    "dss2_csr_axpy_args": CsrAxpyArgs, "dss2_wgrad_args": WgradArgs, "dss2_wgrad_plan_t": WgradPlan, "dss2_reduce_desc": ReduceDesc,
    "dss2_wls_args": WlsArgs, "dss2_wls_solve_args": WlsSolveArgs, "dss2_wls_bad_data_args": WlsBadDataArgs,
    "dss2_wls_large_args": WlsLargeArgs, "dss2_wls_robust_args": WlsRobustArgs, "dss2_sgemm_desc": SgemmDesc,
    "dss2_collate_desc": CollateDesc, "dss2_stack_dims": StackDims, "dss2_stack_args": StackArgs, "dss2_optim_hyper": OptimHyper,
    "dss2_optim_desc": OptimDesc, "dss2_optim_flat_desc": OptimFlatDesc, "dss2_adamax_desc": AdamaxDesc,
    "dss2_adamax_flat_desc": AdamaxFlatDesc, "dss2_grad_desc": GradDesc, "dss2_grad_flat_desc": GradFlatDesc,
    "dss2_lanegroup_head": LanegroupHead, "dss2_lanegroup_wgrad_job": LanegroupWgradJob, "dss2_lanegroup_wgrad_args": LanegroupWgradArgs,
    "dss2_gat_graph": GatGraph, "dss2_gat_conv": GatConv, "dss2_gat_args": GatArgs,
    "dss2_gine_graph": GineGraph, "dss2_gine_conv": GineConv, "dss2_gine_args": GineArgs,
    "dss2_gnn_graph": GnnGraph, "dss2_gnn_conv": GnnConv, "dss2_gnn_args": GnnArgs,
    "dss2_cheb_graph": ChebGraph, "dss2_cheb_layer": ChebLayer, "dss2_cheb_args": ChebArgs, "dss2_cheb_edge_args": ChebEdgeArgs,
}

_SIGNATURES = {
    # name: (restype, argtypes)
    "dss2_last_error": (C.c_char_p, []),
    "dss2_version": (C.c_int, []),
    "dss2_debug_chain_clock_probe": (None, [C.c_void_p]),
    "dss2_plan_begin": (C.c_int, [C.POINTER(C.c_void_p)]),
    "dss2_plan_end": (C.c_int, [C.c_void_p]),
    "dss2_plan_size": (C.c_int, [C.c_void_p]),
    "dss2_plan_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dss2_plan_destroy": (None, [C.c_void_p]),
    "dss2_topology_probe": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dss2_csr_build": (C.c_int, [C.POINTER(CsrBuildArgs), C.c_void_p]),
    "dss2_csr_build_work_ints": (C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    "dss2_tiles_uniform": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p]),
    "dss2_tiles_walk": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "dss2_ell_tiles_build": (C.c_int, [C.POINTER(EllBuildArgs), C.c_void_p]),
    "dss2_deg_pows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_segment_sum": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_int64, C.c_int, C.c_void_p]),
    "dss2_gather_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "dss2_rng_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "dss2_dropout_mask": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dss2_gate_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int32, C.c_float, C.c_int,
                                 C.c_void_p]),
    "dss2_dropout_params": (None, [C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "dss2_csr_axpy": (C.c_int, [C.POINTER(CsrAxpyArgs), C.c_void_p]),
    "dss2_pack_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dss2_edge_fwd": (C.c_int, [C.POINTER(EdgeArgs), C.c_void_p]),
    "dss2_edge_bwd": (C.c_int, [C.POINTER(EdgeArgs), C.c_void_p]),
    "dss2_edge_plan": (C.c_int, [C.c_int] * 5 + [C.POINTER(EdgePlan)]),
    "dss2_edge_combine_fwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "dss2_edge_combine_bwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p]),
    "dss2_gemm_prop": (C.c_int, [C.POINTER(GemmPropArgs), C.c_void_p]),
    "dss2_gemm_prop_plan": (C.c_int, [C.POINTER(GemmPropArgs), C.POINTER(GemmPlan)]),
    "dss2_chain_sp6_single_group_min_tiles": (C.c_int, []),
    "dss2_gemm_prop_chain": (C.c_int, [C.POINTER(GemmPropArgs), C.c_void_p, C.c_int, C.c_void_p]),
    "dss2_gemm_prop_chain_head": (C.c_int, [C.POINTER(GemmPropArgs), C.c_void_p, C.c_int, C.POINTER(ChainHead), C.c_void_p]),
    "dss2_gemm_prop_chain_plan": (C.c_int, [C.c_int] * 7 + [C.POINTER(ChainPlan)]),
    "dss2_gemm_prop_chain_head_supported": (C.c_int, [C.c_int] * 6),
    "dss2_gemm_prop_chain_head_wgrad_supported": (C.c_int, [C.c_int] * 6),
    "dss2_gemm_prop_chain_edge_supported": (C.c_int, [C.c_int] * 6),
    "dss2_gemm_prop_chain_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_gemm_prop_chain16_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_gemm_prop_chain_f16_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_gemm_prop_chain_gate_words": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_gemm_prop16_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_wgrad": (C.c_int, [C.POINTER(WgradArgs), C.c_void_p]),
    "dss2_wgrad_plan": (C.c_int, [C.POINTER(WgradArgs), C.c_int, C.POINTER(WgradPlan)]),
    "dss2_wgrad_batched": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "dss2_reduce_slabs_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "dss2_reduce_slabs": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "dss2_wls_loss_partials": (C.c_int, [C.POINTER(WlsArgs), C.c_void_p]),
    "dss2_wls_loss_grad": (C.c_int, [C.POINTER(WlsArgs), C.c_void_p]),
    "dss2_wls_loss_value": (C.c_int, [C.POINTER(WlsArgs), C.c_void_p]),
    "dss2_get_pflow": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_void_p]),
    "dss2_eval_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_eval_scratch_doubles": (C.c_int64, []),
    "dss2_wls_solve": (C.c_int, [C.POINTER(WlsSolveArgs), C.c_void_p]),
    "dss2_wls_solve_lds_bytes": (C.c_size_t, [C.c_int]),
    "dss2_wls_bad_data": (C.c_int, [C.POINTER(WlsBadDataArgs), C.c_void_p]),
    "dss2_wls_bad_data_lds_bytes": (C.c_size_t, [C.c_int]),
    "dss2_wls_solve_large": (C.c_int, [C.POINTER(WlsLargeArgs), C.c_void_p]),
    "dss2_wls_large_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "dss2_wls_large_groups": (C.c_int64, [C.POINTER(WlsSolveArgs)]),
    "dss2_wls_large_max_nodes": (C.c_int, []),
    "dss2_wls_large_lds_bytes": (C.c_size_t, [C.c_int]),
    "dss2_wls_robust": (C.c_int, [C.POINTER(WlsRobustArgs), C.c_void_p]),
    "dss2_wls_robust_large": (C.c_int, [C.POINTER(WlsRobustArgs), C.c_void_p]),
    "dss2_small_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dss2_measure_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.c_void_p, C.c_int64, C.c_void_p]),
    "dss2_measure_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    "dss2_masked_zscore": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_masked_zscore_scratch_doubles": (C.c_int64, [C.c_int64]),
    "dss2_collate": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "dss2_csr_build_graphs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "dss2_csr_build_graphs_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "dss2_csr_build_padded": (C.c_int, [C.POINTER(PaddedBuildArgs), C.c_void_p]),
    "dss2_collate_cursor": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "dss2_accum_scalar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_collate_ragged_multi": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "dss2_collate_ragged": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "dss2_adamax_step": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "dss2_adamax_step_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "dss2_stack_wpack_words": (C.c_int64, [C.POINTER(StackDims)]),
    "dss2_stack_flat_floats": (C.c_int64, [C.POINTER(StackDims)]),
    "dss2_stack_supported": (C.c_int, [C.POINTER(StackDims), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_stack_pack": (C.c_int, [C.POINTER(StackDims), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_stack_forward": (C.c_int, [C.POINTER(StackArgs), C.c_void_p]),
    "dss2_stack_backward": (C.c_int, [C.POINTER(StackArgs), C.c_void_p]),
    "dss2_stack_reduce": (C.c_int, [C.POINTER(StackDims), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_stack_fold_scratch_floats": (C.c_int64, [C.POINTER(StackDims)]),
    "dss2_adamax_step_flat": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dss2_optim_step": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(OptimHyper), C.c_int, C.c_void_p]),
    "dss2_optim_step_dev": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(OptimHyper), C.c_void_p, C.c_void_p]),
    "dss2_optim_step_flat": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.POINTER(OptimHyper), C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "dss2_grad_sqsum_partials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dss2_grad_clip_scale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "dss2_gemm_prop_lds_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_wgrad_batched_groups": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_wgrad_y_slices": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_wgrad_lds_bytes_ex": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_wgrad_lds_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dss2_gat_forward": (C.c_int, [C.POINTER(GatArgs), C.c_void_p]),
    "dss2_gat_backward": (C.c_int, [C.POINTER(GatArgs), C.c_void_p]),
    "dss2_lanegroup_wgrad": (C.c_int, [C.POINTER(LanegroupWgradArgs), C.c_void_p]),
    "dss2_gine_forward": (C.c_int, [C.POINTER(GineArgs), C.c_void_p]),
    "dss2_gine_backward": (C.c_int, [C.POINTER(GineArgs), C.c_void_p]),
    "dss2_gnn_forward": (C.c_int, [C.POINTER(GnnArgs), C.c_void_p]),
    "dss2_gnn_backward": (C.c_int, [C.POINTER(GnnArgs), C.c_void_p]),
    "dss2_gnn_dis": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "dss2_cheb_edge_forward": (C.c_int, [C.POINTER(ChebEdgeArgs), C.c_void_p]),
    "dss2_cheb_edge_backward": (C.c_int, [C.POINTER(ChebEdgeArgs), C.c_void_p]),
    "dss2_cheb_forward": (C.c_int, [C.POINTER(ChebArgs), C.c_void_p]),
    "dss2_cheb_backward": (C.c_int, [C.POINTER(ChebArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libdss2_hip.so in-tree with hipcc --offload-arch=gfx950 (works without a GPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    res = subprocess.run(["bash", script], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"building libdss2_hip.so failed:\n{res.stdout}\n{res.stderr}")
    if verbose:
        print(res.stdout.strip())
    return LIB_PATH


def lib():
    """The loaded library with typed signatures.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the DSS2 HIP kernels are not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


_RAW_STREAM = None


def stream_ptr(device) -> int:
    """hipStream_t of torch's current stream on `device` as an integer.  torch._C._cuda_getCurrentRawStream is the call
    torch's own compiled-kernel launchers use: ~0.3 us against ~5 us for torch.cuda.current_stream(device).cuda_stream,
    which a step pays 14 times."""
    global _RAW_STREAM
    if _RAW_STREAM is None:
        import torch
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        _RAW_STREAM = raw if raw is not None else (lambda idx: torch.cuda.current_stream(idx).cuda_stream)
    if isinstance(device, int):
        idx = device
    else:
        import torch
        idx = (device if isinstance(device, torch.device) else torch.device(device)).index
        if idx is None:
            idx = torch.cuda.current_device()
    return _RAW_STREAM(idx)


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().dss2_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
