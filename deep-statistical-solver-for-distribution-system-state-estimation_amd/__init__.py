"""MI355X-native (gfx950) implementation of the DSS2 message-passing + WLS-loss hot path.

Drop-in modules ``networks`` (EdgeAggregation, TAGConv, MPN, SkipMPN, PFN, SkipPFN, GATv2Conv, GAT_DSSE, GINEConv, GINE_DSSE, GCN2Conv, FAConv, gnn_dsse, ChebConv, WrappedMultiConv, MultiConvNet) and ``data``
(gsp_wls_edge, get_pflow) mirror /root/reference/networks.py and /root/reference/data.py for the
path BASELINE.json names; everything below them is hand-written HIP in libdss2_hip.so.
"""
from . import _lib, flags, synthetic, topology  # noqa: F401
from . import ops, plans, route  # noqa: F401
from . import networks, data, parallel, graphs, optim, dataset  # noqa: F401
from .optim import FusedAdamax, FusedAdam, FusedAdamW, FusedRMSprop, FusedSGD  # noqa: F401
from . import estimator  # noqa: F401
from . import runner, multi  # noqa: F401
from .multi import MaskEmbdMPN, MultiMPN, MaskEmbdMultiMPN, MaskEmbdMultiMPN_NoMP, EdgeAggregationGeneral  # noqa: F401
from .networks import EdgeAggregation, TAGConv, MPN, SkipMPN, PFN, SkipPFN, MessagePassing  # noqa: F401
from .gat import GATv2Conv, GAT_DSSE  # noqa: F401
from .gine import GINEConv, GINE_DSSE  # noqa: F401
from .gnn import GCN2Conv, FAConv, gnn_dsse  # noqa: F401
from .cheb import ChebConv, WrappedMultiConv, MultiConvNet  # noqa: F401
from .data import gsp_wls_edge, get_pflow  # noqa: F401
from .estimator import wls_estimate_banded, wls_bad_data_banded, wls_robust_banded, band_order, BandOrder  # noqa: F401
from .estimator import wls_estimate, wls_estimate_large, WLSResult, wls_bad_data, wls_bad_data_large, WLSBadDataResult, wls_robust, WLSRobustResult  # noqa: F401
from .dataset import data_from_pickles, DataLoader, DeviceDataset, MixedDataset  # noqa: F401

__all__ = ["MaskEmbdMPN", "MultiMPN", "MaskEmbdMultiMPN", "MaskEmbdMultiMPN_NoMP", "EdgeAggregationGeneral", "EdgeAggregation", "TAGConv", "MPN", "SkipMPN", "PFN", "SkipPFN", "MessagePassing", "GATv2Conv", "GAT_DSSE", "GINEConv", "GINE_DSSE", "GCN2Conv", "FAConv", "gnn_dsse", "ChebConv", "WrappedMultiConv", "MultiConvNet",
           "gsp_wls_edge", "get_pflow", "wls_estimate", "wls_estimate_large", "wls_estimate_banded", "wls_bad_data_banded", "wls_robust_banded", "band_order", "BandOrder", "WLSResult", "wls_bad_data", "wls_bad_data_large", "WLSBadDataResult", "wls_robust", "WLSRobustResult", "estimator", "data_from_pickles", "DataLoader", "DeviceDataset", "MixedDataset", "FusedAdamax", "FusedAdam", "FusedAdamW", "FusedRMSprop", "FusedSGD", "dataset", "networks", "data", "parallel", "graphs", "optim", "synthetic",
           "topology", "flags", "ops", "plans", "gat", "gine", "gnn", "cheb"]
