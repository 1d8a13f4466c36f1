"""GPU: the two propagation hops of the f16x3 weight gradient as products on the matrix pipe (csrc/dss2_wgrad16h.hip, HM = true;
flags.WGRAD_HOPS_MFMA, DSS2_WGRAD_HOPS_MFMA) against the gathered fp32 hops (switch off: the kernel as it was).

dW_m = (P^m G)^T X and db = colsum(G) of the three-layer launch (the folded layer and two plain ones) are compared with fp64 torch on the
same operands.  The yardstick is the switch-off route's own max-normalised error against that oracle, worst over the case's layers and
matrices: every dW_m of the new route may be at most 4 x that and never above the project's 1e-5 parity bar -- an f16x3 product carries
2^-22 relative error and the two chained hops add two such roundings to what the contraction over the rows already has.  db and the
folded layer's scaled bias sums never see the hops: bit-identical between the routes.  Same inputs, same bits, call after call.

Both errors are printed per case (pytest -s shows them; profiles/wgrad_hops_mfma_errors.txt keeps a run)."""
import importlib

import pytest
import torch

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, NMAT = 128, 3


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


def _topo(pkg, grids, B, seed, parallel=False):
    b = pkg.synthetic.make_batch(grids, B, seed=seed)
    ei = b["edge_index"]
    if parallel:      # every third branch a second time: rows of P with two entries for one neighbour (and ELL slices wider than four)
        ei = torch.cat([ei, ei[:, ::3]], dim=1)
    return pkg.topology.get_topology(ei.to(DEV), b["x"].shape[0])


def _oracle(topo, G, X):
    N = topo.N
    rp, col, w = topo.rowptrT.cpu().long(), topo.colT.cpu().long(), topo.wT.cpu().double()
    rows = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    P = torch.sparse_coo_tensor(torch.stack([rows, col]), w, (N, N)).to(DEV)
    Z, out = G.double(), []
    for m in range(NMAT):
        if m:
            Z = torch.sparse.mm(P, Z)
        out.append(Z.t() @ X.double())
    return out, G.double().sum(0)


def _run(pkg, topo, Gs, Xs, hops_mfma):
    """The three-layer launch of the C2 backward: layer 0 folded (scaled bias sums), two plain layers."""
    stride = NMAT * H * H + H
    out = torch.full((2 * stride,), float("nan"), device=DEV)
    first = torch.full((stride + NMAT * H,), float("nan"), device=DEV)
    old = pkg.flags.WGRAD_HOPS_MFMA
    try:
        pkg.flags.WGRAD_HOPS_MFMA = hops_mfma
        pkg.ops.wgrad_batched(topo, Gs, H, Xs, H, NMAT, out, first_rowscale2=topo.deg_pows, first_out=first)
    finally:
        pkg.flags.WGRAD_HOPS_MFMA = old
    torch.cuda.synchronize()
    return [first, out[:stride], out[stride:]]


def _errors(res, refs):
    """max |dW_m - oracle| / max |oracle| per (layer, matrix)"""
    errs = {}
    for l, (dW, _) in enumerate(refs):
        for m in range(NMAT):
            g = res[l][m * H * H:(m + 1) * H * H].view(H, H).double()
            errs[(l, m)] = (g - dW[m]).abs().max().item() / max(dW[m].abs().max().item(), 1e-300)
    return errs


def _takes_the_kernel(pkg, topo):
    ts = pkg.ops._wgrad_tiles(topo, NMAT, H, H, 1)
    return pkg.ops._wgrad_shape_plan(ts, NMAT, H, H, pkg.ops._wgrad_mode(ts, NMAT, 1)).kernel == pkg._lib.WGRAD_F16_32


CASES = {
    # name: (grids, B, per-layer scale of G)
    "cigre14": (["cigre14"], 1024, (0.1, 1.0, 10.0)),
    "mixed": (["cigre14", "cigre14_reswitched"], 333, (0.1, 1.0, 10.0)),
    "padded_last_tile": (["cigre14"], 77, (0.1, 1.0, 10.0)),            # 77 graphs, two per 32-row tile: the last tile holds one
    "layers_2^12_apart": (["cigre14"], 512, (2.0 ** -12, 1.0, 2.0 ** 12)),   # the running exponent Eg is per layer; hb must still cover the hops
    "layers_2^12_apart_falling": (["cigre14"], 512, (2.0 ** 12, 1.0, 2.0 ** -12)),
    "parallel_branches": (["cigre14"], 300, (0.1, 1.0, 10.0)),           # repeated (row, neighbour) pairs are summed before P is split
}


@pytest.mark.parametrize("name", list(CASES))
def test_hops_on_the_matrix_pipe_against_fp64_and_the_gathered_hops(pkg, name):
    grids, B, gscale = CASES[name]
    topo = _topo(pkg, grids, B, seed=31, parallel=(name == "parallel_branches"))
    assert _takes_the_kernel(pkg, topo), "cigre14 batches run the 32-row f16x3 weight gradient"
    N = topo.N
    torch.manual_seed(41)
    Xs = [torch.relu(torch.randn(N, H, device=DEV)) * (3.0 ** l) for l in range(3)]
    Gs = [torch.randn(N, H, device=DEV) * s for s in gscale]
    refs = [_oracle(topo, G, X) for G, X in zip(Gs, Xs)]
    off = _run(pkg, topo, Gs, Xs, False)
    on = _run(pkg, topo, Gs, Xs, True)
    again = _run(pkg, topo, Gs, Xs, True)
    e_off, e_on = _errors(off, refs), _errors(on, refs)
    ref_err = max(e_off.values())
    print(f"\nwgrad hops [{name}]: gathered fp32 hops max-normalised error {ref_err:.3e}, matrix-pipe hops {max(e_on.values()):.3e}"
          f"  (per matrix, worst layer: " + ", ".join(f"m={m}: {max(e_off[(l, m)] for l in range(3)):.2e} -> {max(e_on[(l, m)] for l in range(3)):.2e}"
                                                      for m in range(NMAT)) + ")")
    stride = NMAT * H * H + H
    for l in range(3):
        assert torch.isfinite(on[l]).all()
        # what the hops do not touch: dW_0, db, the folded layer's scaled bias sums -- same bits
        assert torch.equal(on[l][:H * H], off[l][:H * H]), l
        assert torch.equal(on[l][NMAT * H * H:], off[l][NMAT * H * H:]), l
        db = refs[l][1]
        assert (on[l][NMAT * H * H:stride].double() - db).abs().max().item() <= 2e-6 * max(db.abs().max().item(), 1e-300)
        assert torch.equal(on[l], again[l]), l      # same inputs, same bits
    for key, e in e_on.items():
        assert e <= 4.0 * ref_err, (key, e, ref_err)
        assert e <= 1e-5, (key, e)
