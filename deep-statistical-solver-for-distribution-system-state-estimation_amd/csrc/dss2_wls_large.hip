// The batched WLS state estimator of dss2_wls_solve.hip for graphs whose gain matrix does not fit into LDS, fp64, gfx950: the same
// measurement model, Gauss-Newton iteration, outputs and decisions (dss2_wls_core.hpp: the row owners' assembly, the decision, the
// objective), one workgroup of 256 threads per graph, the whole iteration in ONE launch -- with G in global memory and a blocked
// factorisation.
//
//   workspace (global, one slice per workgroup; the workgroups stride over the graphs)
//         A   rows 0 .. ns - 1: the lower triangle of G;  row ns: the right-hand side b.  Row r lies in block row R = r / 16 and has
//             16 (R + 1) entries (its columns 0 .. r and padding up to the end of its diagonal block), rows one after the other:
//             wl_row_off(r) = 256 R (R + 1) / 2 + (r % 16) 16 (R + 1).  Every 16 x 16 block is 16 rows of 128 contiguous bytes.
//   LDS   Pt  the panel of the current block column, TRANSPOSED: Pt[j][i] = L[i, j0 + j] for the rows i below the diagonal block
//             (stride S = ns + 1 rounded up to 8; the row index is the absolute one)                          16 S doubles
//         Ld  the factorised diagonal block, invd the reciprocals of its diagonal                              256 + 16
//         u, du, ctl, slk as in the LDS kernel
//
//   per iteration
//     1. A <- 0 (coalesced), then thread r OWNS row r and b[r] (ws_accumulate_row_at on the global row; ns > 256: several rows each).
//     2. Blocked right-looking Cholesky WITH the b row, per block column of 16 (j0 .. j1):
//          a. wave 0 takes the diagonal block into registers (lane i holds row i), factorises it with the pivot test -- every value
//             another lane needs comes through v_readlane, no LDS round trip, no barrier -- and writes it to A, Ld and invd;
//          b. thread i solves row i of the panel (rows j1 .. ns, the b row among them) against Ld in registers and writes it to A and Pt;
//          c. the trailing update A[i, c] -= sum_j Pt[j][i] Pt[j][c] on 8 x 8 register tiles over the lower triangle of tiles, plain
//             v_fma_f64: per j a thread reads 8 + 8 doubles from LDS for 64 multiply-adds.
//        Three barriers per block column (3 ns / 16 per factorisation against the LDS kernel's 2 ns), none inside a step.
//     3. Blocked back substitution L^T du = y (y = the b row): wave 0 solves the diagonal block (lane c owns column c, v_readlane),
//        then thread c owns du[c] for the columns left of the block and reads rows of A coalesced.  Two barriers per block.
//     4. ws_decide, as in the LDS kernel.
//
// A pivot <= 0 or not finite only clears `ok` (wave 0's; thread 0 decides) and is replaced by 1: every loop runs to its fixed end.
// Every __syncthreads() sits in control flow that is uniform over the workgroup.  Global memory written by one thread and read by
// another of the same workgroup is separated by a barrier (all waves of a workgroup share their CU's vector cache).
// No atomics, one writer per value, fixed summation orders; a slice's contents before a graph do not matter (A is zeroed, Pt, Ld are
// written before they are read; what is read from Pt beyond row ns only reaches tile entries that are not stored).
// The kernel body (wls_blocked_kernel), its device functions and the launch path live in dss2_wls_large_core.hpp, which
// csrc/dss2_wls_robust.hip shares; this file instantiates the plain estimator, and its banded form (half_bandwidth > 0: the same steps on
// rows that keep a band of G, for graphs beyond the cap above; dss2_wls_banded.hpp), which enters through the same function: wb_route
// there is the route of every entry that serves both forms.
#include "dss2_wls_banded.hpp"

using namespace dss2;

extern "C" int dss2_wls_large_max_nodes(void) { return WL_MAX_NODES; }
extern "C" size_t dss2_wls_large_lds_bytes(int nodes_per_graph) {
  return nodes_per_graph > 0 && nodes_per_graph <= WL_MAX_NODES ? wl_lds_bytes(nodes_per_graph) : 0;
}
extern "C" size_t dss2_wls_large_workspace_bytes(int nodes_per_graph, int64_t groups) { return wl_workspace_bytes(nodes_per_graph, groups); }
extern "C" int64_t dss2_wls_large_groups(const dss2_wls_solve_args* ap) {
  if (!ap || wl_check_size(*ap, "wls_solve_large") != 0 || ap->max_groups < 0) return 0;
  return wl_grid(*ap);
}

static int wls_solve_large_launch(const dss2_wls_large_args* bp, void* stream) {
  using B = dss2_wls_large_args;
  return wb_route<wls_blocked_kernel<B>, wls_banded_kernel<B>>(*bp, "wls_solve_large", "wls_solve_large (banded)", as_stream(stream));
}
extern "C" int dss2_wls_solve_large(const dss2_wls_large_args* bp, void* stream) {
  return dss2::entry(wls_solve_large_launch, stream, dss2::copied(bp, "dss2_wls_solve_large"));
}
