/*
 * dss2_hip.h -- C ABI of libdss2_hip.so: the MI355X (gfx950) kernels for the DSS2 hot path.
 *
 * The reference (TU-Delft-AI-Energy-Lab/Deep-Statistical-Solver-for-Distribution-System-State-
 * Estimation) has no FFI layer: the path is PyTorch-eager Python (networks.py, data.py) on top of
 * torch_geometric.  Each entry point below replaces a chain of ATen/PyG ops at the cited
 * reference lines; the Python mirror of the reference interface (networks.MPN etc.,
 * data.gsp_wls_edge / get_pflow) calls them through ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host; the caller (PyTorch's
 *    caching allocator) owns every buffer, the library allocates nothing and keeps no state
 *    except a thread-local error string;
 *  - fp32 row-major matrices with an explicit leading dimension `ld*` (in floats), so the
 *    reference's column slices (data.x[:, :8], data.edge_attr[:, 6:]) are passed without copies;
 *  - all launches are asynchronous on `stream` (a hipStream_t passed as void*); no host sync;
 *  - return 0 on success, non-zero on error; message via dss2_last_error().
 *
 * Graph structure ("topology", built once per distinct edge_index and cached by the caller):
 *   directed edge list d in [0,E2): E2 = 2E when the reference's undirect_graph() doubles the
 *   graph (networks.py:240-258; d >= E is the reverse of stored edge d-E with edge_attr columns
 *   0 and 2 negated), else E2 = E.
 *   CSR by target:  rowptr[N+1], col[E2] = source node, ent[E2] = stored edge id | flip<<31,
 *                   w[E2] = gcn_norm weight deg^-1/2[src] * deg^-1/2[tgt]  (PyG TAGConv).
 *   CSR by source (transpose): rowptrT, colT (= target node), entT, wT.
 *   Within a row, entries are sorted by d (the order index_add visits them on the CPU).
 *   tile_start[ntiles+1]: consecutive node ranges that contain only whole graphs (no edge
 *   crosses a tile) with at most 32*nrb rows each; one workgroup processes one tile in LDS.
 */
#ifndef DSS2_HIP_H
#define DSS2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* dss2_last_error(void);
int dss2_version(void);

/* ---- topology ------------------------------------------------------------------------- */

/* Content hash + the reference's directedness rule in ONE pass over edge_index[2,E] (int64):
 *   out3[0], out3[1] = two independent 64-bit position-dependent hashes (wrapping integer sums: independent of the
 *                      order of evaluation) -- together the 128-bit key of the caller's structure cache;
 *   out3[2]          = number of edges (v0 -> u0) that reverse the batch's FIRST edge (u0 -> v0):
 *                      MPN.is_directed(edge_index) <=> out3[2] == 0  (networks.py:236-238, first edge only).
 * out3 must be zeroed by the caller; one 24-byte device-to-host copy replaces the reference's per-forward sync. */
int dss2_topology_probe(const int64_t* edge_index, int64_t n_edges, uint64_t* out3, void* stream);

/* ---- launch plans (round 5): one C call per step where a step cannot be captured into a hipGraph ----------------------------- *
 * The reference's training loop runs its step from Python batch after batch (/root/reference/dss2_run.py:134-144).  Here a step is *
 * ~14-60 launches through this C ABI, and the Python around every launch (argument structs, tensor bookkeeping, autograd) costs     *
 * ~20 us of host time: small configurations are host-bound (C1: 0.29 ms eager against 0.10 ms as a hipGraph replay).  A plan is the *
 * library's own record of a step: between dss2_plan_begin and dss2_plan_end EVERY launch entry point of this header (all threads:    *
 * autograd runs the backward on its own) still launches, and also appends itself -- bound to copies of its host-side argument        *
 * structs and tables -- to the plan; dss2_plan_run(plan, stream) then re-issues the same launches, in order, on `stream`, from ONE  *
 * C call.  Same contract as a hipGraph replay: the recorded device pointers must stay valid (record the step on tensors that        *
 * live as long as the plan, e.g. inside a private memory pool), by-value scalars are frozen (use the device-side step counter of    *
 * dss2_optim_step_flat / _dev and use_host_seed = 0 of dss2_rng_next, as under capture).  Only launches of this library are         *
 * recorded.  One plan records at a time (process-wide).  Every entry point that launches a STEP's work records itself (model, loss, *
 * dss2_get_pflow / dss2_eval_batch, dropout masks, optimizer, dss2_collate / dss2_collate_cursor, dss2_accum_scalar, and            *
 * dss2_csr_build_padded: the structure of a padded batch is a function of device data and part of the step); the entry              *
 * points that are not launches of a step -- structure build (dss2_topology_probe, dss2_csr_build, dss2_csr_build_graphs,             *
 * dss2_tiles_*, dss2_ell_tiles_build, dss2_deg_pows), measurement model, z-score, ragged collations -- return 3 while a plan records *
 * instead of being silently left out of it.                                                                                         */
typedef struct dss2_plan dss2_plan;
int dss2_plan_begin(dss2_plan** out);
int dss2_plan_end(dss2_plan* plan);
int dss2_plan_size(const dss2_plan* plan);                /* recorded launches */
int dss2_plan_run(const dss2_plan* plan, void* stream);
void dss2_plan_destroy(dss2_plan* plan);

/* ---- dss2_csr_build: the whole per-topology structure on the device, no host round trip.
 * Replaces MPN.undirect_graph's concatenations (networks.py:240-258), PyG gcn_norm / degree (per TAGConv call) and the
 * index handling of PyG's scatter: counting sort of the directed edge list by target, by source, and of the stored
 * edges by incident bus (integer atomics for counts and slot claims, then a per-row sort by directed edge id, so the
 * result is independent of the order the atomics land in).  doubled != 0: directed list d in [0, 2E), d >= E is the
 * reverse of stored edge d - E (flip flag in ent); 0: the list is used as given.
 * Outputs (device, caller-allocated): the arrays of the header comment (E2 = doubled ? 2E : E), perm / permT
 * (directed edge id of every CSR entry), efrom / eto, deg[N] (in-degree as float), and
 *   lastcut[N+1]: largest q' <= q such that no edge spans the boundary before row q' (a legal tile cut);
 *   meta[16] (int32): 0 max in-degree, 1 max out-degree, 2 longest / 4 shortest whole-graph segment, 3 number of
 *   segments, 5 error flag (1: endpoint outside [0, N); 2: ELL width smaller than a row), 6 / 7 max CSR entries per
 *   tile (by target / by source, written by dss2_ell_tiles_build), 8.. ntiles per candidate (dss2_tiles_walk).
 * work: dss2_csr_build_work_ints(N, E, doubled) int32 of device scratch. */
typedef struct dss2_csr_build_args {
  const int64_t* edge_index; int64_t n_edges; int64_t n_nodes; int32_t doubled;
  int32_t no_flip;   /* doubled only: 1 = reverse edges carry NO sign-flip flag in ent / entT (the Multi* / MaskEmbd* variants of
                      * the reference duplicate edge_attr unchanged, networks.py:440-444; MPN negates columns 0 and 2) */
  int32_t* rowptr; int32_t* col; int32_t* ent; int32_t* perm; float* w;
  int32_t* rowptrT; int32_t* colT; int32_t* entT; int32_t* permT; float* wT;
  int32_t* inc_rowptr; int32_t* inc_ent; int32_t* efrom; int32_t* eto;
  float* deg; int32_t* lastcut; int32_t* meta; int32_t* work;
} dss2_csr_build_args;
int dss2_csr_build(const dss2_csr_build_args* args_host, void* stream);
int64_t dss2_csr_build_work_ints(int64_t n_nodes, int64_t n_edges, int doubled);
/* The same arrays (args.work unused) in ONE launch for a batch of equal-size graphs whose ranges in the stored edge list are known (round 6):
 * graph g = rows [g * nodes_per_graph, ..) and stored edges [edge_ptr[g], edge_ptr[g + 1]) (DEVICE int64 [G + 1]; NULL: edges_per_graph
 * each).  Every global offset is then a graph-local prefix sum plus (1 or 2) * edge_ptr[g], so one wave per graph builds counts, row
 * pointers, slot claims, per-row order, gcn_norm weights, incidence lists, legal cuts and statistics in LDS -- and, if deg_pows != NULL,
 * the [N][4] folded-bias row scales of dss2_deg_pows -- with the definitions, and therefore the bits, of dss2_csr_build (an edge that leaves
 * its graph's rows sets meta[5] = 1).  What the device loader uses for every batch it assembles: a batch with a NEW structure per step
 * (BASELINE config C5) goes from ~26 launches to 5.  dss2_csr_build_graphs_supported: nodes_per_graph <= 192, max_edges_per_graph <= 1024
 * and the per-wave scratch within LDS. */
int dss2_csr_build_graphs(const dss2_csr_build_args* args_host, int32_t nodes_per_graph, const int64_t* edge_ptr, int32_t edges_per_graph,
                          int32_t max_edges_per_graph, float* deg_pows, void* stream);
int dss2_csr_build_graphs_supported(int32_t nodes_per_graph, int32_t max_edges_per_graph);

/* tile_start[ntiles+1] for batches of equal-size graphs (closed form): tile t starts at min(t * rows_per_tile, N). */
int dss2_tiles_uniform(int32_t* tile_start, int32_t ntiles, int32_t rows_per_tile, int64_t n_nodes, void* stream);
/* general batches: greedy packing of whole segments for n_cand (<= 8) candidate row budgets tm_host[c] at once, from
 * lastcut; tile_starts_host[c]: device array of cap + 1 ints; ntiles_dev[c] <- number of tiles, or -1 when a segment
 * exceeds the budget.  Sequential per candidate (each start depends on the previous one). */
int dss2_tiles_walk(const int32_t* lastcut, int64_t n_nodes, const int32_t* tm_host, int32_t n_cand,
                    int32_t* const* tile_starts_host, int32_t cap, int32_t* ntiles_dev, void* stream);

/* per-tile ELL slices of both CSRs, [ntiles][width][tm] int2 each (width 0: skipped, pointers may be NULL):
 *   ell_tiles / ellT_tiles          {local other node, weight bits}, empty slot {own row, 0}     (tile kernels)
 *   ell_ent_tiles / ellT_ent_tiles  {local other node, stored edge id | flip}, empty slot {0, -1} (edge-MLP kernels)
 * also meta[6], meta[7] <- max CSR entries of one tile (atomic max). */
typedef struct dss2_ell_build_args {
  const int32_t* rowptr; const int32_t* col; const int32_t* ent; const float* w;
  const int32_t* rowptrT; const int32_t* colT; const int32_t* entT; const float* wT;
  const int32_t* tile_start; int32_t ntiles; int32_t tm; int32_t ell_width; int32_t ellT_width;
  void* ell_tiles; void* ell_ent_tiles; void* ellT_tiles; void* ellT_ent_tiles; int32_t* meta;
  int32_t uniform_rows;   /* round 6.  > 0 (with n_nodes): tiles of equal-size graphs, tile t = rows [t * uniform_rows, (t + 1) * uniform_rows) cut at
                           * n_nodes -- tile_start is then an OUTPUT of this launch (dss2_tiles_uniform folded in); 0: tile_start is read */
  int64_t n_nodes;
} dss2_ell_build_args;
int dss2_ell_tiles_build(const dss2_ell_build_args* args_host, void* stream);

/* The structure of a PADDED batch of equal-size graphs, as launches of a training step (host-free epochs on data whose topology changes
 * per sample, BASELINE config C5).  Graph g owns the stored edge slots [g * edge_stride, (g + 1) * edge_stride) of edge_index[2][E],
 * E = G * edge_stride; only the first edge_count[g] of them are branches, the rest are padding edges that the structure never lists:
 * every shape is a function of (G, edge_stride) alone, the structure a function of DEVICE data (edge_index, edge_count) -- so this entry
 * point, unlike the builds above, records itself into launch plans and is captured into hipGraphs.  Launches: one workgroup forms
 * csr_ptr[G + 1] (exclusive sums of the counts), edge_total[0] (their sum: the batch's real edge count, what the loss divides by) and
 * resets meta; the quarter-wave-per-graph build of dss2_csr_build_graphs writes the arrays of csr (entries of graph g at (1 or 2) *
 * csr_ptr[g]; directed ids stay d = stored slot, reverse d + E; efrom / eto are written for every slot, padding included; array tails
 * beyond rowptr[N] are left alone) and deg_pows[N][4]; then one ELL launch per tiling in ell[0 .. n_ell) (closed-form tilings:
 * uniform_rows > 0).  edge_count[g] outside [0, edge_stride] sets meta[5] = 3 and the graph gets no edges (nothing is read out of
 * bounds).  csr.work is unused. */
#define DSS2_PADDED_MAX_TILINGS 4
typedef struct dss2_padded_build_args {
  dss2_csr_build_args csr;
  int32_t nodes_per_graph; int32_t edge_stride;
  const int32_t* edge_count;     /* DEVICE [G] */
  int64_t* csr_ptr;              /* DEVICE [G + 1], written */
  int32_t* edge_total;           /* DEVICE [1], written */
  float* deg_pows;               /* DEVICE [N][4], written */
  int32_t n_ell; int32_t pad_;
  dss2_ell_build_args ell[DSS2_PADDED_MAX_TILINGS];
} dss2_padded_build_args;
int dss2_csr_build_padded(const dss2_padded_build_args* args_host, void* stream);

/* out[N,4] <- columns [deg, A deg, A^2 deg, A^3 deg] (A = the gcn_norm propagation matrix of the CSR), accumulated in
 * float64 in CSR order: the row scales of a bias folded through m propagations.  work: 2 N device doubles. */
int dss2_deg_pows(const int32_t* rowptr, const int32_t* col, const float* w, const float* deg, int64_t n_nodes,
                  float* out, double* work, void* stream);

/* ---- K6: standalone CSR segmented sum (the scatter-add of MessagePassing aggr='add',
 *      networks.py:164,206, measured on its own).  out[i,:] = sum_{e in row i} msg[ent[e],:]
 *      `ent` holds row indices into msg (directed edge ids).  h in {32, 64, 128, 256} with 16-byte aligned operands
 *      takes the HBM-rate kernel (16-byte lanes); any other width / alignment a one-thread-per-element kernel.
 *      Summation order inside a row = CSR order (ascending directed edge id): deterministic, no atomics. */
int dss2_segment_sum(const float* msg, int64_t ldm, const int32_t* rowptr, const int32_t* ent,
                     float* out, int64_t ldo, int64_t n_rows, int h, void* stream);

/* out[r,:] = src[idx[r],:], r < n_rows: the gather half of PyG MessagePassing.propagate (x_j = x[edge_index[0]],
 * x_i = x[edge_index[1]]; call site networks.py:206) and the backward of the segmented sum. */
int dss2_gather_rows(const float* src, int64_t lds, const int32_t* idx, float* out, int64_t ldo, int64_t n_rows, int h,
                     void* stream);

/* ---- weight packing: nn.Linear weights -> MFMA B-operand fragment order ----------------- */

typedef struct dss2_pack_desc {
  const float* src;   /* W, row-major [rows, cols] with leading dimension ld            */
  float* dst;         /* packed matrix base: [ncg][kpad/8][64 lanes][4]                 */
  int32_t rows, cols, ld;
  int32_t transpose;  /* bit 0: 1: B[k][j] = W[j][k] (forward, K=cols); 0: B[k][j] = W[k][j].
                       * bit 1: write the bf16x3 layout [ncg][kpad/16][3 planes][64 lanes][8 bf16] (kpad a multiple of 16):
                       * every weight split into three bf16 pieces h + m + l for the fp32-accurate bf16 MFMA path
                       * bit 2: ignored by the kernels (the host side marks descriptors whose src the fold of the same step writes)
                       * bit 3: the f16x2 layout of the f16x3 chains (round 5): dst = the GROUP's buffer [matrix][ncg][kpad/16][2 planes]
                       * [64 lanes][8 fp16] + one int32 per matrix and packed column ([matrix][ncg * 32]: the exponent s of the power-
                       * of-two scale applied to that column before the split, 2^s max_k |B[k][j]| in [2^14, 2^15)); koff = matrices in
                       * the group, joff = this matrix's index (not offsets); the matrix is written whole, padding included          */
  int32_t koff;       /* k offset of this block inside the packed matrix (any value)   */
  int32_t kpad;       /* padded K of the packed matrix (multiple of 8)                  */
  int32_t ncg;        /* number of 32-column groups of the packed matrix                */
  int32_t joff;       /* column offset of this block inside the packed matrix           */
} dss2_pack_desc;

/* descs: device array of n_desc descriptors.  Several descriptors may fill disjoint k / column
 * ranges of one packed matrix (stacked or side-by-side blocks).  The kernel writes exactly the
 * elements B[koff + k][joff + j], k < K, j < J; the caller zero-fills dst once so that padding
 * (k >= total K, columns >= total J) stays zero. */
int dss2_pack_weights(const dss2_pack_desc* descs, int n_desc, int max_elems, void* stream);

/* ---- K1: EdgeAggregation (networks.py:159-209) ------------------------------------------ */

/* S[i,:] = sum_{e: tgt(e)=i} relu(W1 . [x_i | x_src(e) | ea'(e)] + b1)      (first Linear + ReLU
 * of networks.py:170-174,181, aggregated before the second Linear, which is linear:
 * out = S . W2^T + deg * b2 is finished by dss2_gemm_prop with nmat = 1), and its backward, which RECOMPUTES the ReLU
 * gates: the two passes must run the same arithmetic.  One argument struct serves both:
 *   graph, one of two forms.  ell_ent != NULL: tiles of 32 * nrb rows holding whole graphs (tile_start [ntiles + 1]) and their
 *     ELL entry table, int2 {local other node, stored edge id | flip << 31 (-1 = empty slot)} [ntiles][ell_width][32 * nrb],
 *     built once per topology from the CSR by target (forward, backward with by_source = 0) or by source (by_source = 1);
 *     1 <= ell_width <= 32.  ell_ent == NULL: the CSR (rowptr, col, ent over n_nodes rows; by_source = 1: the transposed one),
 *     one row per wavefront -- any degree.
 *   dss2_edge_fwd writes S [N, h].  bwd_with_u != 0 announces that the backward will be asked for U (the gradient w.r.t. x):
 *     the forward then takes the arithmetic that backward recomputes its gates with (dss2_edge_plan).
 *   dss2_edge_bwd reads dS [N, h], the gradient w.r.t. S.
 *     by_source = 0: per-workgroup partials of dW1 [h, 2 fn + fe] and db1 [h] into slab[n_slabs][h * (2 fn + fe) + h] (finish
 *       with dss2_reduce_slabs*; on tiles min(n_slabs, ntiles) persistent workgroups write one slab each) and, if U != NULL,
 *       U[i,:] = sum_{e -> i} dz_e (ldu floats per row).
 *     by_source = 1: U[i,:] = sum_{e: src(e) = i} dz_e; slab is not touched.
 * fn must be 8 and fe must be 6 (the only dims the reference's data produces).  h <= 256. */
typedef struct dss2_edge_args {
  const float* x; int64_t ldx; const float* ea; int64_t ldea; const float* W1; const float* b1; const float* dS;
  const int32_t* tile_start; const void* ell_ent; int32_t ell_width, nrb, ntiles, pad_;
  const int32_t* rowptr; const int32_t* col; const int32_t* ent; int64_t n_nodes;
  float* S; float* slab; float* U; int64_t ldu; int32_t n_slabs;
  int32_t h, fn, fe, bwd_with_u, by_source;
} dss2_edge_args;
int dss2_edge_fwd(const dss2_edge_args* args_host, void* stream);
int dss2_edge_bwd(const dss2_edge_args* args_host, void* stream);

/* Which kernel each of the three passes of an edge MLP runs, and its launch geometry: the record dss2_edge_fwd / dss2_edge_bwd
 * dispatch from (edge_select in csrc/dss2_edge.hip) and the layer chain's edge phases are derived from.  Families fall through
 * bf16x6 -> fp32 MFMA -> VALU tile; no entry table: the CSR kernels (DESIGN.md 4.3 holds the table). */
enum dss2_edge_family {
  DSS2_EDGE_NONE = 0,     /* the pass is refused (h, an ELL width above 32) or not run (by source without U)                    */
  DSS2_EDGE_CSR,          /* one CSR row per wavefront (edge_hidden_*_kernel)                                                   */
  DSS2_EDGE_VALU,         /* VALU tile kernel, a row per wavefront (edge_tile_kernel)                                           */
  DSS2_EDGE_VALU_HALF,    /* ... two rows per wavefront (h <= 32; DSS2_EDGE_TILE_HALF=0: off)                                   */
  DSS2_EDGE_FP32_MFMA,    /* first Linear as fp32 MFMAs (edge_mfma_*_kernel)                                                    */
  DSS2_EDGE_BF16X6        /* first Linear as bf16x6 (dss2_edge16.hip)                                                           */
};
typedef struct dss2_edge_pass_t {
  int32_t family;         /* dss2_edge_family                                                                                   */
  int32_t nrb;            /* 32-row blocks the kernel is instantiated (matrix pipe) or staged (VALU) for; CSR: 0                */
  int32_t parts;          /* 2: 128- / 192-row tiles walked as two parts of 64 / 96 rows; else 1                                */
  int32_t block;          /* threads per workgroup                                                                              */
  int32_t wg_per_tile;    /* forward: workgroups per tile (2 with parts); backward passes: 0 = min(n_slabs, ntiles) persistent
                           * workgroups (CSR: n_slabs); CSR forward: 0 = a wavefront per row                                    */
  int32_t lds_bytes;      /* dynamic LDS of the launch                                                                          */
} dss2_edge_pass_t;
typedef struct dss2_edge_plan_t {
  dss2_edge_pass_t fwd, bwd, bwd_src;   /* forward, backward by target, backward by source                                     */
  int32_t pair_exact;     /* 1: forward and backward by target form the pre-activation with the same values in the same order
                           * (same family), so the recomputed gates are the forward's bit for bit                               */
  int32_t pad_;
} dss2_edge_plan_t;
/* ell_width / ellT_width: the ELL widths of the entry tables by target / by source, 0 = no table (the passes that would read it
 * run on the CSR).  with_u: the backward forms U (dss2_edge_args.bwd_with_u, U != NULL); without it there is no pass by source.
 * Answers from the arguments and the environment alone: no GPU needed. */
int dss2_edge_plan(int h, int nrb, int ell_width, int ellT_width, int with_u, dss2_edge_plan_t* out);

/* EdgeAggregation with node features of any width (networks.py:159-209 as MultiMPN / MaskEmbdMultiMPN instantiate it on the
 * hidden activation, networks.py:486-498).  AB[N, 2h] = X [W1[:, :d] ; W1[:, d:2d]]^T (one dss2_gemm_prop); W1c = &W1[0][2d]
 * with row stride ldw = 2d + fe; fe <= 8; any h (hidden units are independent: more than 256 run as several launches).
 *   fwd: S[i,:] = sum_{e: tgt(e)=i} relu(AB[i, :h] + AB[src(e), h:] + W1c ea'(e) + b1)
 *   bwd: dz_e = dS[tgt(e)] (z_e > 0).  by_source = 0 (CSR by target): dAB[i, :h] = sum dz, slab[n_slabs][h*fe + h] =
 *        partial dW1c, db1 (finish with dss2_reduce_slabs); by_source = 1 (CSR by source): dAB[j, h:] = sum dz.
 * Reverse edges flagged in `ent` negate edge_attr columns 0 and 2 (the reference's MPN doubling); the Multi* variants double
 * without sign flips, i.e. their structure carries no flags. */
int dss2_edge_combine_fwd(const float* AB, int64_t ldab, const float* ea, int64_t ldea, const float* W1c, int64_t ldw,
                          const float* b1, const int32_t* rowptr, const int32_t* col, const int32_t* ent, float* S,
                          int64_t n_nodes, int h, int fe, void* stream);
int dss2_edge_combine_bwd(const float* AB, int64_t ldab, const float* ea, int64_t ldea, const float* W1c, int64_t ldw,
                          const float* b1, const float* dS, const int32_t* rowptr, const int32_t* col, const int32_t* ent,
                          float* dAB, float* slab, int n_slabs, int64_t n_nodes, int h, int fe, int by_source, void* stream);

/* ---- K2/K4: fused tile GEMM + Horner graph propagation --------------------------------- *
 * Y = epilogue( sum_{m=0..nmat-1} P^m (X . B_m) ),  P = A_hat given by (rowptr, col, w).
 *  forward TAGConv (PyG TAGConv; call sites networks.py:267,271):
 *        X = h, B_m = lins[m].weight^T, P = A_hat (CSR by target), bias, optional dropout mask
 *        and ReLU;  mathematically sum_m lins[m](A_hat^m h) + b, evaluated as
 *        G0 + A_hat (G1 + A_hat G2) with G_m = h W_m^T (propagation at OUTPUT width).
 *  data-gradient of TAGConv: X = dOut, B_m = lins[m].weight, P = A_hat^T (CSR by source).
 *  plain Linear (second Linear of the edge MLP): nmat = 1, bias scaled per row by rowscale.
 * Epilogue order: + bias[col]*(rowscale?rowscale[row]:1); * dmask; relu; * (relu_src > 0);
 * + add_src.  One workgroup per tile; requires nrb in {1,2,4,8} and nmat in 1..4.          */
typedef struct dss2_gemm_prop_args {
  const float* X; int64_t ldx; int32_t kreal; int32_t kpad;
  const float* Bp;                 /* packed [nmat][ncg][kpad/8][64][4]                   */
  const float* bias; const float* rowscale;
  const float* relu_src; int64_t ld_relu;
  const float* dmask; int64_t ld_dmask;
  const float* add_src; int64_t ld_add;
  float* Y; int64_t ldy; int32_t hout; int32_t ncg;
  int32_t relu; int32_t nmat; int32_t nrb; int32_t ntiles;
  const int32_t* tile_start;
  const int32_t* rowptr; const int32_t* col; const float* w;
  int32_t max_nnz;                 /* max CSR entries of one tile (CSR staging)            */
  int32_t ell_width;               /* > 0: max row degree of the batch; the tile's graph    *
                                    * slice is staged as ELL [ell_width][rows] (fixed trip  *
                                    * count); 0: stage the CSR slice (any degree)           */
  int32_t prop_in;                 /* > 0: INPUT-side propagation (narrow inputs): X has    *
                                    * kreal/(prop_in+1) real columns; the kernel appends    *
                                    * P X, P^2 X, ... in LDS and runs ONE GEMM against the  *
                                    * k-stacked matrix [B_0; B_1; ...] (nmat must be 1)     */
  int32_t narrow_h;                /* > 0: OUTPUT-side propagation for narrow outputs: the  *
                                    * nmat matrices (narrow_h columns each, nmat*narrow_h   *
                                    * <= 32) sit side by side in ONE 32-column group; the   *
                                    * Horner recurrence runs across column blocks in LDS    */
  const float* prebias;            /* optional [nmat][hout] with pre_rowscale [N][4]: adds the  *
                                    * rank-nmat term sum_m pre_rowscale[row][m] * prebias[m][col] *
                                    * before the activation.  With pre_rowscale rows             *
                                    * [s, P s, P^2 s, P^3 s] this is sum_m P^m (s (x) prebias_m): *
                                    * a row-scaled bias inside every X B_m, i.e. the edge MLP's   *
                                    * second Linear folded in (s = deg, prebias_m = W_m b2)       */
  const float* pre_rowscale;
  const void* ell_tiles;           /* optional: per-tile ELL slices precomputed once per     *
                                    * topology, int2 {local src, weight bits}[ntiles]        *
                                    * [ell_width][32*nrb] (rows >= tile rows: {row, 0});      *
                                    * NULL: the kernel derives the slice from the CSR         */
  /* in-kernel dropout (nn.Dropout of networks.py:268, regenerated instead of stored): drop_state = device {seed,   *
   * offset} of this forward call (dss2_rng_next) or NULL; the epilogue multiplies element (row, col) by 0 or       *
   * drop_scale = 1/(1-p) according to Philox4x32-10(seed, offset, drop_id, row, col/4) >= drop_thr = p * 2^32,     *
   * where drop_id > 0 names the layer whose mask this is (0: no dropout; in a chain: per layer).  Applied where     *
   * `dmask` (an explicit [N, hout] multiplier tensor, still supported) is applied.                                 */
  const uint64_t* drop_state; uint32_t drop_thr; float drop_scale; int32_t drop_id;
  int32_t b_format;   /* layout of the packed weights: 0 = fp32 fragments; 1 = bf16x3 fragments (dss2_gemm_prop_chain, and
                         dss2_gemm_prop where dss2_gemm_prop_plan answers DSS2_GEMM_BF16X6_KHALF; kpad is then a multiple of 16) */
  int32_t max_tile_rows;   /* 0: unknown (any tile may hold up to 32 * nrb rows); > 0: an upper bound of EVERY tile's row count --
                              the tall-tile chains then leave out the row pieces that are padding in every tile (70-bus graphs in
                              96-row tiles: rows 72..95, a quarter of the hops and of the epilogue) */
} dss2_gemm_prop_args;

int dss2_gemm_prop(const dss2_gemm_prop_args* args_host, void* stream);
/* Which kernel a launch of these arguments runs and its geometry: the record the library's own dispatch launches from (gemm_select in
 * csrc/dss2_gemm_prop.hip).  Narrow layers (args.narrow_h > 0) stream X where nmat * narrow_h <= 8, kpad % 16 == 0, X rows can be read 16
 * bytes at a time (kreal % 4 == 0, ldx % 4 == 0, X 16-byte aligned) and, for nmat > 1, ELL slices exist; else they take the tile
 * kernel.  General layers stage the X tile in two K halves where matrix-sequential tall tiles (nmat > 1, nrb * nmat >= 16) would
 * otherwise leave a column group without its wave; bf16x3 weights (b_format 1) run in that form only.                                   */
typedef enum dss2_gemm_kernel {
  DSS2_GEMM_NONE = 0,          /* the launch is refused: see dss2_gemm_prop_plan_t.reason                     */
  DSS2_GEMM_NARROW_STREAM,     /* narrow, nothing of X staged (gemm_narrow_stream_kernel)                     */
  DSS2_GEMM_NARROW,            /* narrow, X tile in LDS (gemm_narrow_kernel)                                  */
  DSS2_GEMM_FP32,              /* gemm_prop_kernel<nrb, nmat>, fp32 MFMAs                                     */
  DSS2_GEMM_FP32_KHALF,        /* ... with K-halved staging: every column group its wave                      */
  DSS2_GEMM_BF16X6_KHALF       /* gemm_prop_kernel<nrb, nmat, true, row_split>: bf16x6, K-halved              */
} dss2_gemm_kernel;
typedef struct dss2_gemm_prop_plan_t {
  int32_t kernel;              /* dss2_gemm_kernel                                                            */
  int32_t reason;              /* kernel == NONE: the code dss2_gemm_prop returns (2: no such kernel for these arguments, 3: the tile
                                * does not fit LDS)                                                           */
  int32_t row_split;           /* waves per column group (1; bf16x6: 2 unless DSS2_GEMM_RS=1)                 */
  int32_t waves;               /* column-group waves (narrow kernels: 4)                                      */
  int32_t block;               /* threads per workgroup = 64 * waves * row_split                              */
  int32_t pad_;
  uint64_t lds_bytes;          /* dynamic LDS of the launch; a K-halved kernel's is the K-halved figure       */
  uint64_t sizing_lds;         /* what dss2_gemm_prop_lds_bytes answers: the general kernel's LDS WITHOUT K-halving, from the shape
                                * alone.  Callers size tiles and merged GEMMs by it, and the dispatch's own "tile needs ... B of LDS"
                                * refusal (reason 3) tests it too -- not lds_bytes: a shape that would fit K-halved only is refused,
                                * as it always was.  (Narrow launches are refused by the narrow tile kernel's own LDS.)            */
} dss2_gemm_prop_plan_t;
/* fills *out from the arguments and the environment alone (no GPU, nothing dereferenced; ntiles is not read).  Arguments that are
 * errors whatever the kernel (bad kpad / ncg, a missing CSR, prebias or dropout on a narrow launch, ...) are dss2_gemm_prop's to
 * refuse and are not looked at here.  Returns 0, or 2 for a null pointer.                                                     */
int dss2_gemm_prop_plan(const dss2_gemm_prop_args* args_host, dss2_gemm_prop_plan_t* out);
/* Policy constant: 96- / 192-row tiles with ONE column group (hout <= 32) take the split-plane chain -- single-wave workgroups -- only
 * from this many tiles on (a launch with fewer runs the multi-wave chain of that shape, which 192-row tiles do not have); -1: never
 * (DSS2_CHAIN_SP6_NCG1=0).  Applied in one place, dss2_gemm_prop_chain_plan; the *_supported queries below answer for the
 * capability, without a tile count. */
int dss2_chain_sp6_single_group_min_tiles(void);

/* ---- layer chain: n_layers (<= 8) H -> H layers of dss2_gemm_prop in ONE launch, the activation
 *      tile staying in LDS from layer to layer (tiles hold whole graphs, so a tile's next layer depends on that tile
 *      only).  args describes the first layer's input X and everything the layers share (shapes, leading
 *      dimensions ldy / ld_relu / ld_dmask / ld_add, topology, pre_rowscale); per layer: packed weights, bias,
 *      epilogue operands and the output Y (every layer's output is still written once: the backward pass and the
 *      weight gradients read it).  Forward chain of TAGConv layers (/root/reference/networks.py:266-269 iterated)
 *      or, with the transposed graph and packs, the chain of their data-gradients.
 *      Supported: dss2_gemm_prop_chain_supported(...) != 0 (ELL slices, kreal == hout <= 256, hout % 4 == 0,
 *      16-byte aligned operands); otherwise call dss2_gemm_prop per layer.                                          */
typedef struct dss2_chain_layer {
  const float* Bp; const float* bias; const float* relu_src; const float* dmask; const float* add_src;
  const float* prebias; float* Y; int32_t relu; int32_t drop_id;   /* drop_id: as in dss2_gemm_prop_args, per layer */
  /* Optional, only where dss2_gemm_prop_chain_gate_words(...) > 0 (else leave NULL: the kernels of other shapes ignore both).
   * y_bits: the chain also writes one bit per stored element, Y > 0, as ntiles x gate_words 64-bit words in the kernel's own
   * order (per lane of the wave that owns the element: opaque to the caller).  gate_bits: such a buffer, written by a chain launch over the SAME tiles, hout and nmat, replaces the reads of
   * relu_src (which must still be given: it defines the gate) -- 1/32 of the bytes and no latency-exposed vector loads. */
  const uint64_t* gate_bits; uint64_t* y_bits;
} dss2_chain_layer;
/* 64-bit words per tile of y_bits / gate_bits for this shape; 0: the chain kernel of this shape has no bit form */
int dss2_gemm_prop_chain_gate_words(int nrb, int nmat, int kreal, int hout, int ell_width);
int dss2_gemm_prop_chain(const dss2_gemm_prop_args* args_host, const dss2_chain_layer* layers_host, int n_layers, void* stream);
/* The chain with the narrow head TAGConv fused in (replaces a dss2_gemm_prop launch next to the chain that re-reads [N, hid];
 * /root/reference/networks.py:266-275 -- the last TAGConv(dim_hid, dim_out) of MPN / SkipMPN and its data gradient).
 * mode 1 (forward chain): after the last chained layer, Y[N][nout] = bias + sum_m P^m (h W_m^T) (+ add_src), h = that layer's
 *   output (still written to its own Y for the backward).  mode 2 (transposed chain = data gradients): the chain's input tile is
 *   X = (gate > 0) * dropout(drop_id) * sum_m (P^T)^m G W_m with G[N][nout] the gradient w.r.t. the head's output, gate the
 *   head's input activation; X is also written to Xout (the weight-gradient kernels read it); args.X is ignored.
 * W[m]: the head's weights [nout][hid] row-major, m < nmat.  nout <= 4.  Same tiles / ELL slices as the chain. */
/* The edge MLP's first Linear (the bf16x6 tile kernels of dss2_edge_fwd / dss2_edge_bwd, by target, without U) as a phase
 * of the chain with the fused head, tile by tile (where dss2_gemm_prop_chain_edge_supported says so):
 *   mode 1: the chain's input tile is S = sum over the incoming edges of relu(W1 [x_i | x_j | edge_attr] + b1), computed in the
 *     launch's staging instead of read from args.X; S [N][hid] is still written (row-major, ld = hid).
 *   mode 2: the last layer's output (conv 0's input gradient dS) is NOT written to its Y; the edge MLP's backward runs on it in the
 *     same launch and writes ONE slab per tile to `slab`: [ntiles][hid * 22 + hid] floats = [dW1 ([hid][22]) | db1], to be summed
 *     over the tiles (dss2_reduce_slabs*).
 * x [N][8] (ldx), edge_attr [E][6] (ldea), W1 [hid][22], b1 [hid], ell_ent: the forward topology's per-tile ELL table of the edge
 * kernels ({other node, eid | flip << 31}, ell_width = width). */
typedef struct dss2_chain_edge {
  const float* x; const float* ea; const float* W1; const float* b1;
  const void* ell_ent;
  float* S;       /* mode 1 */
  float* slab;    /* mode 2 */
  int64_t ldx, ldea;
  int32_t width, pad;
} dss2_chain_edge;

typedef struct dss2_chain_head {
  const float* W[4];
  const float* bias; const float* add_src; float* Y;      /* mode 1 */
  const float* G; const float* gate; float* Xout;         /* mode 2 */
  int64_t ld_add, ldy, ldg, ld_gate, ldxo;
  int32_t nout, mode, drop_id, pad;
  float* wg_slab;   /* mode 2, optional (round 5): the head's WEIGHT gradient from the same staging -- one slab per tile,
                     * [ntiles][nmat * nout * hid + nout] floats = [dW_0 .. dW_{nmat-1} ([nout][hid] each) | db], to be summed over the tiles
                     * (dss2_reduce_slabs*); `pad` > 0: the stride between the tiles' slabs in floats (a multiple of 4 lets the reduction use
                     * 16-byte lanes).  Needs gate (the head's input rows) and nout <= 2 on 64-, 96- or 192-row tiles
                     * (dss2_gemm_prop_chain_head_wgrad_supported); NULL: not computed */
  dss2_chain_edge edge;   /* optional (W1 == NULL: off): the edge MLP's first Linear inside this launch, see dss2_chain_edge */
} dss2_chain_head;
int dss2_gemm_prop_chain_head(const dss2_gemm_prop_args* args_host, const dss2_chain_layer* layers_host, int n_layers,
                              const dss2_chain_head* head_host, void* stream);
/* mask of the head modes dss2_gemm_prop_chain_head runs for this shape: bit 0 = mode 1 (forward), bit 1 = mode 2 (backward).
 * 3 on the split-plane chain of 64-row tiles (hid >= 96, bf16x6 weights), 2 on its 96- / 192-row form, 0 otherwise. */
int dss2_gemm_prop_chain_head_supported(int nrb, int nmat, int kreal, int hout, int ell_width, int nout);
/* != 0: a mode-2 launch of this shape also forms the head's weight gradient (dss2_chain_head.wg_slab) */
int dss2_gemm_prop_chain_head_wgrad_supported(int nrb, int nmat, int kreal, int hout, int ell_width, int nout);
/* mask of the edge phases (dss2_chain_edge) a launch of this shape runs: bit 0 = mode 1 (forward; ell_width = the forward ELL's),
 * bit 1 = mode 2 (backward; ell_width = the transposed ELL's); edge_width = the edge kernels' ELL width.  64-row tiles, nmat = 3,
 * hid = 128 (four column groups), f16x3 weights (b_format 2), and edge kernels that would run their bf16x6 form; 0 otherwise. */
int dss2_gemm_prop_chain_edge_supported(int nrb, int nmat, int kreal, int hout, int ell_width, int edge_width);
int dss2_gemm_prop_chain_supported(int nrb, int nmat, int kreal, int hout, int ell_width);
/* != 0: the chain can also run with args.b_format = 1 -- weights packed as bf16x3 fragments, the tile GEMM as six
 * v_mfma_f32_32x32x16_bf16 per fp32 product term set (h/m/l splits of both operands, fp32 accumulation): fp32-accurate
 * results at 12 instead of 32 MFMA cycles per unit of k.  Two-row-block tiles, H <= 128. */
int dss2_gemm_prop_chain16_supported(int nrb, int nmat, int kreal, int hout, int ell_width);
/* ... and with args.b_format = 2 as f16x3 (round 5): every layer's Bp = a group buffer in the f16x2 layout (dss2_pack_desc, transpose
 * bit 3: two fp16 planes per matrix + scale exponents), three fp16 MFMAs per product, the activation tile scaled per tile and layer by
 * an exact power of two (csrc/dss2_gemm_chain_sp.hip, MS = 2).  64-row tiles, hout = kreal a multiple of 32; layers gated by fp32
 * activations (relu_src without gate_bits) are refused -- callers keep bf16x3 weights for those.  Also through
 * dss2_gemm_prop_chain_head.  Errors of the size of fp32 arithmetic's own rounding. */
int dss2_gemm_prop_chain_f16_supported(int nrb, int nmat, int kreal, int hout, int ell_width);

/* The ONE decision behind the seven queries above and behind the dispatch of dss2_gemm_prop_chain(_head) (chain_select in
 * csrc/dss2_gemm_chain.hip): for a chain of hid -> hid layers on tiles of 32 * nrb rows, per weight format (args.b_format 0, 1, 2),
 * the kernel a launch runs, its geometry, and what that kernel can carry. */
enum dss2_chain_family {
  DSS2_CHAIN_NONE = 0,   /* the launch is refused                                                                              */
  DSS2_CHAIN_FP32,       /* fp32 MFMAs, multi-wave (dss2_gemm_chain.hip)                                                       */
  DSS2_CHAIN_BF16X6,     /* bf16x6, multi-wave (dss2_gemm_chain16.hip)                                                         */
  DSS2_CHAIN_SP,         /* split planes, 64-row tiles (dss2_gemm_chain_sp.hip): bf16x6 (format 1) or f16x3 (format 2)         */
  DSS2_CHAIN_SP6         /* split planes, 96- / 192-row tiles (dss2_gemm_chain_sp6.hip)                                        */
};
typedef struct dss2_chain_kernel_t {
  int32_t family;        /* dss2_chain_family                                                                                  */
  int32_t row_split;     /* waves that share a column group (1, 2, or 3 on 96-row tiles)                                       */
  int32_t waves;         /* the wave count the kernel is instantiated for (split planes of tall tiles: the column groups)      */
  int32_t block, lds_bytes;   /* threads per workgroup, dynamic LDS of the launch                                              */
  int32_t gate_words;    /* 64-bit words per tile of y_bits / gate_bits of the format's split-plane form; 0: it has none.
                          * (> 0 beside family NONE: an ELL width above 32, which the chain refuses for these tiles)           */
  int32_t head_modes;    /* mask of the dss2_chain_head modes (bit 0: mode 1, bit 1: mode 2) for the nout asked; 0: no head    */
  int32_t head_wgrad;    /* != 0: a mode-2 launch also forms the head's weight gradient (dss2_chain_head.wg_slab)              */
  int32_t edge_modes;    /* mask of the dss2_chain_edge phases for the edge_width asked (format 2 only)                        */
} dss2_chain_kernel_t;
typedef struct dss2_chain_plan_t { dss2_chain_kernel_t fmt[3]; } dss2_chain_plan_t;
/* ntiles: the launch's tile count, 0 = "for the capability" (what the queries above ask).  nout / edge_width: 0 = no head / no edge
 * phase asked.  ell_width is the chain's own (the transposed one for a data-gradient chain). */
int dss2_gemm_prop_chain_plan(int nrb, int nmat, int hid, int ell_width, int ntiles, int nout, int edge_width, dss2_chain_plan_t* out);

/* != 0: dss2_gemm_prop (one layer) accepts args.b_format = 1 for this shape -- the tall tiles (128 / 192 rows) that run
 * matrix-sequentially with the X tile staged in two K halves; same bf16x6 arithmetic as the chain.  A reader of dss2_gemm_prop_plan
 * (operands taken as aligned), like dss2_gemm_prop_lds_bytes below. */
int dss2_gemm_prop16_supported(int nrb, int nmat, int kreal, int hout, int max_nnz, int ell_width);

/* Diagnostic: the clock the chip holds under the dominant kernel.  probe != NULL (16 uint64 of device memory): every later split-plane
 * chain launch on 64-row tiles leaves {s_memtime, s_memrealtime} at the start and at the end of its workgroups 0, 256, 512, 768;
 * shader cycles over 100 MHz ticks = the in-kernel clock (bench.py: roofline.held_clock_ghz).  NULL: off (the default). */
void dss2_debug_chain_clock_probe(unsigned long long* probe);

/* ---- dropout random state.  state[2] = persistent device {seed, offset}; snapshot[2] <- the pair this forward call's
 * kernels (forward AND backward) read.  use_host_seed != 0: snapshot = {host_seed, 0} (eager mode: the host draws the seed
 * from torch's generator, so torch.manual_seed reproduces); 0: snapshot = {state.seed, state.offset++} (inside a hipGraph
 * capture, where a by-value seed would be frozen into the graph: every replay advances the device-side offset). */
int dss2_rng_next(uint64_t* state, uint64_t* snapshot, uint64_t host_seed, int use_host_seed, void* stream);
/* the mask a kernel with (snapshot, drop_id, p) applies, written out as [n_rows, h] multipliers (0 or 1/(1-p)): lets a
 * test feed the very same mask to the CPU oracle. */
int dss2_dropout_mask(const uint64_t* snapshot, int32_t drop_id, float p, int64_t n_rows, int h, float* out, int64_t ldo,
                      void* stream);
/* gradient through "dropout, then ReLU" of a contiguous [n_rows, h] layer output y (networks.py:268-269):
 * out = g * mask * (y > 0), mask = the (snapshot, drop_id, p) mask (snapshot NULL: no dropout); relu == 0: mask only. */
int dss2_gate_grad(const float* g, const float* y, float* out, int64_t n_rows, int h, const uint64_t* snapshot,
                   int32_t drop_id, float p, int relu, void* stream);
/* host helper: drop_thr / drop_scale for a dropout rate p (the one definition both sides use) */
void dss2_dropout_params(float p, uint32_t* thr, float* scale);

/* ---- one propagation hop in global memory: out[i,:] = epi(add[i,:] + sum_{e in CSR row i} w[e] T[col[e],:]).  The TAGConv
 *      path for graphs whose connected components exceed the LDS-resident tiles (> 192 buses): a layer is then one plain
 *      tile GEMM (dss2_gemm_prop, nmat = 1, the K+1 matrices side by side) and K of these hops; epilogue fields as in
 *      dss2_gemm_prop_args, applied in the same order (bias, dropout, relu, relu_src gate, add_src).  float4 lanes when h % 4 == 0 and
 *      every operand is 16-byte aligned, scalar lanes otherwise.                                                          */
typedef struct dss2_csr_axpy_args {
  const int32_t* rowptr; const int32_t* col; const float* w;
  const float* T; int64_t ldt;             /* gathered operand [N, >= h]                        */
  const float* add; int64_t ld_add;        /* optional addend (G_m of the Horner recurrence)     */
  float* out; int64_t ldo;
  const float* bias; const float* relu_src; int64_t ld_relu; const float* add_src; int64_t ld_src;
  const uint64_t* drop_state; uint32_t drop_thr; float drop_scale; int32_t drop_id; int32_t relu;
  int64_t n_rows; int32_t h; int32_t pad_;
} dss2_csr_axpy_args;
int dss2_csr_axpy(const dss2_csr_axpy_args* args_host, void* stream);

/* ---- K4: weight gradient of TAGConv / Linear -------------------------------------------- *
 * dW_m[o,i] = sum_n (P^m G)[n,o] * X[n,i]   (P = A_hat^T via the CSR by source), m < nmat,
 * db[o] = sum_n G[n,o] * (rowscale ? rowscale[n] : 1).
 * Partial sums per workgroup go to slab[n_split][nmat*hout*hin + hout]; finish with
 * dss2_reduce_slabs.  Deterministic (no float atomics).                                    */
typedef struct dss2_wgrad_args {
  const float* G; int64_t ldg; int32_t hout;
  const float* X; int64_t ldx; int32_t hin;
  const float* rowscale;
  float* slab; int32_t n_split; int32_t nmat; int32_t nrb; int32_t ntiles;
  const int32_t* tile_start;
  const int32_t* rowptrT; const int32_t* colT; const float* wT;
  int32_t max_nnz; int32_t ell_width;   /* as in dss2_gemm_prop_args, for the transposed CSR */
  const void* ell_tiles;                /* per-tile ELL slices of the transposed graph, or NULL   */
  const float* rowscale2;               /* optional [N][4] (16-byte aligned): additionally emit, for *
                                         * every m, sum_n rowscale2[n][m] G[n, o] (the gradient of  *
                                         * dss2_gemm_prop's prebias_m when rowscale2 is its          *
                                         * pre_rowscale); slab = [nmat*hout*hin][hout][nmat*hout]    */
  int32_t narrow; int32_t mfma_bf16;    /* narrow != 0 (needs nmat*hout <= 32): the propagated  *
                                         * copies P^m G are appended as extra COLUMNS of one    *
                                         * 32-wide block instead of nmat separate blocks; same  *
                                         * slab layout [nmat*hout*hin + hout].                  *
                                         * mfma_bf16: the mode word.  0: fp32 MFMA.  != 0: the  *
                                         * products on the 16-bit matrix pipe, fp32-accurate,   *
                                         * as bf16x6; (mfma_bf16 & 255) == 2: as f16x3, bits    *
                                         * 8..15 = headroom bits for the gain of the hops,      *
                                         * ceil(log2(max row sum of |P^T|^K)), bit 16 = the     *
                                         * 32-row kernel forms its hops as fp32 gathers.  Which *
                                         * kernel takes a launch is decided in ONE place and    *
                                         * can be asked: dss2_wgrad_plan below.                 */
} dss2_wgrad_args;

int dss2_wgrad(const dss2_wgrad_args* args_host, void* stream);
/* Which kernel a launch of these arguments runs and its geometry: the record the library's own dispatch launches from.
 * Families fall through in this order: narrow (args.narrow) -> f16x3 on 32-row tiles -> f16x3 on 96- .. 192-row tiles
 * -> bf16x6 -> fp32 MFMA.  The 16-bit families share one set of operand conditions (no rowscale, ELL slices, G / X /
 * rowscale2 16-byte aligned, ldg and ldx multiples of 4); a launch that misses them, or a kernel's own shape
 * conditions, takes the next family.                                                                               */
typedef enum dss2_wgrad_kernel {
  DSS2_WGRAD_NONE = 0,            /* no kernel: see dss2_wgrad_plan_t.reason                                         */
  DSS2_WGRAD_NARROW_STREAM,       /* narrow, nmat*hout <= 8: streaming kernel (un-batched launches only)           */
  DSS2_WGRAD_FP32_NARROW,         /* narrow: wgrad<nrb, 1, 1>                                                      */
  DSS2_WGRAD_FP32,                /* wgrad<nrb, nmat, nb, w8>                                                      */
  DSS2_WGRAD_BF16_64,             /* bf16x6, 64-row tiles                                                          */
  DSS2_WGRAD_BF16_32,             /* bf16x6, 32-row tiles                                                          */
  DSS2_WGRAD_BF16_TALL,           /* bf16x6, 96- .. 192-row tiles                                                  */
  DSS2_WGRAD_F16_32,              /* f16x3, 32-row tiles                                                           */
  DSS2_WGRAD_F16_TALL,            /* f16x3, 96- .. 192-row tiles                                                   */
  DSS2_WGRAD_F16_TALL_PAIR        /* ... two 32-column layers of a batch per workgroup                             */
} dss2_wgrad_kernel;
typedef struct dss2_wgrad_plan_t {
  int32_t kernel;                 /* dss2_wgrad_kernel                                                             */
  int32_t reason;                 /* kernel == NONE: the code dss2_wgrad returns (3: no tile fits LDS, 2: no such instantiation) */
  int32_t nb; int32_t w8;         /* FP32: output blocks per workgroup, eight-wave form                            */
  int32_t grid_y; int32_t z_groups;   /* the launch is n_split x grid_y x z_groups workgroups                      */
  int32_t y_slices;
  int32_t f16x3_covers;           /* an f16x3 kernel covers these operands, tile height, K, ELL width and columns, whatever the mode
                                   * word and DSS2_WGRAD_TALL_F16 say: are headroom bits worth forming (a device read) at all?       */
  uint64_t launch_lds;            /* dynamic LDS of the launch                                                     */
  uint64_t sizing_lds;            /* what callers size n_split by, together with y_slices and z_groups             */
  /* sizing_lds / y_slices are NOT always launch_lds / grid_y: they answer from the shape alone with the bf16x6
   * kernel's figures wherever that kernel's shape conditions hold and the mode word is non-zero, else with the fp32
   * kernel's LDS and 1 -- also where an f16x3 kernel takes the launch (smaller LDS; hout = 32 on tall tiles), where
   * the operands send a launch on to the fp32 kernel, and for the fp32 family's own column groups.  n_split, and
   * with it the summation order and the speed of every configuration, was tuned on these figures; sizing by the
   * kernel that runs is a separate, measured change.                                                               */
} dss2_wgrad_plan_t;
/* fills *out for a launch of args with n_layers layers (0: dss2_wgrad; >= 1: dss2_wgrad_batched, whose pointer tables are
 * not seen here -- a misaligned layer is that call's error).  args->slab and args->n_split are not read: ask first,
 * size them after.  Returns 0, or 2 for a null pointer.                                                             */
int dss2_wgrad_plan(const dss2_wgrad_args* args_host, int n_layers, dss2_wgrad_plan_t* out);
/* Readers of that record for callers that hold a shape only (operands taken as aligned, ELL slices as present where
 * ell_width > 0): sizing_lds (_ex: with the mode word, else 0), y_slices, and z_groups of an n_layers batch.        */
size_t dss2_wgrad_lds_bytes_ex(int nrb, int nmat, int hout, int hin, int max_nnz, int ell_width, int mfma_bf16);
int dss2_wgrad_y_slices(int nrb, int nmat, int hout, int hin, int ell_width, int mfma_bf16, int has_rowscale2);
int dss2_wgrad_batched_groups(int nrb, int hout, int hin, int mfma_bf16, int n_layers);

/* The same for n_layers (<= 8) layers of IDENTICAL shape and leading dimensions in one launch (one grid
 * slice per layer): Gs / Xs / slabs are HOST arrays of device pointers replacing args->G / X / slab;
 * rowscale2s (NULL, or a HOST array with NULL entries for plain layers) replaces args->rowscale2 per layer;
 * every other field of args applies to all layers.  slab_stride (elements, 0 = the dense per-layer
 * stride): distance between consecutive workgroups' partial results inside slabs[l]; with slabs[l] =
 * base + (offset of layer l) and slab_stride = the sum of the layers' lengths, ONE dss2_reduce_slabs call
 * finishes all layers (or one call per destination buffer).  The layers of a block are independent once
 * their output gradients exist; at small H a single layer cannot fill the chip.                          */
int dss2_wgrad_batched(const dss2_wgrad_args* args_host, const float* const* Gs, const float* const* Xs,
                       float* const* slabs, const float* const* rowscale2s, int64_t slab_stride, int n_layers,
                       void* stream);

/* out[j] = sum_{s < n_slabs} slab[s*stride + j], j < len, fixed order. */
int dss2_reduce_slabs(const float* slab, int n_slabs, int64_t stride, float* out, int64_t len, void* stream);

/* up to 32 such reductions in ONE launch (same fixed order per output); descs_host: HOST array, passed by value */
typedef struct dss2_reduce_desc {
  const float* slab; float* out; int64_t stride; int64_t len; int32_t n_slabs; int32_t pad_;
} dss2_reduce_desc;
int dss2_reduce_slabs_multi(const dss2_reduce_desc* descs_host, int n_desc, void* stream);

/* ---- K3: gsp_wls_edge + get_pflow, forward and backward (data.py:328-459) --------------- *
 * Phase 1 (dss2_wls_loss_partials): applies theta *= (1 - slack) IN PLACE on output[:,1]
 * (data.py:413), computes the batch-global V_hv / V_lv (data.py:335-336), the AC branch flows,
 * bus injections and the five batch sums
 *     sums[0] = sum_nodes sum_c delta^2 R^-1 lambda_c     sums[1] = sum_edges (same, edges)
 *     sums[2] = sum_nodes relu(v-1.1)+relu(0.9-v)         sums[3] = sum_edges relu(|th_ij|-0.5)
 *     sums[4] = sum_edges relu(loading-1.5)               sums[5] = N, sums[6] = E  (doubles)
 * and the per-bus residual coefficients apq[N,2] = dJ/dp_i, dJ/dq_i (times N).
 * Between the phases a data-parallel caller all-reduces sums[0..6].
 * Phase 2 (dss2_wls_loss_grad): loss scalar (data.py:450-459) and d loss / d output[N,2]
 * (gradient w.r.t. the output BEFORE the in-place masking, as autograd gives in the reference).
 * inc_rowptr/inc_ent: incidence CSR over the STORED edges: row i lists e | end<<31 for every
 * stored edge with from(e)=i (end 0) or to(e)=i (end 1), sorted by (end, e).              */
typedef struct dss2_wls_args {
  const float* input; int64_t ld_in;            /* [N,8]  data.x[:, :8]                   */
  const float* edge_input; int64_t ld_ein;      /* [E,6]  data.edge_attr[:, :6]           */
  float* output; int64_t ld_out;                /* [N,2]  model output (theta masked in place) */
  const float* node_param; int64_t ld_np;       /* [N,3]  vn_kv, slack, zero_inj          */
  const float* edge_param; int64_t ld_ep;       /* [E,7]  G,B,Gs,Bs,closed,shift,imax     */
  const float* x_mean; const float* x_std;      /* [8]                                     */
  const float* edge_mean; const float* edge_std;/* [6]                                     */
  const int32_t* efrom; const int32_t* eto;     /* [E] stored edge endpoints               */
  const int32_t* inc_rowptr; const int32_t* inc_ent;
  int64_t n_nodes; int64_t n_edges;
  float lam_v, lam_p, lam_pf, lam_reg;
  double* sums;            /* [8] device                                                  */
  double* partials;        /* [n_blocks_max*5] device scratch, n_blocks_max = 1024         */
  float* vminmax;          /* [130] device scratch: [2+2b], [3+2b] = (min, max) of vn_kv over workgroup b < 64 */
  float* apq;              /* [N,2] device scratch                                         */
  float* loss;             /* [1] device                                                   */
  float* grad_output;      /* [N,2] device, contiguous                                     */
  float* pflow;            /* optional [E,8]: get_pflow's 8 outputs per stored edge, or NULL */
  int32_t flags;           /* DSS2_WLS_* below                                             */
  uint32_t* counter;       /* DSS2_WLS_FUSED_FINISH: one device word, zero before the first use (the kernel re-zeroes it) */
  const float* gscale;     /* dss2_wls_loss_grad: optional DEVICE scalar, the upstream gradient of the loss (autograd's
                              grad_output): the kernel scales d loss / d output by it instead of a separate multiply */
  const int32_t* edge_count; /* optional DEVICE scalar: the batch's REAL edge count, which the edge means divide by and sums[6] carries
                              instead of n_edges (padded batches: n_edges counts the padding slots too); NULL: n_edges */
} dss2_wls_args;
#define DSS2_WLS_VMM_CACHED 1     /* vminmax[] already holds this node_param's partial (min, max) pairs: no vminmax launch */
#define DSS2_WLS_FUSED_FINISH 2   /* the LAST workgroup of the partials kernel to finish sums the workgroup partials in a
                                     fixed order into sums[0..7] and writes the (local-batch) loss: no finish launch (same
                                     summation order, same bits).  The partials are handed over through memory (write-through
                                     stores, a relaxed agent-scope arrival count, agent-scope loads in the last workgroup): no
                                     release fence -- on MI355X that would write back an XCD's whole L2 per workgroup (the
                                     first form of this path: 28 us at N = 61 440 against 10 + 4.7 us for two launches) */
#define DSS2_WLS_NO_LOSS_WRITE 4  /* dss2_wls_loss_grad leaves loss[0] alone */

int dss2_wls_loss_partials(const dss2_wls_args* args_host, void* stream);
int dss2_wls_loss_grad(const dss2_wls_args* args_host, void* stream);
/* loss[0] <- the loss of the batch sums[0..6] describe (after a data-parallel caller has all-reduced them) */
int dss2_wls_loss_value(const dss2_wls_args* args_host, void* stream);

/* get_pflow alone (data.py:328-390; evaluation path dss2_run.py:193-194): y[N,2] = (v, theta)
 * in physical units; writes pflow[E,8] = loading_lines, loading_trafo, P_from, Q_from, P_to,
 * Q_to, I_from, I_to.  vminmax[130] is device scratch.  apply_shift != 0: the angle difference is
 * theta_i - theta_j - edge_param[:, 5] (the reference's phase_shift=False, data.py:364-365); 0: shift = 0
 * (phase_shift=True, the default and what gsp_wls_edge uses). */
int dss2_get_pflow(const float* y, int64_t ldy, const float* node_param, int64_t ld_np,
                   const float* edge_param, int64_t ld_ep, const int32_t* efrom, const int32_t* eto,
                   int64_t n_nodes, int64_t n_edges, float* vminmax, float* pflow, int apply_shift, void* stream);

/* ---- evaluation metrics of one test batch (/root/reference/dss2_run.py:178-208), kept on the
 *      device: yhat[N,2] <- (out[:,0] * x_std[0] + x_mean[0], out[:,1] * (1 - slack)); get_pflow of the labels y and
 *      of yhat (pf_true / pf_out [E,8] as dss2_get_pflow); then
 *      acc[0..9] += rmse_v, mae_v, rmse_th, mae_th, rmse_loading, mae_loading, rmse_loading_trafos,
 *                   mae_loading_trafos, prop_std_v, prop_std_th
 *      (loadings compared where the true loading != 0; std unbiased like torch.std): the ten per-batch
 *      quantities the reference sums over its test loader, so an epoch's evaluation needs ONE device-to-host copy.
 *      scratch: dss2_eval_scratch_doubles() device doubles; vminmax: 130 device floats.                          */
int dss2_eval_batch(const float* out, int64_t ldo, const float* y, int64_t ldy, const float* node_param, int64_t ld_np,
                    const float* edge_param, int64_t ld_ep, const int32_t* efrom, const int32_t* eto,
                    int64_t n_nodes, int64_t n_edges, const float* x_mean, const float* x_std, float* yhat,
                    float* pf_true, float* pf_out, float* vminmax, double* scratch, double* acc, void* stream);
int64_t dss2_eval_scratch_doubles(void);

/* ---- batched weighted-least-squares state estimation: Gauss-Newton on the normal equations, fp64, ONE launch per solve
 *      (csrc/dss2_wls_solve.hip).  The measurement model is gsp_wls_edge's: per bus z = (V, theta, P_inj, Q_inj) with weights R^-1
 *      (x[:, 0:8]), per stored branch (P_from, Q_from) (edge_attr[:, 0:4]), de-normalised in fp64 where the normalised entry is
 *      non-zero (a de-normalised weight below 0 counts as 0); h(u) as data.py:370-376, 428-435 with shift = 0 and V_lv the batch
 *      minimum of x[:, 8].  Graph g owns buses [g n, (g + 1) n), n = nodes_per_graph -- or, with graph_ptr (the end of the struct),
 *      [graph_ptr[g], graph_ptr[g + 1]) with n an upper bound; edges never cross graphs.  Per graph
 *          J(u) = sum_buses sum_k c_k R^-1 (z - h)^2 + sum_branches sum_k w_pf R_edge^-1 (z_edge - h_edge)^2,  c = (w_v, w_v, w_p, w_p)
 *      is minimised from `init` [N, 2] = (v in p.u., theta in rad), or from v = 1, theta = 0 (init = NULL); theta at slack buses
 *      (x[:, 9] != 0) is 0 and stays 0.  Each of at most max_iter iterations forms G = H^T W H and b = H^T W r with the analytic
 *      Jacobian, replaces the slack angles' rows and columns by the identity, factorises G (Cholesky) and applies du = G^-1 b;
 *      a pivot <= 0 or not finite, or a step that is not finite, ends the graph with status 2 and the state of the previous
 *      iterate; max |du| < tol ends it with status 0; status 1 = max_iter reached (tol = 0 never stops early).
 *      One workgroup per graph with the packed gain matrix in LDS: nodes_per_graph is capped by dss2_wls_solve_lds_bytes(n) <= 160 KiB
 *      (rc 2 above it).  No atomics and a fixed summation order: two runs agree to the bit.  Allocates nothing, never synchronises. */
typedef struct dss2_wls_solve_args {
  const float* x; int64_t ldx;                    /* [N, >= 10] node tensor: 8 measurement columns, vn_kv, slack flag            */
  const float* edge_attr; int64_t ldea;           /* [E, >= 10] edge tensor: 4 measurement columns, 2 unused, G, B, Gs, Bs       */
  const float* x_mean; const float* x_std;        /* [8]                                                                          */
  const float* edge_mean; const float* edge_std;  /* [>= 4]                                                                       */
  const int32_t* efrom; const int32_t* eto;       /* [E] stored edge endpoints                                                    */
  const int32_t* inc_rowptr; const int32_t* inc_ent; /* incidence CSR as in dss2_wls_args                                         */
  int64_t n_nodes; int64_t n_edges;               /* n_edges = 0 (one-bus graphs): inc_rowptr all 0; edge_attr, efrom, eto, inc_ent may be NULL */
  int32_t nodes_per_graph; int32_t max_iter;
  double tol;
  double w_v, w_p, w_pf;
  const float* init; int64_t ld_init;             /* [N, >= 2] start in physical units, or NULL = flat start                      */
  float* state;                                   /* [N, 2]  (v, theta), contiguous                                               */
  double* objective;                              /* [G, 2]  bus part and branch part of J at the final fp64 state               */
  int32_t* iterations;                            /* [G]     updates applied                                                      */
  int32_t* status;                                /* [G]     0 converged, 1 max_iter reached, 2 factorisation failed             */
  double* last_step;                              /* [G]     max |du| of the last update applied (0 if none)                      */
  float* vminmax;                                 /* [130] device scratch                                                         */
  int32_t max_groups;                             /* > 0: at most this many workgroups (they stride over the graphs); 0: the library's choice */
  int32_t half_bandwidth;                         /* dss2_wls_solve_large alone reads it (0: its dense form, > 0: its banded form, below); every other entry ignores the word.
                                                   * This word used to be padding (pad_): a caller of dss2_wls_solve_large MUST set it to 0 for the dense form -- a struct
                                                   * that was never zeroed now selects the banded form, or gets rc 2 for a negative value */
  /* Batches that mix bus counts (every entry that takes this block).  graph_ptr = NULL: the uniform layout above.  Otherwise graph g
   * owns buses [graph_ptr[g], graph_ptr[g + 1]) and nodes_per_graph is an UPPER BOUND on a graph's bus count: LDS, workspace, the
   * workgroup's width, the grid and every size refusal go by it, and n_nodes need not be a multiple of it.  The kernel reads the two
   * words once per graph and refuses a graph with fewer than 1 or more than nodes_per_graph buses or with rows outside [0, n_nodes):
   * status 2, iterations 0, last_step 0, objective (0, 0), n_downweighted / n_removed / dof / suspect 0, chi2_limit +inf, removed -1,
   * no state or per-measurement row written; the other graphs are solved.  Measurement ids stay global; V_lv is the batch's.  */
  const int64_t* graph_ptr;                       /* [n_graphs + 1] device memory, or NULL                                        */
  int64_t n_graphs;                               /* ignored when graph_ptr is NULL                                               */
} dss2_wls_solve_args;
int dss2_wls_solve(const dss2_wls_solve_args* args_host, void* stream);
/* bytes of LDS a graph of nodes_per_graph buses needs (pure host arithmetic) */
size_t dss2_wls_solve_lds_bytes(int nodes_per_graph);

/* ---- the rest of the classical estimator on the same solve, still ONE launch (csrc/dss2_wls_bad_data.hip): the chi-square test on J,
 *      normalized residuals, removal of the largest one followed by a re-solve, and the state's standard deviation.  Per graph:
 *        1. Gauss-Newton exactly as dss2_wls_solve (`solve` is its argument block, outputs included), from init / the flat start, later
 *           from the current state;
 *        2. at the last iterate G is formed and factorised once more and inverted in place: Sigma = G^-1;
 *        3. for every ACTIVE measurement i (effective weight w_i = c_k R^-1 > 0, not removed), with h_i its Jacobian row without the
 *           slack angles' columns:  S_i = 1 - w_i h_i Sigma h_i^T (the residual sensitivity w_i Omega_ii) and
 *           rN_i = |z_i - h_i(u)| sqrt(w_i / S_i) where S_i >= s_min, 0 below it (critical measurements: the residual says nothing);
 *        4. dof = #active - #free states, chi2_limit = dof (1 - 2 / (9 dof) + z_p sqrt(2 / (9 dof)))^3 (Wilson-Hilferty; +inf for
 *           dof <= 0), suspect = J > chi2_limit with J the objective at the final state;
 *        5. the arg-max of rN (ties: the smallest id; a NaN wins): if it exceeds `threshold` and fewer than max_removals measurements
 *           are gone, its id and rN are recorded, its weight is 0 from here on, and the graph goes back to 1.
 *      A failed factorisation in any solve or in 2. ends the graph with status 2: the state of the previous iterate (in 2.: the last
 *      one), the removals so far, per-measurement outputs and state_std 0.  Measurement ids (int32): 4 i + k for bus i (global row), k in V, theta, P, Q;
 *      4 N + 2 e + k for stored branch e, k in P_from, Q_from; rc 2 where 4 N + 2 E does not fit.  iterations counts the updates of
 *      all solves; status and last_step are the last solve's.  No atomics, one writer per value, fixed summation orders.
 *      TWO FORMS behind the one entry, chosen by `workspace`:
 *        workspace == NULL   the gain matrix, and then Sigma, on the packed triangle in LDS: dss2_wls_solve's kernel geometry and size
 *                            limit with a fixed block on top (dss2_wls_bad_data_lds_bytes(n) <= 160 KiB: 99 buses; rc 2 above).
 *        workspace != NULL   the blocked form for 1 to dss2_wls_large_max_nodes() buses (256): dss2_wls_solve_large's layout, geometry
 *                            (256 threads, dss2_wls_large_groups(&solve) workgroups, max_groups honoured) and workspace --
 *                            dss2_wls_large_workspace_bytes(nodes_per_graph, dss2_wls_large_groups(&solve)) bytes, 16-byte aligned,
 *                            contents irrelevant before and after: G is inverted in place on its block rows, as in LDS, so the solve's
 *                            slice is all it needs.  rc 2 with a message, before any launch, for a misaligned or short workspace, n
 *                            above the cap, or what the other form refuses of the parameters.  Runs, batch positions and group
 *                            counts agree to the bit; the two forms agree to rounding (another summation order), not to the bit.
 *        workspace != NULL and solve.half_bandwidth > 0
 *                            the banded form (csrc/dss2_wls_banded.hpp, dss2_wls_solve_large's banded form below): the same rounds on
 *                            rows that keep a band of G, beyond 256 buses.  Sigma is wanted only at the diagonal and between buses
 *                            within two branches of each other -- inside the band -- and the entries of G^-1 inside the band of a
 *                            banded Cholesky factor follow from L by the selected-inverse recurrence, block column by block column
 *                            from the last, in place (csrc/dss2_wls_banded_invert.hpp).  Workspace as for the banded solve; LDS is the
 *                            banded solve's plus the fixed block (320 bytes), which is the cap on (n, hb).  Equal-size graphs only
 *                            (graph_ptr: rc 2).  A graph with a non-zero outside the declared band: status 2, 0 iterations, objective
 *                            0, its start as its state, dof 0, no removal, its per-measurement rows and its slice not written.
 *                            The kernel works on the graph as it is numbered here; bus_label, if given, translates a removed BUS
 *                            measurement's id for `removed` alone: 4 bus_label[id / 4] + id % 4 (branch ids are the stored order's
 *                            either way).  The arg-max and its ties (the smallest id) go by the ids as numbered here.  */
typedef struct dss2_wls_bad_data_args {
  dss2_wls_solve_args solve;
  double threshold;                               /* > 0: the largest normalized residual is removed above it                     */
  double z_p;                                     /* the standard normal quantile of the test's confidence                        */
  double s_min;                                   /* in (0, 1): sensitivities below it give rN = 0                                */
  int32_t max_removals; int32_t pad_;             /* 0 .. 64                                                                      */
  const int32_t* bus_label;                       /* [N] or NULL; the banded form only: the caller's row of the kernel's row k    */
  int32_t* dof;                                   /* [G]                                                                          */
  double* chi2_limit;                             /* [G]                                                                          */
  int32_t* suspect;                               /* [G]     J > chi2_limit                                                       */
  int32_t* removed;                               /* [G, max(max_removals, 1)] ids in the order of removal, -1 in unused slots    */
  double* removed_rn;                             /* [G, max(max_removals, 1)] their normalized residuals when removed, 0 unused  */
  int32_t* n_removed;                             /* [G]                                                                          */
  double* bus_rn; double* bus_sens;               /* [N, 4]  rN and S of the final solve, 0 where inactive                        */
  double* edge_rn; double* edge_sens;             /* [E, 2]  (an edge that leaves its graph is not written)                       */
  double* state_std;                              /* [N, 2]  sqrt(Sigma_jj), 0 at slack angles                                    */
  void* workspace; uint64_t workspace_bytes;      /* NULL, 0: the LDS form; otherwise the blocked form's workspace (above)       */
} dss2_wls_bad_data_args;
int dss2_wls_bad_data(const dss2_wls_bad_data_args* args_host, void* stream);
/* bytes of LDS a graph of nodes_per_graph buses needs (pure host arithmetic): the solve's plus a fixed block */
size_t dss2_wls_bad_data_lds_bytes(int nodes_per_graph);

/* ---- dss2_wls_solve for graphs beyond its LDS cap (csrc/dss2_wls_large.hip): the same estimator, algorithm, outputs and decisions,
 *      still ONE launch and one workgroup per graph, with the gain matrix in a caller-provided workspace in global memory and a blocked
 *      Cholesky (16-column blocks: the diagonal block factorised by one wave, the panel below it solved by its rows' owners and kept in
 *      LDS, the trailing update on 8 x 8 register tiles) and a blocked back substitution.  It serves every bus count from 1 to
 *      dss2_wls_large_max_nodes() (256: 512 states); above it rc 2.  The workgroups stride over the graphs, each in its own slice of
 *      the workspace: dss2_wls_large_workspace_bytes(nodes_per_graph, dss2_wls_large_groups(&solve)) bytes, 16-byte aligned, contents
 *      irrelevant before and after.  No atomics, fixed summation orders: runs, batch positions and group counts agree to the bit.
 *      rc 2 with a message for a null argument, a null, misaligned or short workspace, N not a multiple of n, n above the cap.
 *      THE BANDED FORM (solve.half_bandwidth > 0, csrc/dss2_wls_banded.hpp) lifts the cap for graphs whose buses are numbered so that the gain
 *      matrix is a band: hb = half_bandwidth >= max (r - c) over the non-zeros G[r, c] (states: bus i has states 2 i and 2 i + 1; G
 *      couples the buses within two branches of each other).  Same kernel steps, decisions and outputs on another layout: block row R
 *      (16 states) keeps only the block columns R - Wb .. R, Wb = ceil(hb / 16), the right-hand side is a row of its own, and the
 *      factorisation, the panel in LDS and the back substitution stay inside the band.  With nb = ceil(2 n / 16):
 *        workspace   groups * (256 nb (Wb + 1) + 16 nb) * 8 bytes, groups = min(graphs, DSS2_WLS_BAND_GROUPS, max_groups if > 0)
 *        LDS         (16 (16 Wb + 8) + 16 * 16 + 16 + 4 n) * 8 + 16 + 16 ceil(n / 16) bytes <= DSS2_WLS_BAND_LDS_BYTES: the cap on (n, hb)
 *      Equal-size graphs only (graph_ptr: rc 2).  A graph with a non-zero outside the declared band is not assembled: status 2,
 *      0 iterations, its start as its state; nothing is written outside its slice, and the other graphs are solved.  rc 2 with a
 *      message for half_bandwidth < 0, (n, hb) above the cap, a short workspace and what the dense form refuses of the rest.
 *      half_bandwidth = 0 is the dense form above, unchanged.  */
#define DSS2_WLS_BAND_BLOCK 16           /* states of a block row and of a block column */
#define DSS2_WLS_BAND_GROUPS 512         /* workgroups at most */
#define DSS2_WLS_BAND_LDS_BYTES 163840   /* the LDS of a workgroup */
#define DSS2_WLS_BAND_BAD_DATA_BYTES 320 /* what dss2_wls_bad_data's banded form keeps in LDS behind the banded solve's */
typedef struct dss2_wls_large_args {
  dss2_wls_solve_args solve;                      /* as for dss2_wls_solve                                                        */
  void* workspace; uint64_t workspace_bytes;
} dss2_wls_large_args;
int dss2_wls_solve_large(const dss2_wls_large_args* args_host, void* stream);
/* bytes of workspace `groups` workgroups need for graphs of nodes_per_graph buses (pure host arithmetic; 0 for a bus count not served) */
size_t dss2_wls_large_workspace_bytes(int nodes_per_graph, int64_t groups);
/* the number of workgroups dss2_wls_solve_large will launch for these arguments (max_groups honoured); 0 for arguments it refuses */
int64_t dss2_wls_large_groups(const dss2_wls_solve_args* solve);
int dss2_wls_large_max_nodes(void);
/* bytes of LDS a graph of nodes_per_graph buses needs (pure host arithmetic) */
size_t dss2_wls_large_lds_bytes(int nodes_per_graph);

/* ---- the Huber M-estimator on the same kernels (csrc/dss2_wls_robust.hip): iteratively re-weighted Gauss-Newton, ONE launch.  With
 *      w_i = c_k R^-1 the weight dss2_wls_solve gives measurement i, r_i = z_i - h_i(u) and t_i = sqrt(w_i) |r_i| at the current
 *      iterate, the factor q_i is gamma / t_i where t_i > gamma and the iteration's number (from 0) is >= plain_iters, and 1 elsewhere
 *      (a NaN and a weight of 0 keep 1); an iteration is dss2_wls_solve's with w_i q_i in place of w_i in G and b.  Start, slack
 *      angles, pivot test, decision, statuses and max_groups are dss2_wls_solve's; gamma = +inf gives its five outputs to the bit.
 *      At the final state, with weighting on: solve.objective is the Huber cost sum rho(t_i), rho = t^2 (dss2_wls_solve's term) up to
 *      gamma and 2 gamma t - gamma^2 above, split into bus part and branch part; q per measurement; the count of q < 1 per graph.
 *      dss2_wls_robust keeps the gain matrix in LDS (dss2_wls_solve's size limit; workspace unused); dss2_wls_robust_large is the
 *      blocked form with dss2_wls_solve_large's workspace (dss2_wls_large_workspace_bytes, dss2_wls_large_groups) and size limit.
 *      dss2_wls_robust_large with solve.half_bandwidth > 0 is the banded form of dss2_wls_solve_large with this weighting (same
 *      workspace, LDS, cap and refusals; the per-bus counts of q < 1 pass through the first n ints of the workgroup's slice).
 *      No atomics, fixed summation orders.  rc 2 with a message for what the plain entries refuse, gamma not > 0 (a NaN included),
 *      plain_iters < 0, a null output. */
typedef struct dss2_wls_robust_args {
  dss2_wls_solve_args solve;                      /* as for dss2_wls_solve; objective is the Huber cost                           */
  double gamma;                                   /* > 0; +inf: the plain estimator                                               */
  int32_t plain_iters; int32_t pad_;              /* >= 0: the first plain_iters iterations run with q = 1                        */
  double* bus_q;                                  /* [N, 4]  q of (V, theta, P, Q) at the final state                             */
  double* edge_q;                                 /* [E, 2]  q of (P_from, Q_from) (an edge that leaves its graph is not written) */
  int32_t* n_downweighted;                        /* [G]     measurements with q < 1                                              */
  void* workspace; uint64_t workspace_bytes;      /* dss2_wls_robust_large only                                                   */
} dss2_wls_robust_args;
int dss2_wls_robust(const dss2_wls_robust_args* args_host, void* stream);
int dss2_wls_robust_large(const dss2_wls_robust_args* args_host, void* stream);

/* ---- batched small dense products in weight space (folding the edge MLP's second Linear into conv 0
 *      and the chain rule back): C[M,N] (+)= sum_b op(A_b)[M,K] . op(B_b)[K,N]  (+ u[i] * v[j]).     */
typedef struct dss2_sgemm_desc {
  const float* A[4]; const float* B[4];    /* nbatch <= 4 operand pairs, summed                 */
  float* C;
  const float* u; const float* v;          /* optional rank-1 term                              */
  int64_t c_off;                           /* >= 0: C = base_out + c_off (elements); < 0: use C */
  int32_t M, N, K, lda, ldb, ldc, transA, transB, nbatch, accumulate;
} dss2_sgemm_desc;

/* max_tiles = max over the descriptors of ceil(M/32) * ceil(N/32); descs is a DEVICE array */
int dss2_small_gemm(const dss2_sgemm_desc* descs, int n_desc, int max_tiles, float* base_out, void* stream);

/* ---- dataset side: what sits in front of the path in every training step.
 *      Replaces the arithmetic of data_from_pickles (/root/reference/data.py:119-190) and the
 *      torch_geometric DataLoader collation the driver relies on (/root/reference/dss2_run.py:68-69,134).
 *      Samples of one case have uniform shapes (n buses, e closed branches).                            */

/* measurement model, nodes (data.py:119-141).  nodes [rows][7] float64 = (vm_pu, va_rad, p_mw, q_mvar, vn_kv,
 * bool_slack, bool_zero_inj); meas_v_mask [n_per_sample] bytes (1 = voltage magnitude measured at that bus);
 * z [rows][4] float64 standard-normal draws (the reference's np.random.normal(0, |std|) = z * |std|).
 * x [rows][11] float32 <- (V, 1/var, theta, 1/var, P, 1/var, Q, 1/var, vn_kv, bool_slack, bool_zero_inj),
 * NOT yet normalised.  float64 arithmetic rounded once, like numpy.  A NaN in a raw value gives a NaN
 * measurement AND a NaN weight (the reference's torch.maximum and cap keep it), never a weight of 0.       */
int dss2_measure_nodes(const double* nodes, const uint8_t* meas_v_mask, int32_t n_per_sample, const double* z,
                       double v_noise, double pm_noise, double p_noise, double zero_inj_coef, float* x, int64_t rows,
                       void* stream);

/* measurement model, closed branches (data.py:144-167).  edges [rows][11] float64 = (from_bus, to_bus, p_from_mw,
 * q_from_mvar, G, B, Gs, Bs, closed line, phase shift, imax or sn); z [rows][2].
 * edge_attr [rows][13] float32 <- (P, 1/var, Q, 1/var, G, B | G, B, Gs, Bs, closed, shift, imax_or_sn).     */
int dss2_measure_edges(const double* edges, const uint8_t* meas_pflow_mask, int32_t e_per_sample, const double* z,
                       double p_noise, float* edge_attr, int64_t rows, void* stream);

/* masked z-score (data.py:179-190): for the first num_feat (<= 16) columns, mean / std over the NON-ZERO entries,
 * out = nan_to_num((t - mean) * (t != 0) / std); the other columns are copied.  mean/stdv [num_feat] are written
 * (nan -> 0, +-inf -> +-FLT_MAX like the reference); both are the exact double sum divided in double and rounded
 * to float once, so a column of one repeated value has that value as its mean and std 0.  In place allowed
 * (out == t, ld_out == ld); out of place every output row takes ld values, so ld_out >= ld (cells [ld, ld_out) of a
 * row are not written); any other ld_out returns 2.  scratch: device doubles,
 * dss2_masked_zscore_scratch_doubles(rows) of them.  Deterministic (fixed-order double partial sums).     */
int dss2_masked_zscore(const float* t, int64_t rows, int32_t ld, int32_t num_feat, float* out, int32_t ld_out,
                       float* mean, float* stdv, double* scratch, void* stream);
int64_t dss2_masked_zscore_scratch_doubles(int64_t rows);

/* batch collation (PyG Batch semantics): for slot b of the batch and sample s = sample_ids[b] (NULL: s = b),
 * kind 0: dst[b][0..chunk) = src[s][0..chunk)                    (float rows of x / edge_attr / y, chunk floats)
 * kind 2: the same for int32 words                                (per-sample edge counts of a padded store, chunk = 1)
 * kind 1: dst[r][b*chunk + j] = src[s][r][j] + b * nodes_per_sample   (int64 edge_index, chunk = e; shared != 0:
 *         every sample uses the one [2][e] list at src).   descs_host: HOST array of 1..4 descriptors, passed
 *         to the kernel by value (no descriptor copy); sample_ids: DEVICE int64 [batch].                     */
typedef struct dss2_collate_desc {
  const void* src; void* dst;
  int32_t chunk; int32_t kind; int32_t shared; int32_t pad_;
  int64_t nodes_per_sample;
} dss2_collate_desc;
int dss2_collate(const dss2_collate_desc* descs_host, int32_t n_desc, const int64_t* sample_ids, int64_t batch, void* stream);
/* The same collation with the batch's position on the DEVICE (host-free epochs: dss2_run.py:131-147's loop as N replays of one
 * recorded step).  cursor: DEVICE int64[2] = {position, epoch length}; slot b reads sample_ids[(cursor[0] + b) mod cursor[1]]
 * (cursor[1] <= 0: no wrap).  advance != 0: a one-thread launch behind the collation moves cursor[0] forward by `batch` (wrapping
 * at cursor[1]: cursor[0] <- (cursor[0] + batch) mod cursor[1], also when batch exceeds the epoch length), so the identical
 * pair of launches, replayed, walks the epoch -- which is why this entry point is recorded into
 * launch plans and captured into hipGraphs like every other launch of a step.  The caller re-draws sample_ids (a device
 * permutation) and zeroes cursor[0] between epochs; nothing is read back. */
int dss2_collate_cursor(const dss2_collate_desc* descs_host, int32_t n_desc, const int64_t* sample_ids, int64_t* cursor,
                        int64_t batch, int advance, void* stream);
/* acc[0] += value[0]; acc[1] += 1 (DEVICE double[2], DEVICE float): the running sum of the step losses of an epoch
 * (dss2_run.py:146-147: `total_loss += loss.item()`, without the host read) as a launch of this library, so that a recorded step
 * carries it. */
int dss2_accum_scalar(double* acc, const float* value, void* stream);

/* Ragged collation for batches that mix cases with different closed-branch counts per sample (BASELINE config C5):
 * one call per case; item j < count is the j-th sample of that case in the batch: sample samp[j] of the case's store,
 * written at node row node_off[j] / edge row edge_off[j] of the batch (DEVICE int64 arrays, uploaded by the host, which
 * decides the batch composition and reads nothing back).  Descriptor fields are re-used:
 *   kind 0: chunk floats per sample; nodes_per_sample = floats per ROW of dst; shared != 0: an edge-row operand
 *           (offset by edge_off), else a node-row operand (node_off);
 *   kind 1: edge_index, chunk = e of this case; dst[r][edge_off[j] + k] = src[samp[j]][r][k] + node_off[j] with dst row
 *           stride e_total (shared != 0: one [2][e] list for every sample). */
int dss2_collate_ragged(const dss2_collate_desc* descs_host, int32_t n_desc, const int64_t* samp, const int64_t* node_off,
                        const int64_t* edge_off, int64_t count, int64_t e_total, void* stream);
/* The same for up to 4 cases in ONE launch (round 6): descs_host[n_cases][n_desc], per case its three DEVICE tables and its item count
 * (HOST arrays of pointers / counts).  A mixed batch is then one upload and one launch. */
int dss2_collate_ragged_multi(const dss2_collate_desc* descs_host, int32_t n_cases, int32_t n_desc, const int64_t* const* samp,
                              const int64_t* const* node_off, const int64_t* const* edge_off, const int64_t* count, int64_t e_total,
                              void* stream);

/* ---- whole-stack kernels ("keep a graph resident in LDS across all L blocks") -------------------
 * /root/reference/networks.py:340-388 (PFN / SkipPFN: PFN-L chained MPN / SkipMPN blocks on the same edge inputs) and
 * :212-338 (one block), for the reference driver's own model line (dss2_run.py:72-88: dim_hid 32, K = 2, 8 layers,
 * 5 blocks, dropout 0.3).  One launch walks a tile of whole graphs through EVERY block of the stack: edge MLP ->
 * aggregation -> the H -> H TAGConv layers (conv 0 on the aggregated hidden with the edge MLP's second Linear folded
 * in) -> the narrow head -> residual, the 8-wide block output handed to the next block in LDS.  The backward launch
 * walks the same tiles through the blocks in reverse with data- and weight-gradients fused (weight gradients stay in
 * MFMA accumulators / LDS across a workgroup's tiles; one slab per workgroup and block, summed in a fixed order by
 * dss2_stack_reduce, which also applies the chain rule of the fold).  Covers dim_hid == 32, K == 2, dim_featn == 8,
 * dim_feate == 6, block output widths <= 8, 2..8 layers per block, tiles of <= 64 rows with ELL slices; every other shape
 * runs the per-block kernels above.
 *
 * params: DEVICE table of the blocks' parameter pointers in MPN._params() order, per block
 *   [W1 (hid x 22), b1, W2 (hid x hid), b2, then per conv: bias, W_0, W_1, W_2]  = 4 + 4 * (n_hh + 1) pointers.
 * wpack: uint32 scratch of dss2_stack_wpack_words() elements, rewritten by dss2_stack_pack every step (weights change).
 * Gradient layout of dss2_stack_reduce's output = the blocks' flat layouts back to back, per block
 *   [W1 | b1] [W2 | b2] then per conv [W_0 W_1 W_2 | bias]   (networks.MPN._flat_offsets). */
typedef struct dss2_stack_dims {
  int32_t n_blocks;        /* MPN blocks in the stack (1: a single MPN / SkipMPN) */
  int32_t n_hh;            /* H -> H TAGConv layers per block = n_gnn_layers - 1, 1..7 */
  int32_t dout_inner;      /* output width of blocks 0 .. n_blocks-2 (= dim_featn = 8) */
  int32_t dout_last;       /* output width of the last block, <= 8 */
  int32_t skip_inner;      /* SkipMPN residual on the inner blocks */
  int32_t skip_last;       /* ... on the last block (a standalone SkipMPN) */
} dss2_stack_dims;

typedef struct dss2_stack_args {
  dss2_stack_dims dims;
  const float* x; int64_t ldx;               /* [N, 8] input of block 0 */
  const float* ea; int64_t ldea;             /* [E, 6] stored edge features */
  const uint32_t* wpack;
  const int32_t* tile_start; int32_t ntiles; int32_t tm;      /* tm = 32 * nrb: row stride of the ELL tile slices */
  const int32_t* ell_w; const int32_t* ell_e; int32_t ell_width;        /* by target: {local col, weight} / {local col, ent} */
  const int32_t* ellT_w; const int32_t* ellT_e; int32_t ellT_width;     /* by source (backward only) */
  const float* deg_pows;                     /* [N, 4] column m = A^m deg */
  float* eacache;                            /* [ntiles][ell_width + ellT_width][64][8]: per-tile gathered, sign-corrected edge_attr
                                                rows; written by dss2_stack_pack (tiles != NULL), read by forward and backward */
  float* xs;                                 /* [n_blocks][N][8]: slot b = input of block b (slot 0 unused) */
  float* acts;                               /* [n_blocks][n_hh + 1][N][32]: slot 0 = aggregated hidden S, slot l = h_l */
  float* out; int64_t ldo;                   /* forward: [N, dout_last] */
  const float* gout; int64_t ldg;            /* backward: gradient of out */
  float* dxbuf;                              /* backward scratch [N][8]: gradient between blocks */
  float* dx_out;                             /* backward, optional: gradient of x [N][8] */
  float* slab; int64_t slab_stride; int32_t n_wg;     /* backward: n_wg persistent workgroups, one slab each */
  const uint64_t* drop_state; uint32_t drop_thr; float drop_scale; int32_t drop_stride;   /* mask id = b * drop_stride + l + 1 */
  int64_t n_nodes;
} dss2_stack_args;

int64_t dss2_stack_wpack_words(const dss2_stack_dims* dims);
int64_t dss2_stack_flat_floats(const dss2_stack_dims* dims);
/* 1 when the shape is covered (see above); 0 otherwise (the caller then runs the per-block kernels) */
int dss2_stack_supported(const dss2_stack_dims* dims, int hid, int nmat, int fn, int fe, int nrb, int ell_width, int ellT_width);
/* fold (Wf_m = W_m W2, bf_m = W_m b2 of conv 0), bf16x3 fragment packing of every matrix for the forward and the
 * data-gradient GEMMs, copies of W1 / b1 / biases -- ONE launch per step.  rng_state / rng_snapshot (optional): the
 * dropout state hand-over of dss2_rng_next done by the same launch.  tick (optional): *tick += 1 (the device-side step
 * count of a capturable optimizer). */
int dss2_stack_pack(const dss2_stack_dims* dims, const float* const* params, uint32_t* wpack, uint64_t* rng_state,
                    uint64_t* rng_snapshot, uint64_t host_seed, int use_host_seed, float* tick,
                    const dss2_stack_args* tiles, void* stream);
/* tiles (optional, the forward's argument struct): the same launch also gathers args->eacache from args->ea through the two
 * ELL slices (edge_attr changes per batch, the weights per step: both are per-forward work).  NULL: weights only (a backward
 * that has to re-pack because another forward ran in between). */
int dss2_stack_forward(const dss2_stack_args* args, void* stream);
int dss2_stack_backward(const dss2_stack_args* args, void* stream);
/* flat[i] = sum over the n_slabs slabs (fixed order; slab_stride a multiple of 4), then the chain rule of the fold: conv 0's
 * and W2 / b2's gradients from the folded ones (dW_m = dWf_m W2^T + dbf_m (x) b2; dW2 = sum_m W_m^T dWf_m;
 * db2 = sum_m W_m^T dbf_m).  Two launches. */
int dss2_stack_reduce(const dss2_stack_dims* dims, const float* slab, int32_t n_slabs, int64_t slab_stride,
                      const float* const* params, float* flat, float* fold_scratch, void* stream);
int64_t dss2_stack_fold_scratch_floats(const dss2_stack_dims* dims);      /* size of fold_scratch (device floats) */

/* ---- optimizer step (/root/reference/dss2_run.py:91-92,143: Adamax, lr 3e-3, and the other optimizers of torch.optim
 * a user puts into the driver's `getattr(optim, NAME)`: Adam / AdamW, RMSprop, SGD).  ONE multi-tensor kernel templated on the rule, the
 * arithmetic of torch's single-tensor path (foreach=False, fused=False) in fp32, in three forms:
 *   dss2_optim_step       descs_host: HOST array, passed to the kernels by value (no descriptor copy, nothing to keep alive, safe inside
 *                         a hipGraph capture), 80 tensors per launch (80 x 48 B plus the hyper-parameters stay under 4 KB of kernel
 *                         arguments).  `step` is the 1-based step count (bias corrections 1 - beta^step).  grad pointers may be views of
 *                         the flat gradient bucket the backward produces.
 *   dss2_optim_step_dev   the same with the step count on the device (float, like torch's capturable optimizers): *step_dev is advanced
 *                         by one and then used, so the launches can be captured into a hipGraph with the rest of the step.
 *   dss2_optim_step_flat  ONE launch for any number of tensors whose gradients are views of ONE flat bucket (what every backward of this
 *                         library produces: networks._MPNFn / _PFNFn / stack._FusedStackFn): descs_dev is a DEVICE table that holds,
 *                         per tensor, the element offset of its gradient inside the bucket -- constant from step to step, so the table
 *                         is written once -- and grad_base, the bucket's address of THIS step, travels by value.  step >= 1: host-side
 *                         step count; step == 0: the count lives in *step_dev (float) and is advanced by the launch itself (its last
 *                         workgroup to finish; counter = one device word, zero before the first use), so the launch can be captured.
 *                         max_n: the largest tensor's element count; n_desc <= 65535.
 * State slots s0 / s1 / s2 (NULL where the rule does not use one):
 *   ADAM     exp_avg, exp_avg_sq, max_exp_avg_sq (AMSGRAD)        RMSPROP  square_avg, momentum_buffer (MOMENTUM), grad_avg (CENTERED)
 *   SGD      momentum_buffer (MOMENTUM)                           ADAMAX   exp_avg, exp_inf
 * lr_dev != NULL: the learning rate is read from the device (a 0-dim fp32 tensor a scheduler fills in place) instead of `lr`, so a
 * recorded step -- hipGraph or launch plan -- follows a schedule. */
enum dss2_optim_rule { DSS2_OPT_ADAM = 0, DSS2_OPT_RMSPROP = 1, DSS2_OPT_SGD = 2, DSS2_OPT_ADAMAX = 3 };
enum dss2_optim_flag {
  DSS2_OPT_AMSGRAD = 1,        /* ADAM: denominators from the running maximum of exp_avg_sq (slot 2) */
  DSS2_OPT_DECOUPLED_WD = 2,   /* ADAM: AdamW's p *= 1 - lr * wd instead of g += wd * p */
  DSS2_OPT_CENTERED = 4,       /* RMSPROP: variance around the running mean gradient (slot 2) */
  DSS2_OPT_MOMENTUM = 8,       /* RMSPROP (slot 1), SGD (slot 0) */
  DSS2_OPT_NESTEROV = 16       /* SGD */
};
typedef struct dss2_optim_hyper {
  int32_t rule; int32_t flags;
  float lr;                    /* used when lr_dev == NULL */
  float beta1, beta2;          /* ADAM / ADAMAX betas; RMSPROP: beta2 = alpha */
  float omb1, omb2;            /* 1 - beta1, 1 - beta2 as the caller rounds them (torch forms them in double) */
  float eps, weight_decay;
  float momentum, omdamp;      /* RMSPROP / SGD momentum; SGD: 1 - dampening */
  int32_t pad_;
  const float* lr_dev;
} dss2_optim_hyper;
typedef struct dss2_optim_desc {
  float* param; const float* grad; float* s0; float* s1; float* s2; int64_t n;
} dss2_optim_desc;
typedef struct dss2_optim_flat_desc {
  float* param; int64_t grad_off; float* s0; float* s1; float* s2; int64_t n;
} dss2_optim_flat_desc;
int dss2_optim_step(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper* hyper, int step, void* stream);
int dss2_optim_step_dev(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper* hyper, float* step_dev, void* stream);
int dss2_optim_step_flat(const dss2_optim_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base,
                         const dss2_optim_hyper* hyper, int step, float* step_dev, uint32_t* counter, void* stream);

/* Adamax with its own argument lists and 40-byte descriptors: ADAPTERS onto the three entry points above (rule DSS2_OPT_ADAMAX, the
 * hyper-parameters as arguments, lr from the host), same kernels, same results bit for bit, same 80 tensors per by-value launch.
 * The two by-value forms convert their table to dss2_optim_desc on the host, one allocation per call (a caller that minds it fills
 * dss2_optim_desc and calls dss2_optim_step*); like there, a descriptor with n < 0 is refused as incomplete.
 * dss2_adamax_step = dss2_optim_step, dss2_adamax_step_dev = dss2_optim_step_dev, dss2_adamax_step_flat = dss2_optim_step_flat (its
 * DEVICE table stays in the layout below; the kernel reads either).  Errors name the entry point that was called. */
typedef struct dss2_adamax_desc {
  float* param; const float* grad; float* exp_avg; float* exp_inf; int64_t n;
} dss2_adamax_desc;
typedef struct dss2_adamax_flat_desc {
  float* param; int64_t grad_off; float* exp_avg; float* exp_inf; int64_t n;
} dss2_adamax_flat_desc;
int dss2_adamax_step(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, void* stream);
int dss2_adamax_step_dev(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float* step_dev, void* stream);
int dss2_adamax_step_flat(const dss2_adamax_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, float* step_dev,
                          uint32_t* counter, void* stream);

/* ---- torch.nn.utils.clip_grad_norm_(parameters, max_norm) (2-norm, error_if_nonfinite=False) in two launches, deterministic.
 * The gradients are either a HOST table passed by value (descs_host, 192 tensors per launch: more tensors are more launches) or views
 * of one flat bucket (descs_dev: DEVICE table of {offset, n}, grad_base by value).  dss2_grad_sqsum_partials: workgroup w of n_wg walks
 * elements w * 256 + t, stride n_wg * 256, of every tensor in table order and writes ONE fp64 partial (chunk c of a by-value table:
 * partials[c * n_wg + w]); ceil(n_desc / 192) * n_wg <= 256.  dss2_grad_clip_scale: every workgroup re-adds the partials in index order,
 * total = sqrt(sum), coef = min(1, max_norm / (total + 1e-6)) in fp32 (torch's formula; a non-finite gradient gives a non-finite norm
 * and coefficient, as in torch), scales its share of the gradients in place, and workgroup 0 writes total to *norm_out.  No float
 * atomics: two runs give the same bits. */
#define DSS2_OPTIM_GRAD_CHUNK 192      /* tensors of a by-value table per launch */
#define DSS2_OPTIM_MAX_PARTIALS 256    /* launches x n_wg at most: the length of `partials` */
typedef struct dss2_grad_desc { float* grad; int64_t n; } dss2_grad_desc;
typedef struct dss2_grad_flat_desc { int64_t grad_off; int64_t n; } dss2_grad_flat_desc;
int dss2_grad_sqsum_partials(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base, int n_desc,
                             int n_wg, double* partials, void* stream);
int dss2_grad_clip_scale(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, float* grad_base, int n_desc, int n_wg,
                         const double* partials, float max_norm, float* norm_out, void* stream);

/* ---- shared by the lane-group models GAT_DSSE and GINE_DSSE: the head Linears and the outer-product weight gradients ------- *
 * The head runs inside each model's launches (csrc/dss2_lanegroup.hpp); dss2_lanegroup_wgrad is csrc/dss2_lanegroup.hip.         */
typedef struct dss2_lanegroup_head {       /* Linear(c, dense) -> Linear(dense, nout) on the last conv's output (or on hin) */
  const float* W1; const float* b1; const float* W2; const float* b2;
  const float* hin; int64_t ldhin;         /* head input when the launch has no conv (num_layers = 1) */
  float* z1; float* out; int64_t ldo;      /* forward: hidden [N][dense], output [N][nout] */
  const float* gout; int64_t ldgo; float* dz1;   /* backward: output gradient, hidden gradient [N][dense] */
  int32_t c; int32_t dense; int32_t nout; int32_t pad_;
} dss2_lanegroup_head;
#define DSS2_LANEGROUP_WGRAD_MAX_JOBS 16
typedef struct dss2_lanegroup_wgrad_job {  /* slab[s][col + o * xw + k] = sum_n G[n][o] X[n][k], then [col + gw * xw + o] = sum_n G[n][o] */
  const float* G; int64_t ldg; const float* X; int64_t ldx; int32_t gw; int32_t xw; int32_t col; int32_t pad_;
} dss2_lanegroup_wgrad_job;
typedef struct dss2_lanegroup_wgrad_args { /* node chunk s of ceil(N / n_slabs) rows -> slab row s */
  dss2_lanegroup_wgrad_job jobs[DSS2_LANEGROUP_WGRAD_MAX_JOBS];
  float* slab; int64_t n_nodes; int32_t n_slabs; int32_t slab_len; int32_t n_jobs; int32_t pad_;
} dss2_lanegroup_wgrad_args;
int dss2_lanegroup_wgrad(const dss2_lanegroup_wgrad_args* args_host, void* stream);

/* ---- GATv2 (PyG GATv2Conv, heads >= 1, concatenated or averaged) and the GAT_DSSE model (reference networks.py:113-156),      *
 * csrc/dss2_gat.hip -------------------------------------------------------------------------------------------------------------- *
 * Graph: the Topology of the edge list AS GIVEN (no doubling): CSR by target (rowptr / col = source / ent = stored edge id) and by  *
 * source (rowptrT / colT = target / entT).  add_self_loops != 0: entries with source == target are skipped and one self loop per   *
 * node is added whose edge term is the mean over the remaining incoming edges (fill_value 'mean'; 0 without any).  Lane group of   *
 * `group` (8 / 16 / 32) lanes per node: cin <= group, edge_dim <= 16, head dense / out widths <= 32; with H = heads (0 means 1)   *
 * and cout the channels of ONE head, H == 1 needs cout <= group, H > 1 needs H * Cp <= group, Cp = cout rounded up to a power of   *
 * two (a lane is head h, channel c at h * Cp + c).  Rows h * cout .. h * cout + cout - 1 of lin_l / lin_r / lin_edge / att belong  *
 * to head h; softmax per head.  concat != 0 (or H == 1): output [N][H * cout], bias[H * cout]; concat == 0: the mean over the     *
 * heads, output [N][cout], bias[cout] added after the mean.  The head Linears read a mean (or one head), not a concatenation.     *
 * The grid is n_slabs workgroups; every launch that produces weight-gradient partials writes its columns of ALL n_slabs rows of    *
 * `slab` ([n_slabs][slab_len]); one dss2_reduce_slabs(_multi) over the whole slab gives the flat gradient.  Slab columns of a     *
 * conv at slab_off, with w = H * cout and oc the output's columns: att[w], bias[oc], lin_l.weight[w][cin], lin_l.bias[w],          *
 * lin_r.weight[w][cin], lin_r.bias[w], lin_edge.weight[w][ed] (its parameter order); of the head: W1[dense][c], b1[dense],       *
 * W2[nout][dense], b2[nout].                                                                                                      */
typedef struct dss2_gat_graph {
  const int32_t* rowptr; const int32_t* col; const int32_t* ent;
  const int32_t* rowptrT; const int32_t* colT; const int32_t* entT;
  const float* ea; int64_t ldea;           /* edge attributes [E][ed] (leading dimension ldea); NULL when ed == 0 */
  int64_t n_nodes; int32_t ed; int32_t add_self_loops;
  float slope;                             /* attention LeakyReLU slope (negative_slope) */
  int32_t nonlin;                          /* after every conv: 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 Tanh */
  float* slab; int32_t n_slabs; int32_t slab_len;
} dss2_gat_graph;
typedef struct dss2_gat_conv {
  const float* att; const float* bias; const float* Wl; const float* bl; const float* Wr; const float* br; const float* We;  /* bias, bl, br, We may be NULL */
  const float* h; int64_t ldh;             /* layer input [N][cin] */
  float* y; float* m; float* s;            /* forward: output after the nonlinearity [N][oc]; per-target, per-head softmax max / sum [N][H] */
  float* dxl; float* dxr;                  /* backward: d x_l, d x_r [N][H * cout] (kept for dss2_lanegroup_wgrad) */
  float* dedge; float* dself;              /* backward: per-edge [E][H * cout] / self-loop [N][H * cout] d x_l contributions */
  int32_t cin; int32_t cout; int32_t slab_off;   /* cout: the channels of one head */
  int32_t heads;                           /* H; 0 means 1 (a zero-initialised struct of an older caller) */
  int32_t concat; int32_t pad_;            /* with H > 1: != 0 concatenates the heads, 0 takes their mean; ignored with one head */
} dss2_gat_conv;
typedef struct dss2_gat_args {
  dss2_gat_graph g;
  dss2_gat_conv up;                        /* backward: the layer whose SOURCE pass this launch runs (has_up) */
  dss2_gat_conv lo;                        /* the layer whose TARGET pass this launch runs (has_lo): forward, or backward */
  dss2_lanegroup_head head;
  int32_t has_up; int32_t has_lo; int32_t has_head; int32_t group;
  const float* gy; int64_t ldgy;           /* backward without head / up: gradient of lo's output */
  float* dh; int32_t dh_cols; int32_t pad_;  /* backward without lo: gradient of the model input [N][dh_cols], or NULL */
} dss2_gat_args;
/* forward: lo's target pass (online softmax, nonlinearity fused), then the head when has_head */
int dss2_gat_forward(const dss2_gat_args* args_host, void* stream);
/* backward: (head backward | up's source pass | gy), then lo's target pass, or the input gradient into dh */
int dss2_gat_backward(const dss2_gat_args* args_host, void* stream);

/* ---- GINE (PyG GINEConv, nn = one Linear) and the GINE_DSSE model (reference networks.py:71-111), csrc/dss2_gine.hip -------- *
 * Graph: the Topology of the edge list AS GIVEN (no doubling, no self loops added or removed), CSR by target and by source as for  *
 * GAT.  Lane group of `group` (8 / 16 / 32) lanes per node: cin, cout <= group, ed <= 16, head widths <= 32.  The grid is n_slabs *
 * workgroups.  Slab columns of a conv at slab_off: eps[1], lin.weight[cin][ed], lin.bias[cin] (ed > 0 only); of the head at its    *
 * offset: W1[dense][c], b1[dense], W2[nout][dense], b2[nout].  The nn Linear's partials go to nslab ([n_slabs][nslab_len], conv k   *
 * at nn_off: weight[cout][cin], bias[cout]); with nn_off = k * nn_len the n_slabs * n_convs rows of nn_len reduce to its gradient.  */
typedef struct dss2_gine_graph {
  const int32_t* rowptr; const int32_t* col; const int32_t* ent;
  const int32_t* rowptrT; const int32_t* colT; const int32_t* entT;
  const float* ea; int64_t ldea;           /* edge attributes [E][ed], or [E][cin] when ed == 0 (no lin: m = h_j + ea) */
  int64_t n_nodes; int32_t ed;
  int32_t nonlin;                          /* after every conv: 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 Tanh */
  float* slab; int32_t n_slabs; int32_t slab_len;
  float* nslab; int32_t nslab_len; int32_t pad_;
} dss2_gine_graph;
typedef struct dss2_gine_conv {
  const float* eps;                        /* [1], read on the device */
  const float* Wn; const float* bn;        /* nn: Linear(cin, cout) */
  const float* We; const float* be;        /* lin: Linear(ed, cin); NULL when ed == 0 */
  const float* h; int64_t ldh;             /* layer input [N][cin] */
  float* y; float* z;                      /* forward: output after the nonlinearity [N][cout]; nn's input [N][cin] */
  float* dz;                               /* backward: gradient of nn's input [N][cin] */
  int32_t cin; int32_t cout; int32_t slab_off; int32_t nn_off;
} dss2_gine_conv;
typedef struct dss2_gine_args {
  dss2_gine_graph g;
  dss2_gine_conv up;                       /* backward: the conv whose SOURCE pass this launch runs (has_up) */
  dss2_gine_conv lo;                       /* forward: the conv; backward: the conv whose node-local step this launch runs */
  dss2_lanegroup_head head;                /* the two head Linears */
  int32_t has_up; int32_t has_lo; int32_t has_head; int32_t group;
  const float* gy; int64_t ldgy;           /* backward without head / up: gradient of lo's output */
  float* dh; int32_t dh_cols; int32_t pad_;  /* backward without lo: gradient of the model input [N][dh_cols], or NULL */
} dss2_gine_args;
/* forward: lo's aggregation, nn and nonlinearity, then the head when has_head (or the head alone on head.hin) */
int dss2_gine_forward(const dss2_gine_args* args_host, void* stream);
/* backward: (head backward | up's source pass | gy), then lo's node-local step, or the input gradient into dh */
int dss2_gine_backward(const dss2_gine_args* args_host, void* stream);

/* ---- gnn_dsse (reference networks.py:11-69): PyG GCN2Conv, FAConv and TAGConv, csrc/dss2_gnn.hip ------------------------- *
 * Graph: the Topology of the edge list AS GIVEN, CSR by target and by source as for GAT, and dis[N], gcn_norm's deg^-1/2 built  *
 * once per structure by dss2_gnn_dis.  Edge weight w_e = dis[src] dis[dst].  loops != 0 (add_remaining_self_loops): entries with *
 * src == dst are skipped and every node with dis != 0 gets one loop of weight dis^2.  Every conv maps c -> c channels, c <= group *
 * (8 / 16 / 32); TAG K <= DSS2_GNN_MAX_K; head widths <= 32.  The grid is n_slabs workgroups; every launch that produces weight-   *
 * gradient partials writes its columns of ALL n_slabs rows of `slab`.  Slab columns of a conv at slab_off (its parameter order):   *
 *   GCN2  weight1[c][c] (, weight2[c][c]) -- written by its local step                                                            *
 *   FA    att_l.weight[c] (written by its source pass), att_r.weight[c] (by its local step)                                       *
 *   TAG   bias[c], lins.k.weight[c][c] for k = 0..K -- written by its local step (bias columns written even without a bias)       *
 * of the head at its offset: W1[dense][c], b1[dense], W2[nout][dense], b2[nout].                                                  */
#define DSS2_GNN_GCN2 1
#define DSS2_GNN_FA 2
#define DSS2_GNN_TAG 3
#define DSS2_GNN_MAX_K 4
typedef struct dss2_gnn_graph {
  const int32_t* rowptr; const int32_t* col; const int32_t* ent;
  const int32_t* rowptrT; const int32_t* colT; const int32_t* entT;
  const float* dis;                        /* [n_nodes] */
  int64_t n_nodes; int32_t ed;             /* ed: 0 (no edge attributes; the shared lane-group checks read it) */
  int32_t loops;
  int32_t nonlin;                          /* after every conv: 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 Tanh */
  int32_t pad_;
  float* slab; int32_t n_slabs; int32_t slab_len;
} dss2_gnn_graph;
typedef struct dss2_gnn_conv {
  int32_t kind; int32_t K;                 /* DSS2_GNN_*; K: TAG's hop count */
  const float* W[DSS2_GNN_MAX_K + 1];      /* GCN2: weight1, weight2 (NULL: shared); FA: att_l, att_r [c]; TAG: lins.k.weight [c][c] */
  const float* bias;                       /* TAG bias [c] or NULL */
  const float* h; int64_t ldh;             /* conv input [N][c] */
  const float* x0; int64_t ldx0;           /* the model input x_0 [N][c] (GCN2, FA) */
  float param;                             /* GCN2 alpha, FA eps */
  int32_t c;
  float* y;                                /* forward: output after the nonlinearity [N][c] */
  float* u;                                /* forward: GCN2 the product's input [N][c]; TAG P^k h for k = 1..K [K][N][c] */
  float* d;                                /* backward: GCN2 du [N][c]; FA dv [N][c]; TAG g_k = dv W_k [K + 1][N][c] */
  float* se; float* sn;                    /* backward, FA: s_e per edge [E], s of the added loop per node [N] */
  float* part;                             /* backward, FA: the node-local part of the input gradient [N][c] */
  int32_t slab_off; int32_t pad_;
} dss2_gnn_conv;
typedef struct dss2_gnn_args {
  dss2_gnn_graph g;
  dss2_gnn_conv up;                        /* backward: the conv whose SOURCE pass / adjoint hop this launch runs (has_up) */
  dss2_gnn_conv lo;                        /* forward: the conv; backward: the conv whose node-local step this launch runs */
  dss2_lanegroup_head head;                /* the two head Linears */
  int32_t has_up; int32_t has_lo; int32_t has_head; int32_t group;
  int32_t hop; int32_t dx0_first;          /* TAG: forward hop 1..K (0 when K = 0), backward adjoint hop K - 1..0 */
  const float* rin; float* rout;           /* TAG backward: r of hop + 1 (g_K for the first hop; NULL when K = 0), r of hop > 0 */
  const float* gy; int64_t ldgy;           /* backward without head / up: gradient of lo's output */
  float* dh; int32_t dh_cols; int32_t pad_;  /* backward without lo: gradient of the model input [N][dh_cols], or NULL */
  float* dx0;                              /* backward: with lo, the x_0-path gradient [N][c] (written when dx0_first, else added);
                                              without lo, added into dh (NULL: not) */
} dss2_gnn_args;
/* forward: lo's hop / aggregation, product and nonlinearity, then the head when has_head (or the head alone on head.hin) */
int dss2_gnn_forward(const dss2_gnn_args* args_host, void* stream);
/* backward: (head backward | up's source pass or adjoint hop | gy), then lo's local step, or the input gradient into dh */
int dss2_gnn_backward(const dss2_gnn_args* args_host, void* stream);
/* dis[i] = deg_i^-1/2 (0 when deg_i = 0) over the CSR by target: mode 0 all ones (normalize = False), 1 every entry counts,
 * 2 entries with col == i dropped and one loop added (add_remaining_self_loops) */
int dss2_gnn_dis(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int mode, float* dis, void* stream);

/* ---- MultiConvNet (reference networks.py:737-835): parallel PyG ChebConv (normalization=None), one per edge feature, with LEARNED  *
 * edge weights, csrc/dss2_cheb.hip -------------------------------------------------------------------------------------------------- *
 * Graph: a Topology, doubled by the reference's rule or as given: n_edges directed entries (perm / permT: the directed id d of a CSR  *
 * entry), n_rows stored edges (ent / entT: the stored id r; efrom / eto its endpoints); d >= n_rows is the reverse of row d - n_rows   *
 * and carries the same weight.  Entries with source == target are dropped (get_laplacian).  Conv f < n_convs has the edge weights     *
 * w[f][r].  dss2_cheb_edge_forward builds, per f: w (from the edge MLP or from w_in), deg_i = sum of w over the edges LEAVING i,       *
 * lambda = 2 max over every -w_d and every deg_i of the call (one scalar for the whole batch; the FIRST entry in the order d = 0 ..    *
 * n_edges - 1, then the nodes, on a tie), what[f][r] = 2 (-w) / lambda and dn[f][i] = 2 deg_i / lambda, +inf replaced by 0.  Then      *
 *     (A t)_i = (dn_i - 1) t_i + sum_{d: j->i} what_d t_j,   T_0 = x, T_1 = A x, T_k = 2 A T_{k-1} - T_{k-2},                          *
 *     out = sum_f (sum_{k<K} lins[k] T_k + bias)                                                                                       *
 * one node per lane group (`group` = 8 / 16 / 32 lanes, cin, cout <= group), the grid is n_slabs workgroups.  Forward hop launches 1.. *
 * K-1 (one launch, hop 0, when K = 1): hop k writes T_k of every conv and adds its products to y; the first adds the k = 0 products    *
 * and the biases, the last applies dropout (drop_id > 0) and ReLU.  Backward, with r_k the adjoint of T_k and dv the gradient of the   *
 * layer's output before dropout / ReLU: hop launches k = K-1 .. 1 (hop 0 when K = 1) of the layer `up`                                 *
 *     r_{k-1} = lins[k-1]^T dv + c_k A^T r_k - r_{k+1},  dwh_d (+)= c_k <r_k(i), T_{k-1}(j)>,  ddn_i (+)= c_k <r_k(i), T_{k-1}(i)>     *
 * (c_1 = 1, c_k = 2; acc_first != 0 stores, else adds: each entry has one owning lane group per launch), the last one hands sum_f r_0   *
 * to the local step of the layer `lo` below (dv through its gate, r_{K-1} = lins[K-1]^T dv) or writes it to dh.  The weight gradients  *
 * of the lins are outer products of dv and the saved T_k: dss2_lanegroup_wgrad.  dss2_cheb_edge_backward turns dwh / ddn into the      *
 * gradient of w (through what, dn and lambda's arg-max entry; fixed-order sums) and, with the MLP, into dz1 / a1 / dw for              *
 * dss2_lanegroup_wgrad over the n_rows stored edges.                                                                                   */
#define DSS2_CHEB_MAX_K 4                  /* Chebyshev terms of one conv (PyG's K) */
#define DSS2_CHEB_MAX_CONVS 4              /* parallel convs of one layer */
typedef struct dss2_cheb_graph {
  const int32_t* rowptr; const int32_t* col; const int32_t* ent; const int32_t* perm;
  const int32_t* rowptrT; const int32_t* colT; const int32_t* entT; const int32_t* permT;
  const int32_t* efrom; const int32_t* eto; /* [n_rows] source / target of the stored edges */
  int64_t n_nodes; int64_t n_edges; int64_t n_rows;
  int32_t ed;                              /* 0 (the shared lane-group checks read it) */
  int32_t n_convs;
  float* w; float* what;                   /* [n_convs][n_rows] */
  float* dn;                               /* [n_convs][n_nodes] */
  float* lam; int64_t* arg;                /* [n_convs]: lambda_max; its arg-max entry (d, or n_edges + i; -1 with a given lambda) */
  float* slab; int32_t n_slabs; int32_t slab_len;
} dss2_cheb_graph;
typedef struct dss2_cheb_layer {
  const float* W[DSS2_CHEB_MAX_CONVS][DSS2_CHEB_MAX_K];   /* lins.k.weight of conv f, [cout][cin] */
  const float* bias[DSS2_CHEB_MAX_CONVS];  /* [cout] or NULL */
  const float* h; int64_t ldh;             /* layer input [N][cin] */
  float* y;                                /* forward: output after dropout and ReLU [N][cout] */
  float* T;                                /* forward: T_k of conv f at ((f (K - 1) + k - 1) N) cin, k = 1..K-1; NULL when K = 1 */
  float* dv;                               /* backward: gradient of the output before dropout / ReLU [N][cout] */
  float* r[2];                             /* backward: r_k of conv f at r[k % 2] + f N cin; NULL when K = 1 */
  int32_t cin; int32_t cout; int32_t K; int32_t relu; int32_t drop_id; int32_t pad_;
} dss2_cheb_layer;
typedef struct dss2_cheb_args {
  dss2_cheb_graph g;
  dss2_cheb_layer up;                      /* backward: the layer whose adjoint hop this launch runs (has_up) */
  dss2_cheb_layer lo;                      /* forward: the layer; backward: the layer whose local step this launch runs */
  dss2_lanegroup_head head;                /* unused: these models have no head Linears (has_head must be 0) */
  int32_t has_up; int32_t has_lo; int32_t has_head; int32_t group;
  int32_t hop; int32_t acc_first;
  const float* gy; int64_t ldgy;           /* backward without up: gradient of lo's output */
  float* dh; int32_t dh_cols; int32_t pad_;  /* backward without lo: gradient of the model input [N][dh_cols], or NULL */
  float* dwh; float* ddn;                  /* backward: gradients of what per DIRECTED edge [n_convs][n_edges] and of dn [n_convs][n_nodes] */
  const uint64_t* drop_state; uint32_t drop_thr; float drop_scale;   /* dropout of the layers with drop_id > 0 */
} dss2_cheb_args;
typedef struct dss2_cheb_edge_args {
  dss2_cheb_graph g;
  const float* ea; int64_t ldea;           /* has_mlp: edge attributes [n_rows][>= 2]; w = ea[:, :2] + W2 relu(W1 ea[:, :2] + b1) + b2 */
  const float* W1; const float* b1; const float* W2; const float* b2;   /* Linear(2, hid), Linear(hid, 2) */
  const float* w_in; int64_t ldw;          /* without the MLP: the weights [n_rows][n_convs] */
  int32_t has_mlp; int32_t hid;            /* hid <= 64; the MLP needs n_convs == 2 */
  int32_t lambda_given; float lambda;      /* != 0: lambda_max is `lambda` (no gradient through it) */
  int32_t n_wg; int32_t zero_in;           /* workgroups (<= 256); backward: dwh / ddn are all zero and not read (K = 1) */
  float* pmax; int64_t* parg; float* psum; /* [n_convs][n_wg] partials of the maximum, its arg-max and the backward's sum */
  const float* dwh; const float* ddn;      /* backward, as in dss2_cheb_args */
  float* dw;                               /* backward: gradient of the weights [n_rows][n_convs] (both directions summed) */
  float* dz1; float* a1;                   /* backward, has_mlp: gradient of the hidden pre-activation and the hidden activation [n_rows][hid] */
} dss2_cheb_edge_args;
/* w, dn (holding deg), the partial maxima; then lambda, what and dn (two kernels, one after the other on the stream) */
int dss2_cheb_edge_forward(const dss2_cheb_edge_args* args_host, void* stream);
/* the partial sums of lambda's chain; then dw (and dz1, a1) */
int dss2_cheb_edge_backward(const dss2_cheb_edge_args* args_host, void* stream);
/* forward hop args.hop of the layer lo */
int dss2_cheb_forward(const dss2_cheb_args* args_host, void* stream);
/* backward: (adjoint hop args.hop of up | gy), then lo's local step, or the input gradient into dh */
int dss2_cheb_backward(const dss2_cheb_args* args_host, void* stream);

/* LDS bytes a dss2_gemm_prop / dss2_wgrad launch will request (host-side helper; lets the
 * caller reject configurations that do not fit the 160 KiB LDS before launching). */
size_t dss2_gemm_prop_lds_bytes(int nrb, int nmat, int kpad, int ncg, int max_nnz, int ell_width);
size_t dss2_wgrad_lds_bytes(int nrb, int nmat, int hout, int hin, int max_nnz, int ell_width);

#ifdef __cplusplus
}
#endif
#endif /* DSS2_HIP_H */
