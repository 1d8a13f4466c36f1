// Bad-data detection and removal on the batched WLS estimator, fp64, gfx950: the solve of dss2_wls_solve.hip, then the covariance,
// residual sensitivities, normalized residuals, the chi-square test and the removal of the largest normalized residual, repeated --
// all inside ONE launch, one workgroup per graph.  Three kernels, one per place the gain matrix lives.  The LDS and the blocked kernels
// run ONE round body (bd_round) and ONE tail (bd_tail); what a round needs from a layout comes through a storage form.  The banded
// kernel spells the same round and tail out on its own layout (why: at the kernel).
//
//   kernel                          storage form         G lives in                          inverse        Sigma        serves
//   wls_bad_data_kernel<64 / 256>   BdLdsForm<T>         LDS, packed lower triangle          bd_invert      BdPacked     2 n <= 256 states
//   wls_bad_data_blocked_kernel     BdBlockForm          block rows of a workspace slice     wl_invert      BdBlockRows  1 .. 256 buses
//   wls_bad_data_banded_kernel      (its own body)       band rows of a workspace slice      wb_selinv      BdBandRows   beyond 256 buses
//
// The device functions of the solves are those of dss2_wls_core.hpp (LDS) and dss2_wls_large_core.hpp / dss2_wls_banded.hpp (rows), with a
// mask that gives a removed measurement the weight 0 everywhere it enters; the measurement pass, the arg-max, the decision and the
// outputs are those of dss2_wls_bad_data_core.hpp, with Sigma[p, q] addressed by the form's accessor.
//
//   LDS   the solve's carve of its layout, then a fixed block:
//         red   per-wave partial results of the arg-max and of the count of active measurements (4 waves at most)
//         rem   the ids removed so far (at most 64)
//
//   per round (bd_round; trip count = max_removals + 1; a graph that has stopped removing skips the body, uniformly over its workgroup)
//     1. Gauss-Newton from the state in LDS, with the removal mask (the form's gauss_newton: the very loop of the plain solve).
//     2. G at the last iterate, formed and factorised once more (refactor), then inverted IN PLACE (invert).  On the packed triangle:
//          L -> X = L^-1    column by column from the last: the column is copied to du, then row owner i forms -(X[i, j+1..i] . L[j+1..i, j]) / L[j, j]
//          X -> Sigma = X^T X   row by row from the first: thread j forms sum_{k >= i} X[k, i] X[k, j], a barrier, the row is written (rows
//                               above i are never read again, rows below are still X)
//        on the block rows wl_invert (dss2_wls_large_invert.hpp: blocked in 16 rows, the owner of a COLUMN in place of the owner of a row,
//        since 2 n may exceed the workgroup); on the band rows wb_selinv (dss2_wls_banded_invert.hpp): the entries of Sigma inside the
//        band in place of the whole inverse.  A slack angle's row and column of G are the identity, so Sigma has 1 on that diagonal and 0
//        beside it; its h entries are dropped.
//     3. thread l OWNS bus l's four measurements and the two flows of every branch bus l is the from-end of: h_i Sigma h_i^T as a double
//        sum over the (few) non-zeros of the Jacobian row, branch physics recomputed per visit as in the row accumulation.  An injection's
//        row has 2 (deg + 1) non-zeros: its quadratic form costs deg (deg + 1) / 2 + 2 deg branch evaluations.  Then the state_std row.
//     4. arg-max of rN and the count of active measurements: per thread, per wave (shuffles), thread 0 over the waves; ties go to the
//        smallest id.  Thread 0 records the removal and writes the decision; all read it after a barrier.
//   afterwards (bd_tail): state, J with the final weights, dof, the chi-square limit, suspect, the tallies.
//
// Every __syncthreads() sits in control flow that is uniform over the workgroup (failed, the round's flag and ok are uniform: every
// thread derives them from the same LDS words).  On the LDS form the thread that owns a row of Sigma is its index: 2 n <= T is checked
// at the entry.
//
// A kernel keeps what is its own: its LDS carve and workspace slice, its graph loop and how a graph is admitted (ws_range; wb_fits on
// the band), and what is said at each kernel below.
#include "dss2_wls_bad_data_core.hpp"
#include "dss2_wls_large_invert.hpp"
#include "dss2_wls_banded_invert.hpp"

namespace dss2 {

__host__ __device__ inline size_t bd_bytes(int n) { return ws_bytes(n) + BD_EXTRA_BYTES; }

// L (packed lower triangle, after ws_factor) -> Sigma = (L L^T)^-1 in place; tmp: ns doubles.  Starts and ends with a barrier.
template <int T>
__device__ __forceinline__ void bd_invert(double* __restrict__ Gp, double* __restrict__ tmp, int ns, int tid) {
  for (int j = ns - 1; j >= 0; --j) {
    __syncthreads();                     // the columns right of j are X; the previous tmp has been read
    const size_t jj = (size_t)j * (j + 1) / 2 + j;
    const double xjj = 1.0 / Gp[jj];
    for (int i = j + 1 + tid; i < ns; i += T) tmp[i] = Gp[(size_t)i * (i + 1) / 2 + j];
    __syncthreads();
    if (tid == 0) Gp[jj] = xjj;
    for (int i = j + 1 + tid; i < ns; i += T) {
      double* rowi = Gp + (size_t)i * (i + 1) / 2;
      double s = 0.0;
      for (int k = j + 1; k <= i; ++k) s += rowi[k] * tmp[k];
      rowi[j] = -s * xjj;
    }
  }
  __syncthreads();
  for (int i = 0; i < ns; ++i) {
    double s = 0.0;
    if (tid <= i)
      for (int k = i; k < ns; ++k) { const double* rowk = Gp + (size_t)k * (k + 1) / 2; s += rowk[i] * rowk[tid]; }
    __syncthreads();                     // row i has been read by everyone (rows below it are not written in this step)
    if (tid <= i) Gp[(size_t)i * (i + 1) / 2 + tid] = s;
  }
  __syncthreads();
}

struct BdBlockRows {                     // Sigma on the block rows of dss2_wls_large_core.hpp (the blocked kernel)
  const double* Sg;
  __device__ __forceinline__ double operator()(int p, int q) const {
    const int hi = p > q ? p : q, lo = p > q ? q : p;
    return Sg[wl_row_off(hi) + lo];
  }
};

// Sigma on the band rows of dss2_wls_banded.hpp, after wb_selinv: rows.at(A, hi)[lo].  A band row stores its columns from
// 16 (hi / 16 - Wb) on and nothing left of that, so it must only ever be asked for in-band positions -- and it is: bd_bus asks for the
// states of bus li and of the buses incident to it, in pairs (bus, bus), (bus, neighbour) and (neighbour, neighbour of the same bus);
// the two buses of every such pair are within two branches of each other, and wb_fits has checked, before anything of the graph was
// assembled, that every bus's block row reaches back to the lowest bus within two branches of it (a bus's two states share a block
// row).  state_std asks for the diagonal.
struct BdBandRows {
  double* A; WbRows rows;
  __device__ __forceinline__ double operator()(int p, int q) const {
    const int hi = p > q ? p : q, lo = p > q ? q : p;
    return rows.at(A, hi)[lo];
  }
};

// ---- the storage forms: what bd_round and bd_tail need from a layout.  T: the workgroup's threads; gauss_newton returns `failed`,
// refactor (G at the last iterate, formed and factorised once more) a workgroup-uniform `ok`; invert turns the factor into Sigma in
// place, which sigma() then addresses; scratch() takes the objective's per-bus parts.
template <int T_>
struct BdLdsForm {                       // G packed in LDS (dss2_wls_core.hpp)
  static constexpr int T = T_;
  const WsLds& l;
  __device__ __forceinline__ int* ctl() const { return l.ctl; }
  __device__ __forceinline__ const unsigned char* slk() const { return l.slk; }
  __device__ __forceinline__ double* scratch() const { return l.Gp; }
  __device__ __forceinline__ bool gauss_newton(const dss2_wls_solve_args& a, const WsGraph& g, int ns, int tid, const WsRemoved& mask, WsTally& t) const {
    return ws_gauss_newton<T>(a, g, l, ns, tid, mask, t);
  }
  __device__ __forceinline__ bool refactor(const dss2_wls_solve_args& a, const WsGraph& g, int ns, int tid, const WsRemoved& mask) const {
    ws_form<T>(a, g, l.Gp, ns, tid, mask);
    return ws_factor<T>(l.Gp, ns, tid);
  }
  __device__ __forceinline__ void invert(int ns, int tid) const { bd_invert<T>(l.Gp, l.du, ns, tid); }
  __device__ __forceinline__ BdPacked sigma() const { return {l.Gp}; }
};

struct BdBlockForm {                     // G on block rows (WlRows) in the workgroup's slice A of a workspace (dss2_wls_large_core.hpp)
  static constexpr int T = WL_T;
  double* A; WlRows rows; const WlLds& l;
  __device__ __forceinline__ int* ctl() const { return l.ctl; }
  __device__ __forceinline__ const unsigned char* slk() const { return l.slk; }
  __device__ __forceinline__ double* scratch() const { return l.du; }
  __device__ __forceinline__ bool gauss_newton(const dss2_wls_solve_args& a, const WsGraph& g, int ns, int tid, const WsRemoved& mask, WsTally& t) const {
    wl_gauss_newton(a, g, A, rows, l, ns, tid, t, WsNoWeight(), mask);
    return l.ctl[0] != 0 && l.ctl[1] == 0;             // (uniform: the words of the last iteration run, behind its barrier)
  }
  __device__ __forceinline__ bool refactor(const dss2_wls_solve_args& a, const WsGraph& g, int ns, int tid, const WsRemoved& mask) const {
    wl_form(a, g, A, rows, ns, tid, WsNoWeight(), mask);   // (its first barrier: ctl has been read)
    const bool ok = wl_factor(A, rows, l, ns, tid);
    if (tid == 0) l.ctl[3] = ok ? 1 : 0;                   // (wave 0's answer, made the workgroup's)
    __syncthreads();
    return l.ctl[3] != 0;
  }
  __device__ __forceinline__ void invert(int ns, int tid) const { wl_invert(A, l, ns, tid); }
  __device__ __forceinline__ BdBlockRows sigma() const { return {A}; }
};

// One round of a graph on storage form f, with the `nrem` ids in r.rem removed: steps 1 to 4 of the header.  Returns whether the graph
// removes one more (uniform; thread 0 has then recorded it at slot nrem of r.rem, removed and removed_rn); n_active is thread 0's.
// The tally is worked on in a copy and written back: that is for the code generator alone ("Resources" under the blocked form).
template <class Form>
__device__ __forceinline__ bool bd_round(const Form& f, const dss2_wls_bad_data_args& b, const WsGraph& g, const BdLds& r, int64_t gr, int slots, int n,
                                         int ns, int tid, int nrem, WsTally& tally, int& n_active) {
  constexpr int T = Form::T;
  const dss2_wls_solve_args& a = b.solve;
  WsTally t = tally;
  const WsRemoved mask = {r.rem, nrem};
  bool failed = f.gauss_newton(a, g, ns, tid, mask, t);
  if (!failed && !f.refactor(a, g, ns, tid, mask)) {
    failed = true;
    if (tid == 0) t.status = 2;
  }
  if (!failed) f.invert(ns, tid);
  BdBest best = {-1.0, 0x7fffffff};
  int cnt = 0;
  const auto Sg = f.sigma();
  for (int k = tid; k < n; k += T) bd_bus(b, g, Sg, k, mask, failed, best, cnt);
  for (int q = tid; q < ns; q += T)
    b.state_std[(g.base + (q >> 1)) * 2 + (q & 1)] = (failed || ((q & 1) && f.slk()[q >> 1])) ? 0.0 : sqrt(Sg(q, q));
  tally = t;
  return bd_decide<T>(b, r, f.ctl(), gr, slots, failed, nrem, tid, best, cnt, n_active);
}

// A graph's outputs after its rounds: the state in fp32, J at the fp64 state with the final weights, the test, the tallies.
template <class Form>
__device__ __forceinline__ void bd_tail(const Form& f, const dss2_wls_bad_data_args& b, const WsGraph& g, const BdLds& r, int64_t gr, int slots, int n,
                                        int ns, int tid, int nrem, const WsTally& t, int n_active) {
  constexpr int T = Form::T;
  ws_store_state<T>(b.solve, g, ns, tid);
  double jb, je;
  ws_objective<T>(b.solve, g, f.scratch(), tid, WsRemoved{r.rem, nrem}, jb, je);
  if (tid == 0) bd_finish(b, gr, t, jb, je, n_active, nrem, slots, f.slk(), n);
  __syncthreads();                       // the next graph of this workgroup reuses the LDS (rem and slk included)
}

// THE LDS FORM: the launch geometry of wls_solve; LDS is the solve's carve of the largest graph this launch can hold, then the fixed block.
template <int T>
__global__ void __launch_bounds__(T) wls_bad_data_kernel(const dss2_wls_bad_data_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bd_smem[];
  const dss2_wls_solve_args& a = b.solve;
  const BdLds r = bd_carve(bd_smem + ws_bytes(a.nodes_per_graph));   // behind the carve of the largest graph this launch can hold
  const int tid = threadIdx.x;
  const int slots = b.max_removals > 1 ? b.max_removals : 1;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  const int64_t n_graphs = ws_n_graphs(a);
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    const WsRange rg = ws_range(a, gr);
    if (!rg.ok) {                        // uniform over the workgroup
      if (tid == 0) bd_refuse(b, gr, slots);
      continue;
    }
    const int n = rg.n, ns = 2 * n;      // (2 n <= 2 nodes_per_graph <= T: a thread per row of Sigma)
    const WsLds l = ws_carve(bd_smem, n);
    const WsGraph g = ws_graph(rg.base, n, vlv, l.u, l.slk);
    ws_load_start<T>(a, g, l, tid);
    const BdLdsForm<T> form = {l};
    WsTally t = {0, 1, 0.0};
    int nrem = 0, n_active = 0;          // nrem is uniform; n_active is thread 0's
    bool removing = true;                // uniform
    for (int round = 0; round <= b.max_removals; ++round) {
      if (removing) {
        removing = bd_round(form, b, g, r, gr, slots, n, ns, tid, nrem, t, n_active);
        if (removing) ++nrem;
      }
    }
    bd_tail(form, b, g, r, gr, slots, n, ns, tid, nrem, t, n_active);
  }
}

static_assert(2 * (wl_lds_bytes(WL_MAX_NODES) + BD_EXTRA_BYTES) <= (size_t)kMaxLdsBytes, "two workgroups of the largest graph per CU, with the bad-data block");

// THE BLOCKED FORM (args.workspace != NULL): 1 to 256 buses per graph on the layout of csrc/dss2_wls_large.hip -- G on block rows in the
// workgroup's slice of a workspace in global memory, a block column's panel in LDS, 256 threads, the large solve's grid.  LDS is the
// large solve's carve of the bound, then the fixed block.
// (the second launch bound: two waves per SIMD, i.e. two workgroups per CU -- the compiler then keeps to 256 registers in all)
__global__ void __launch_bounds__(WL_T, 2) wls_bad_data_blocked_kernel(const dss2_wls_bad_data_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bl_smem[];
  const dss2_wls_solve_args& a = b.solve;
  // (the slice and the place of the fixed block are sized by nodes_per_graph -- with a graph_ptr: the bound -- as in wls_blocked_kernel)
  double* A = static_cast<double*>(b.workspace) + (size_t)blockIdx.x * wl_graph_doubles(a.nodes_per_graph);
  const BdLds r = bd_carve(bl_smem + wl_lds_bytes(a.nodes_per_graph));
  const int slots = b.max_removals > 1 ? b.max_removals : 1;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  const int64_t n_graphs = ws_n_graphs(a);
  // Two things here are for the register allocator alone (with either one missing the kernel spills).  The graphs
  // ws_range refuses get their outputs in a loop of their own, so that what bd_refuse needs is not kept alive across the solves; and the
  // thread's index passes through an empty asm at the head of every graph, so that addresses formed from it are formed where they are
  // used, not once before the loop and carried through it.
  int tid = threadIdx.x;
  if (tid == 0)
    for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x)
      if (!ws_range(a, gr).ok) bd_refuse(b, gr, slots);
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    asm volatile("" : "+v"(tid));
    const WsRange rg = ws_range(a, gr);
    if (!rg.ok) continue;                // uniform over the workgroup (its outputs were written above)
    const int n = rg.n, ns = 2 * n;
    const WlLds l = wl_carve(bl_smem, n);
    const WsGraph g = ws_graph(rg.base, n, vlv, l.u, l.slk);
    const WsLds start = {nullptr, nullptr, l.u, l.du, l.ctl, l.slk};
    ws_load_start<WL_T>(a, g, start, tid);
    const BdBlockForm form = {A, WlRows(), l};
    WsTally t = {0, 1, 0.0};
    int nrem = 0, n_active = 0;          // nrem is uniform; n_active is thread 0's
    bool removing = true;                // uniform
    for (int round = 0; round <= b.max_removals; ++round) {
      if (removing) {
        removing = bd_round(form, b, g, r, gr, slots, n, ns, tid, nrem, t, n_active);
        if (removing) ++nrem;
      }
    }
    bd_tail(form, b, g, r, gr, slots, n, ns, tid, nrem, t, n_active);
  }
}

static_assert(BD_EXTRA_BYTES == (size_t)DSS2_WLS_BAND_BAD_DATA_BYTES, "the header's constant is the fixed block behind the banded carve");

// THE BANDED FORM (args.workspace != NULL and solve.half_bandwidth > 0): graphs beyond 256 buses on the band rows of dss2_wls_banded.hpp,
// with the entries of Sigma inside the band -- all that steps 3 and 4 read (BdBandRows above) -- in place of the whole inverse.
// wb_fits once per graph, before anything is assembled: a graph that does not fit gets bd_refuse's outputs and its start as its state,
// and its slice stays untouched.  LDS is the banded carve, then the fixed block.
// The kernel works on the relabelled graph (estimator.band_order): the removal list in LDS, the mask and the arg-max -- hence its ties,
// which go to the smallest RELABELLED id -- keep relabelled ids.  Only `removed`, the caller's list, is translated, by the thread that
// records it: a bus measurement's id through bus_label (branch ids are the caller's already: band_order keeps the stored edge order).
// The round and the tail are bd_round's and bd_tail's steps written out here: through the shared body this kernel came out with other
// code (36 accumulator registers for 38) and measured 0.7 .. 1.1 % slower.  A change to bd_round or bd_tail is made here too.
__global__ void __launch_bounds__(WL_T) wls_bad_data_banded_kernel(const dss2_wls_bad_data_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bb_smem[];
  const dss2_wls_solve_args& a = b.solve;
  const int n = a.nodes_per_graph, ns = 2 * n, Wb = wb_blocks(a.half_bandwidth);
  double* A = static_cast<double*>(b.workspace) + (size_t)blockIdx.x * wb_graph_doubles(n, Wb);
  const WbRows rows = {WL_NB * (Wb + 1), WL_NB * Wb};
  const WlLds l = wl_carve(bb_smem, n, wb_pstride(Wb));
  const BdLds r = bd_carve(bb_smem + wb_lds_bytes(n, Wb));
  const int slots = b.max_removals > 1 ? b.max_removals : 1;
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    const WsGraph g = ws_graph(gr * n, n, vlv, l.u, l.slk);
    const WsLds start = {nullptr, nullptr, l.u, l.du, l.ctl, l.slk};
    ws_load_start<WL_T>(a, g, start, tid);
    if (!wb_fits(a, g, l.ctl, rows.shift, tid)) {      // uniform over the workgroup (its second barrier: the start is in LDS)
      ws_store_state<WL_T>(a, g, ns, tid);
      if (tid == 0) bd_refuse(b, gr, slots);
      __syncthreads();                                 // the next graph of this workgroup reuses the LDS
      continue;
    }
    WsTally t = {0, 1, 0.0};
    int nrem = 0, n_active = 0;          // nrem is uniform; n_active is thread 0's
    bool removing = true;                // uniform
    for (int round = 0; round <= b.max_removals; ++round) {
      if (removing) {
        const WsRemoved mask = {r.rem, nrem};
        wl_gauss_newton(a, g, A, rows, l, ns, tid, t, WsNoWeight(), mask);
        bool failed = l.ctl[0] != 0 && l.ctl[1] == 0;      // (uniform: the words of the last iteration run, behind its barrier)
        if (!failed) {
          wl_form(a, g, A, rows, ns, tid, WsNoWeight(), mask);   // (its first barrier: ctl has been read)
          const bool ok = wl_factor(A, rows, l, ns, tid);
          if (tid == 0) l.ctl[3] = ok ? 1 : 0;             // (wave 0's answer, made the workgroup's)
          __syncthreads();
          if (l.ctl[3] == 0) {
            failed = true;
            if (tid == 0) t.status = 2;
          }
        }
        if (!failed) wb_selinv(A, rows, l, ns, tid);
        BdBest best = {-1.0, 0x7fffffff};
        int cnt = 0;
        const BdBandRows Sg = {A, rows};
        for (int k = tid; k < n; k += WL_T) bd_bus(b, g, Sg, k, mask, failed, best, cnt);
        for (int q = tid; q < ns; q += WL_T)
          b.state_std[(g.base + (q >> 1)) * 2 + (q & 1)] = (failed || ((q & 1) && l.slk[q >> 1])) ? 0.0 : sqrt(Sg(q, q));
        removing = bd_decide<WL_T>(b, r, l.ctl, gr, slots, failed, nrem, tid, best, cnt, n_active);
        if (removing) {
          if (tid == 0 && b.bus_label) {                   // (thread 0 wrote removed[] in bd_decide: still its one writer)
            const int id = r.rem[nrem];
            if ((int64_t)id < 4 * a.n_nodes) b.removed[gr * slots + nrem] = 4 * b.bus_label[id >> 2] + (id & 3);
          }
          ++nrem;
        }
      }
    }
    ws_store_state<WL_T>(a, g, ns, tid);
    double jb, je;
    ws_objective<WL_T>(a, g, l.du, tid, WsRemoved{r.rem, nrem}, jb, je);
    if (tid == 0) bd_finish(b, gr, t, jb, je, n_active, nrem, slots, l.slk, n);
    __syncthreads();
  }
}

}  // namespace dss2

using namespace dss2;

extern "C" size_t dss2_wls_bad_data_lds_bytes(int nodes_per_graph) {
  return nodes_per_graph > 0 ? bd_bytes(nodes_per_graph) : 0;
}

static int wls_bad_data_launch(const dss2_wls_bad_data_args* bp, void* stream) {
  const dss2_wls_bad_data_args& b = *bp;
  if (b.workspace)                       // a workspace selects the forms on rows: banded or blocked by half_bandwidth (wb_route)
    return wb_route<wls_bad_data_blocked_kernel, wls_bad_data_banded_kernel, bd_check_params>(b, "wls_bad_data (blocked)", "wls_bad_data (banded)",
                                                                                              as_stream(stream), BD_EXTRA_BYTES);
  if (int rc = ws_check_args(b.solve, "wls_bad_data", BD_EXTRA_BYTES)) return rc;
  const int n = b.solve.nodes_per_graph;
  if (2 * n > 256) { set_error("wls_bad_data: %d states do not fit the workgroup that owns the covariance's rows", 2 * n); return 2; }
  if (int rc = bd_check_params(b, "wls_bad_data")) return rc;
  return ws_launch<wls_bad_data_kernel<64>, wls_bad_data_kernel<256>>(b, bd_bytes(n), "wls_bad_data", as_stream(stream));
}
extern "C" int dss2_wls_bad_data(const dss2_wls_bad_data_args* bp, void* stream) {
  return dss2::entry(wls_bad_data_launch, stream, dss2::copied(bp, "dss2_wls_bad_data"));
}
