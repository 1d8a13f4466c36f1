// The covariance on the blocked layout of dss2_wls_large_core.hpp: wl_factor's L on the block rows in global memory ->
// Sigma = (L L^T)^-1 IN PLACE on the same lower triangle, blocked in WL_NB = 16 rows with the panel in LDS.  Its one user today is the
// blocked bad-data kernel of csrc/dss2_wls_bad_data.hip; nothing here knows of measurements.
//
//   sweep 1   L -> X = L^-1, block row I = rows i0 .. i0 + w - 1 from the first.  The block row's own L is copied to LDS first
//             (Pt[q][k] = L[i0 + q, k] for k < i0; Ld = the diagonal block, identity beyond its width), then
//                 t[q]  = -sum_{k = j}^{i0 - 1} L[i0 + q, k] X[k, j]     (k ascending; e_{j - i0} for a column j of the diagonal block)
//                 X[I, j] = L_II^-1 t                                      (forward substitution on Ld, the arithmetic of wl_panel)
//   sweep 2   X -> Sigma = X^T X, block row I from the first.  Pt[q][k] = X[k, i0 + q] for k >= i0 (0 above the diagonal), then
//                 Sigma[i0 + q, j] = sum_{k = i0}^{ns - 1} X[k, i0 + q] X[k, j]   (k ascending)
//
// COLUMN OWNERSHIP makes both sweeps in place without a copy: thread tid owns the columns j = tid, tid + WL_T, ... of every row.  In both
// sweeps the owner of column j reads column j of the rows it has written or will write, and the panel -- the only read across columns --
// is taken from rows nobody has written in this sweep (sweep 1: block row I itself, before its step; sweep 2: rows >= i0, and a step
// writes rows i0 .. i0 + w - 1 after its panel has been read).  So the barriers guard the panel in LDS alone: two per block row and sweep,
// 4 ceil(ns / 16) + 1 in all.  For fixed k the owners read row k at consecutive columns: global memory is read in coalesced rows (16
// multiply-adds per loaded double, the next row's entry loaded one trip ahead), and an entry
// above the diagonal (inside a diagonal block), the b row (row ns) and the padding rows are never read: they may hold anything.
// A slack angle's row and column of G are the identity, hence of L, X and Sigma too.  One writer per value, no atomics, every sum in a
// fixed order that depends on (ns, j) alone.
#pragma once
#include "dss2_wls_large_core.hpp"

namespace dss2 {

static_assert(WL_T == WL_NB * WL_NB, "wl_invert loads the diagonal block with one thread per entry");

// y = L_II^-1 t on the diagonal block in l.Ld (row-major) with l.invd, in place
__device__ __forceinline__ void wl_invert_solve(const WlLds& l, double (&t)[WL_NB]) {
#pragma unroll
  for (int q = 0; q < WL_NB; ++q) {
    t[q] *= l.invd[q];
#pragma unroll
    for (int m = q + 1; m < WL_NB; ++m) t[m] -= t[q] * l.Ld[m * WL_NB + q];
  }
}

// L (after wl_factor: rows 0 .. ns - 1) -> Sigma in place.  Starts and ends with a barrier.  Uses l.Pt, l.Ld, l.invd.
// The two sweeps are the two passes of ONE loop nest, so that the accumulation -- the only hot statement -- is compiled once.
__device__ __forceinline__ void wl_invert(double* __restrict__ A, const WlLds& l, int ns, int tid) {
  const int last = (ns - 1) / WL_NB;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {               // 0: X = L^-1;  1: Sigma = X^T X
#pragma unroll 1
    for (int i0 = 0; i0 < ns; i0 += WL_NB) {
      const int w = ns - i0 < WL_NB ? ns - i0 : WL_NB, bi = i0 / WL_NB, st = WL_NB * (bi + 1);
      double* rows = A + wl_row_off(i0);
      __syncthreads();                                 // L / X is written (a pass's first step); the previous step has read its panel
      if (pass == 0) {
        for (int k = tid; k < i0; k += WL_T) {
#pragma unroll
          for (int q = 0; q < WL_NB; ++q) l.Pt[(size_t)q * l.S + k] = q < w ? rows[(size_t)q * st + k] : 0.0;
        }
        const int q = tid / WL_NB, p = tid % WL_NB;    // (WL_T = WL_NB * WL_NB threads: one per entry of the diagonal block)
        const double v = (q < w && p <= q) ? rows[(size_t)q * st + i0 + p] : (p == q ? 1.0 : 0.0);
        l.Ld[tid] = v;
        if (p == q) l.invd[q] = 1.0 / v;
      } else {
        for (int k = i0 + tid; k < ns; k += WL_T) {
          const wl_d2* xr = reinterpret_cast<const wl_d2*>(A + wl_row_off(k) + i0);
#pragma unroll
          for (int q = 0; q < WL_NB / 2; ++q) {
            const wl_d2 v = xr[q];
            l.Pt[(size_t)(2 * q) * l.S + k] = (2 * q < w && i0 + 2 * q <= k) ? v.x : 0.0;
            l.Pt[(size_t)(2 * q + 1) * l.S + k] = (2 * q + 1 < w && i0 + 2 * q + 1 <= k) ? v.y : 0.0;
          }
        }
      }
      __syncthreads();
      // the rows k the sums run over: pass 0: j <= k < i0;  pass 1: max(i0, j) <= k < ns
      const int kend = pass == 0 ? i0 : ns, kb1 = pass == 0 ? bi : last + 1;
#pragma unroll 1
      for (int j = tid; j < i0 + w; j += WL_T) {
        double t[WL_NB];
#pragma unroll
        for (int q = 0; q < WL_NB; ++q) t[q] = 0.0;
#pragma unroll 1
        for (int kb = pass == 0 ? j / WL_NB : bi; kb < kb1; ++kb) {
          const double* col = A + wl_row_off(kb * WL_NB) + j;          // (column j of a row of block row kb >= j / 16: inside its padded length)
          const int sk = WL_NB * (kb + 1), rn = kend - kb * WL_NB < WL_NB ? kend - kb * WL_NB : WL_NB;
          double xn = rn > 0 ? col[0] : 0.0;
#pragma unroll 1                       // (one row per trip, the next row's entry loaded ahead: unrolled by 2 or 4 the blocked bad-data kernel no longer fits 256 registers and spills)
          for (int r = 0; r < rn; ++r) {
            const int k = kb * WL_NB + r;
            double x = k >= j ? xn : 0.0;              // (what lies above the diagonal of a diagonal block is dropped)
            if (r + 1 < rn) xn = col[(size_t)(r + 1) * sk];
#pragma unroll
            for (int q = 0; q < WL_NB; ++q) t[q] += l.Pt[(size_t)q * l.S + k] * x;
          }
        }
        if (pass == 0) {
#pragma unroll
          for (int q = 0; q < WL_NB; ++q) t[q] = j < i0 ? -t[q] : (q == j - i0 ? 1.0 : 0.0);
          wl_invert_solve(l, t);
        }
#pragma unroll
        for (int q = 0; q < WL_NB; ++q)
          if (q < w && j <= i0 + q) rows[(size_t)q * st + j] = t[q];
      }
    }
  }
  __syncthreads();
}

}  // namespace dss2
