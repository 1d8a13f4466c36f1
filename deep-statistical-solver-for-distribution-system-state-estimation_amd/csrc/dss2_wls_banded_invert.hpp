// The covariance on the band rows of dss2_wls_banded.hpp: wl_factor's L on the WbRows layout -> the entries of Sigma = (L L^T)^-1 INSIDE
// THE BAND, in place at every stored position of the lower band (rows 0 .. ns - 1).  wl_invert's counterpart (dss2_wls_large_invert.hpp)
// where the dense inverse, O(ns^2) doubles and O(ns^3) work, cannot be paid; its one user is the banded bad-data kernel of
// csrc/dss2_wls_bad_data.hip.  Nothing here knows of measurements.
//
// THE RECURRENCE (the selected inverse, Takahashi's).  Sigma L = L^-T is upper triangular.  For block column J (16 columns from j0), with
// P the rows below it that the band keeps -- rows.below(j0, w, ns): at most 16 Wb, the only rows where L has entries in these columns --
// and Y = L_PJ L_JJ^-1, the blocks of Sigma L below and at the diagonal give
//     Sigma_PJ = -Sigma_PP Y            Sigma_JJ = (L_JJ L_JJ^T)^-1 - Y^T Sigma_PJ = T^T T - Y^T Sigma_PJ,   T = L_JJ^-1.
// Any two rows i, k of P lie less than 16 Wb apart and right of the block column, so Sigma_PP[i, k] is a stored position (row max(i, k)
// starts at or before j0) of a block column behind J.  Taken from the last block column to the first, every Sigma_PP entry read is
// final, and the only L that step J needs -- L_JJ and L_PJ -- is what step J overwrites: it runs in place.
//
//   per block column, from the last (four barriers):
//     1. Ld <- L_JJ (one thread per entry; the identity beyond the block's width), invd
//     2. the owner of panel row i solves y L_JJ = L[i, J] in registers and writes y to the panel in LDS, ROW-MAJOR here: Yp[16 (i - first) + c]
//        (a row's place is its distance from the panel's first row; 16 x 16 Wb doubles of Pt); the last 16 threads solve e_q likewise:
//        row q of T, kept in a register until the barrier and then written over Ld, which nobody reads any more
//     3. thread (i, c4) forms Sigma[i, j0 + 4 c4 .. + 3] = 0 - sum_{k in P, ascending} Sigma_PP[i, k] Y[k, .]: one global load (the same address in
//        four lanes) and two 16-byte LDS loads for four multiply-adds, 4 |P| such sums spread over the workgroup -- at Wb = 1 a row owner per
//        panel row would leave 240 threads idle, and the factorisation's 8 x 8 tiles would leave 248 -- written over L_PJ (read last in 2.)
//     4. thread (a, b) of the 256 forms Sigma[j0 + a, j0 + b] = sum_m T[m, a] T[m, b] - sum_{k in P, ascending} Y[k, a] Sigma[k, j0 + b]
//        (the rows of 3., read 16 wide) and writes it where b <= a < w
// 4 ceil(ns / 16) + 1 barriers in all, each in uniform control flow; every trip count depends on (ns, Wb) alone.  One writer per value,
// no atomics, every sum in a fixed order that depends on (ns, Wb, position) alone.  Never read: the b row, the padding rows, the columns
// left of 0 in the block rows R < Wb, and what lies above the diagonal inside a diagonal block.  A slack angle's row and column of G are
// the identity, hence of L and T: its column of Y is 0, its entries of Sigma_PJ are 0 - 0 and its diagonal is 1.
#pragma once
#include "dss2_wls_banded.hpp"

namespace dss2 {

static_assert(WL_T == WL_NB * WL_NB, "wb_selinv gives the diagonal block one thread per entry");

// y L_JJ = x on the diagonal block in l.Ld (row-major) with l.invd, in place: columns from the last
__device__ __forceinline__ void wb_selinv_solve(const WlLds& l, double (&x)[WL_NB]) {
#pragma unroll
  for (int k = WL_NB - 1; k >= 0; --k) {
    x[k] *= l.invd[k];
#pragma unroll
    for (int m = 0; m < k; ++m) x[m] -= x[k] * l.Ld[k * WL_NB + m];
  }
}

// L (after wl_factor: rows 0 .. ns - 1 of the band) -> Sigma on the lower band, in place.  Starts and ends with a barrier.
// Uses l.Pt (as Yp), l.Ld, l.invd.
__device__ __forceinline__ void wb_selinv(double* __restrict__ A, const WbRows rows, const WlLds& l, int ns, int tid) {
  double* Yp = l.Pt;
#pragma unroll 1
  for (int j0 = (ns - 1) / WL_NB * WL_NB; j0 >= 0; j0 -= WL_NB) {
    const int w = ns - j0 < WL_NB ? ns - j0 : WL_NB;
    const WbPanelRows P = rows.below(j0, w, ns);       // (rows P.first .. P.end - 1; the b row is not among them here)
    const int np = P.end - P.first;                    // (0 in the last block column, the only one that may be narrower than 16)
    const int qa = tid / WL_NB, qb = tid % WL_NB;
    __syncthreads();                                   // L, or the previous step's Sigma, is written; Ld and Yp have been read
    {
      const double v = (qa < w && qb <= qa) ? rows.at(A, j0 + qa)[j0 + qb] : (qa == qb ? 1.0 : 0.0);
      l.Ld[tid] = v;
      if (qa == qb) l.invd[qa] = 1.0 / v;
    }
    __syncthreads();
    for (int i = P.first + tid; i < P.end; i += WL_T) {
      const wl_d2* lrow = reinterpret_cast<const wl_d2*>(rows.at(A, i) + j0);
      double x[WL_NB];
#pragma unroll
      for (int k = 0; k < WL_NB / 2; ++k) { const wl_d2 v = lrow[k]; x[2 * k] = v.x; x[2 * k + 1] = v.y; }
      wb_selinv_solve(l, x);
      wl_d2* yrow = reinterpret_cast<wl_d2*>(Yp + (size_t)(i - P.first) * WL_NB);
#pragma unroll
      for (int k = 0; k < WL_NB / 2; ++k) yrow[k] = wl_d2{x[2 * k], x[2 * k + 1]};
    }
    double trow[WL_NB];
    const int tq = tid - (WL_T - WL_NB);
    if (tq >= 0) {
#pragma unroll
      for (int k = 0; k < WL_NB; ++k) trow[k] = k == tq ? 1.0 : 0.0;
      wb_selinv_solve(l, trow);
    }
    __syncthreads();
    if (tq >= 0) {
#pragma unroll
      for (int k = 0; k < WL_NB; ++k) l.Ld[tq * WL_NB + k] = trow[k];
    }
#pragma unroll 1
    for (int e = tid; e < 4 * np; e += WL_T) {
      const int i = P.first + (e >> 2), c0 = 4 * (e & 3);
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const double* irow = rows.at(A, i);
#pragma unroll 1
      for (int k = P.first; k < P.end; ++k) {
        const double s = k <= i ? irow[k] : rows.at(A, k)[i];
        const wl_d2* y = reinterpret_cast<const wl_d2*>(Yp + (size_t)(k - P.first) * WL_NB + c0);
        const wl_d2 y0 = y[0], y1 = y[1];
        acc[0] += s * y0.x; acc[1] += s * y0.y; acc[2] += s * y1.x; acc[3] += s * y1.y;
      }
      wl_d2* out = reinterpret_cast<wl_d2*>(rows.at(A, i) + j0 + c0);
      out[0] = wl_d2{0.0 - acc[0], 0.0 - acc[1]};
      out[1] = wl_d2{0.0 - acc[2], 0.0 - acc[3]};
    }
    __syncthreads();
    {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < WL_NB; ++m) s += l.Ld[m * WL_NB + qa] * l.Ld[m * WL_NB + qb];
#pragma unroll 1
      for (int k = P.first; k < P.end; ++k) s -= Yp[(size_t)(k - P.first) * WL_NB + qa] * rows.at(A, k)[j0 + qb];
      if (qb <= qa && qa < w) rows.at(A, j0 + qa)[j0 + qb] = s;
    }
  }
  __syncthreads();
}

}  // namespace dss2
