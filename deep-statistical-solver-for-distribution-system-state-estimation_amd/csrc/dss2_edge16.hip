// Edge MLP, first Linear on the bf16 matrix pipe as bf16x6 (fp32-accurate, dss2_common.hpp: split3): forward, and the
// recomputation of the pre-activation in the backward.  gfx950.  (/root/reference/networks.py:176-181: the per-edge
// Linear(22 -> hid) + ReLU, summed per target.)
//
// dss2_edge.hip's matrix-pipe kernels run  Z_k = A_k W1^T,  A_k = [x_i | x_j | edge_attr],  as twelve v_mfma_f32_32x32x2_f32 per
// ELL slot and row block (64 cycles each), between two workgroup barriers per slot (A_k is rebuilt in LDS for every slot), and
// read the slot's validity word per accumulator element.  Here
//   * the x_i term does not depend on the slot: C_i = X_i W1a^T once per tile and row block (K = 8, one k-step of 16);
//   * a slot adds [x_j | edge_attr | 1 | invalid] W1bc^T: K = 8 + 6 + 2 = 16, ONE k-step -- six v_mfma_f32_32x32x16_bf16
//     (32 cycles each) per slot and row block, started on the accumulator C_i;
//   * the bias rides in the k = 14 column (a = 1 on valid slots, b = b1: exact, 1 is a bf16 number and b1 = h + m + l), and
//     the k = 15 column carries a = 1 on EMPTY slots against b = -1e30: an empty slot's pre-activation is hugely negative, the
//     ReLU removes it, and the epilogue is two vector instructions per element (max, add) with no validity lookups;
//   * the split planes of every slot are built in ONE phase after the staging (each input element is split once per workgroup,
//     16-byte row pieces: conflict-free b128 fragment reads without padding), so the slot loop of the forward has no barrier;
//   * 192-row tiles (end of round 5; round 6: 128-row tiles as two parts of 64 rows) are walked as two PARTS of 96 rows by the 96-row instantiations: the whole tile's x rows are staged
//     for each part (x_j may be any of them), everything else is the part's own (EdgeTileArgs::parts / xtm, edge_stage_part).
// The backward recomputes the pre-activation with the very same plane values, fragments and MFMA order -- its gates are bit for
// bit the forward's -- and forms dW1 += dZ_k^T A_k, a contraction over the tile's rows, as bf16x6 too (see edge16_bwd_kernel).
// Built without packed fp32 VALU ops like every translation unit that runs bf16 MFMAs beside other workgroups (csrc/build.sh).
#include <assert.h>

#include "dss2_edge16_tile.hpp"

namespace dss2 {

// (four waves per SIMD: the kernel waits on its staging chain tile_start -> ELL entry -> edge_attr row, and a fourth resident
//  workgroup covers more of it than the 3-8 spilled registers cost: 18.5 -> 15.6 us at C2; the backward, whose vector and matrix
//  work are balanced, lost 3 us when squeezed from two to three waves)
template <int NRB>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 8))) edge16_fwd_kernel(const EdgeTileArgs p) {
  extern __shared__ __attribute__((aligned(16))) float esm[];
  const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
  const int cg = __builtin_amdgcn_readfirstlane(tid >> 6);      // one 32-column group of the hidden layer per wave
  const int c32 = lane & 31, half = lane >> 5;
  const int D = p.D;
  const int parts = p.parts > 1 ? p.parts : 1, XT = p.xtm > 0 ? p.xtm : NRB * 32;      // (192-row tiles: two parts of 96 rows)
  E16Lds L = e16_ptrs<NRB>(esm, D, XT);
  const int j = cg * 32 + c32;
  const E16W w = e16_weights(p.W1, p.b1, j, half);
  for (int vt = blockIdx.x; vt < p.ntiles * parts; vt += gridDim.x) {
    const int tile = vt / parts, r0 = (vt - tile * parts) * (NRB * 32);
    const int ts_full = p.tile_start[tile], R_full = p.tile_start[tile + 1] - ts_full;
    const int ts = ts_full + r0;
    const int R = R_full - r0 < NRB * 32 ? R_full - r0 : NRB * 32;
    if (R <= 0) continue;      // (uniform: a part beyond the tile's rows)
    L.xi = L.s.xs + r0 * FN;
    edge_stage_part<NRB>(p, L.s, tile, XT, r0, ts_full, R_full, tid, nthreads);
    __syncthreads();
    e16_build<NRB>(L, D, tid, nthreads);
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      const f32x16 Sacc = e16_fwd_rb<NRB>(L, w, D, rb, c32, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rb * 32 + acc_row(r, half);
        if (row < R) p.S[(int64_t)(ts + row) * p.h + j] = Sacc[r];
      }
    }
    __syncthreads();      // (a workgroup that walks several tiles restages over the images)
  }
}

// ---- backward by target: dW1, db1 (slab per workgroup) and optionally U[row] = sum over incoming edges of dZ.
// dW1[o][i] += sum_rows dZ_k[row][o] A_k[row][i] is a contraction over the tile's rows, and it is bf16x6 as well (round 4; the
// fp32 form -- sixteen v_mfma_f32_32x32x2_f32 per slot and row block, dZ through a wave-private LDS tile -- took five sixths of
// the kernel's matrix-pipe time: profiles/experiments/r04_edge16_bwd_fp32_dw.hip.txt):
//   * the A operand is dZ^T: lane (o, half) of the recomputation's accumulator already holds dZ[.][o] for the sixteen rows
//     acc_row(r, half) of a row block.  Any order of the contraction index is as good as another, so k-step s takes the lane's
//     registers r = 8 s .. 8 s + 7 as they are: dZ is split in registers and never touches LDS;
//   * the B operand then needs A_k[rho][i] for the same eight rows rho = acc_row(8 s + p, half): A_k is kept as TRANSPOSED
//     planes [plane][column][row block][32 rows in that order] (a row's position is its index with bits 2 and 3 swapped), one
//     ds_read_b128 per plane.  Columns: x_i (8, once per tile -- rows of an empty slot have dZ = 0, the values need no mask),
//     then x_j | edge_attr | 1 | 0 (16, per slot); the 1 column yields db1.
// The recomputation's planes are built per slot too (the forward builds all slots at once and runs its slot loop without a
// barrier; here every slot has its barriers anyway), so a 96-row tile at D = 5 takes 52 KB instead of 130 KB and two workgroups
// share a CU.

template <int NRB, bool WITH_U>
__global__ void __launch_bounds__(512) edge16_bwd_kernel(const EdgeTileArgs p) {
  constexpr int TM = NRB * 32, CS = e16_cs(TM);
  extern __shared__ __attribute__((aligned(16))) float esm[];
  const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
  const int cg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c32 = lane & 31, half = lane >> 5;
  const int D = p.D;
  const int parts = p.parts > 1 ? p.parts : 1, XT = p.xtm > 0 ? p.xtm : NRB * 32;      // (192-row tiles: two parts of 96 rows)
  E16Bwd B = e16_bwd_ptrs<NRB>(esm, D, XT);
  E16Lds L;                           // the view e16_xterm / e16_z read: the one-slot planes are "slot 0"
  L.s = B.s; L.xi = B.xi; L.PI = B.PI; L.PK = B.PK;
  const int j = cg * 32 + c32;
  const E16W w = e16_weights(p.W1, p.b1, j, half);
  // this lane's B-operand column of the weight-gradient product: input column c32 -> x_i (0..7), the slot's columns (8..23), none
  const char* bcol = c32 < FN ? B.ATI + c32 * CS : B.ATK + ((c32 < FN + E16_ATN ? c32 : FN) - FN) * CS;
  const int bps = c32 < FN ? FN * CS : E16_ATN * CS;      // plane stride of that image
  const bool bcol_ok = c32 < FN + E16_ATN;
  f32x16 dWacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) dWacc[r] = 0.f;
  for (int vt = blockIdx.x; vt < p.ntiles * parts; vt += gridDim.x) {
    const int tile = vt / parts, r0 = (vt - tile * parts) * (NRB * 32);
    const int ts_full = p.tile_start[tile], R_full = p.tile_start[tile + 1] - ts_full;
    const int ts = ts_full + r0;
    const int R = R_full - r0 < NRB * 32 ? R_full - r0 : NRB * 32;
    if (R <= 0) continue;      // (uniform: a part beyond the tile's rows)
    B.xi = B.s.xs + r0 * FN;
    edge_stage_part<NRB>(p, B.s, tile, XT, r0, ts_full, R_full, tid, nthreads);
    f32x16 gS[NRB], Uacc[WITH_U ? NRB : 1];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rb * 32 + acc_row(r, half);
        gS[rb][r] = row < R ? p.dS[(int64_t)(ts + row) * p.h + j] : 0.f;
        if (WITH_U) Uacc[rb][r] = 0.f;
      }
    // dS is split into its three bf16 planes ONCE per tile (pairs of consecutive registers, the pairing of the weight-gradient product's
    // A fragments below); a slot then gates the PLANES with 16-bit masks -- 4 vector instructions per element and slot instead of the
    // 7.5 of selecting the gated value and splitting it again.  split3(gate ? g : 0) = gate ? split3(g) : 0 plane by plane: same bits.
    // (where the planes fit beside everything else: not with U -- the fp32 values stay live for it -- and not at 96 rows: 26 / 8 spilled
    //  registers otherwise)
    constexpr bool PRE = !WITH_U && NRB <= 2;
    uint32_t gh[PRE ? NRB : 1][8], gm[PRE ? NRB : 1][8], gl[PRE ? NRB : 1][8];
    if constexpr (PRE) {
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int j = 0; j < 8; ++j) split3_pair(gS[rb][2 * j], gS[rb][2 * j + 1], gh[rb][j], gm[rb][j], gl[rb][j]);
    }
    __syncthreads();
    e16_bwd_build_tile<NRB>(B, tid, nthreads);
    f32x16 ci[NRB];
    for (int k = 0; k < D; ++k) {
      e16_bwd_build_slot<NRB>(B, k, tid, nthreads);
      __syncthreads();
      if (k == 0) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) ci[rb] = e16_xterm<NRB>(L, w, rb, c32, half);
      }
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const f32x16 c = e16_z<NRB>(L, w, 0, rb, c32, half, ci[rb]);
        [[maybe_unused]] uint32_t mk[8];      // (PRE) the gates of registers (2 j, 2 j + 1) as a mask over the two bf16 halves of a plane word
        [[maybe_unused]] f32x16 dz;
        if constexpr (PRE) {
          e16_gate_masks(c, mk);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            dz[r] = relu_open(c[r]) ? gS[rb][r] : 0.f;
            if (WITH_U) Uacc[rb][r] += dz[r];
          }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          uint4 ah, am, al;
          if constexpr (PRE) {
            ah = uint4{gh[rb][4 * st] & mk[4 * st], gh[rb][4 * st + 1] & mk[4 * st + 1], gh[rb][4 * st + 2] & mk[4 * st + 2], gh[rb][4 * st + 3] & mk[4 * st + 3]};
            am = uint4{gm[rb][4 * st] & mk[4 * st], gm[rb][4 * st + 1] & mk[4 * st + 1], gm[rb][4 * st + 2] & mk[4 * st + 2], gm[rb][4 * st + 3] & mk[4 * st + 3]};
            al = uint4{gl[rb][4 * st] & mk[4 * st], gl[rb][4 * st + 1] & mk[4 * st + 1], gl[rb][4 * st + 2] & mk[4 * st + 2], gl[rb][4 * st + 3] & mk[4 * st + 3]};
          } else {
            split3_pair(dz[8 * st + 0], dz[8 * st + 1], ah.x, am.x, al.x);
            split3_pair(dz[8 * st + 2], dz[8 * st + 3], ah.y, am.y, al.y);
            split3_pair(dz[8 * st + 4], dz[8 * st + 5], ah.z, am.z, al.z);
            split3_pair(dz[8 * st + 6], dz[8 * st + 7], ah.w, am.w, al.w);
          }
          e16_dw_step<NRB>(ah, am, al, bcol, bps, bcol_ok, rb, st, half, dWacc);
        }
      }
      __syncthreads();   // everyone is done with the slot's planes
    }
    if (WITH_U) {
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rb * 32 + acc_row(r, half);
          if (row < R) p.U[(int64_t)(ts + row) * p.ldu + j] = Uacc[rb][r];
        }
    }
  }
  if (!p.slab) return;
  e16_store_slab(p.slab + (size_t)blockIdx.x * ((size_t)p.h * FC + p.h), p.h, cg, c32, half, dWacc);
}

bool edge16_ok(int h, int nrb, int D, bool bwd, size_t* lds) {
  if ((h & 31) || h > 256 || !(nrb == 1 || nrb == 2 || nrb == 3 || nrb == 4 || nrb == 6) || D < 1 || D > 32) return false;      // (no kernel of the library tiles at 160 rows)
  // (128- / 192-row tiles: two parts of 64 / 96 rows, the whole tile's x rows staged for each)
  const int tm = nrb == 4 ? 64 : (nrb == 6 ? 96 : nrb * 32);
  *lds = bwd ? e16_bwd_lds_bytes(tm, D, nrb * 32) : e16_lds_bytes(tm, D, nrb * 32);
  return *lds <= (size_t)kMaxLdsBytes;
}

template <int NRB>
static int launch16(const EdgeTileArgs& a, const dss2_edge_pass_t& k, int grid, bool bwd, hipStream_t s) {
  if (!bwd) return launch_edge_kernel<edge16_fwd_kernel<NRB>>("edge16_fwd", a, k, grid, s);
  if (!a.U) return launch_edge_kernel<edge16_bwd_kernel<NRB, false>>("edge16_bwd", a, k, grid, s);
  assert(NRB <= 2);      // (with U that instantiation misses its register budget: edge_select sends it to the VALU tile kernel)
  if constexpr (NRB <= 2) return launch_edge_kernel<edge16_bwd_kernel<NRB, true>>("edge16_bwd", a, k, grid, s);
  return 1;
}

int launch_edge16(const EdgeTileArgs& a, const dss2_edge_pass_t& k, int grid, bool bwd, hipStream_t s) {
  EdgeTileArgs b = a;
  if (k.parts == 2) { b.xtm = a.TM; b.parts = 2; }      // 128- / 192-row tiles as two parts of 64 / 96 rows (the forward: one workgroup per part)
  return k.nrb == 1 ? launch16<1>(b, k, grid, bwd, s) : k.nrb == 2 ? launch16<2>(b, k, grid, bwd, s) : launch16<3>(b, k, grid, bwd, s);
}

}  // namespace dss2
