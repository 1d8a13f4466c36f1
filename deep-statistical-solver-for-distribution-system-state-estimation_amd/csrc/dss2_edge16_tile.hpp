#pragma once
// The bf16x6 edge MLP's tile pieces (planes, weight fragments, the pre-activation Z_k, the backward's transposed images), shared by
// the edge kernels of dss2_edge16.hip and the edge phases of the 64-row split-plane chain (dss2_gemm_chain_sp.hip): one definition of
// the arithmetic, so that S and the recomputed gates are bit for bit the same in both.
#include "dss2_edge_tile.hpp"

namespace dss2 {

constexpr float E16_KILL = -1e30f;

// 8 consecutive k of one operand row -> the three bf16 planes (16 bytes each)
__device__ __forceinline__ void e16_split8(const f32x4 v0, const f32x4 v1, uint4& h, uint4& m, uint4& l) {
  split3_pair(v0[0], v0[1], h.x, m.x, l.x);
  split3_pair(v0[2], v0[3], h.y, m.y, l.y);
  split3_pair(v1[0], v1[1], h.z, m.z, l.z);
  split3_pair(v1[2], v1[3], h.w, m.w, l.w);
}
__device__ __forceinline__ bf16x8 e16_frag(const uint4 v) { return __builtin_bit_cast(bf16x8, v); }

struct E16Lds {
  EdgeStage s;
  const float* xi;      // the x rows of this part's own rows (s.xs + r0 * FN)
  char* PI;      // [3 planes][TM][16 B]: x_i
  char* PK;      // [D][3 planes][2 halves][TM][16 B]: half 0 = x_j, half 1 = edge_attr (6) | valid | empty
};

template <int NRB>
__device__ __forceinline__ E16Lds e16_ptrs(float* esm, int D, int XT) {
  constexpr int TM = NRB * 32;
  E16Lds L;
  L.s.xs = esm;
  L.xi = esm;
  L.s.eaL = L.s.xs + XT * FN;
  L.s.other = reinterpret_cast<int*>(L.s.eaL + D * TM * 8);
  L.PI = reinterpret_cast<char*>(L.s.other + D * TM);
  L.PK = L.PI + 3 * TM * 16;
  L.s.Ak = nullptr; L.s.st = nullptr;
  return L;
}

inline size_t e16_lds_bytes(int TM, int D, int XT) {      // forward: all slots' planes at once (XT: rows of the whole tile, whose x rows are staged)
  return ((size_t)XT * FN + (size_t)D * TM * 8) * 4 + (size_t)D * TM * 4 + 3 * (size_t)TM * 16 + (size_t)D * 6 * TM * 16;
}

// all slots' planes in one phase: unit = (image, row) of 8 elements; images: x_i, then (slot k, half) for k < D
template <int NRB>
__device__ __forceinline__ void e16_build(const E16Lds& L, int D, int tid, int nthreads) {
  constexpr int TM = NRB * 32;
  const EdgeStage& s = L.s;
  for (int u = tid; u < TM * (1 + 2 * D); u += nthreads) {
    const int img = u / TM, row = u - img * TM;
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    char* dst;
    int pstride;
    if (img == 0) {
      v0 = *reinterpret_cast<const f32x4*>(L.xi + row * FN);
      v1 = *reinterpret_cast<const f32x4*>(L.xi + row * FN + 4);
      dst = L.PI + row * 16;
      pstride = TM * 16;
    } else {
      const int k = (img - 1) >> 1, hh = (img - 1) & 1;
      const int o = s.other[k * TM + row];
      if (hh == 0) {
        if (o >= 0) { v0 = *reinterpret_cast<const f32x4*>(s.xs + o * FN); v1 = *reinterpret_cast<const f32x4*>(s.xs + o * FN + 4); }
      } else if (o >= 0) {
        v0 = *reinterpret_cast<const f32x4*>(s.eaL + (k * TM + row) * 8);
        const f32x4 t = *reinterpret_cast<const f32x4*>(s.eaL + (k * TM + row) * 8 + 4);
        v1 = f32x4{t[0], t[1], 1.f, 0.f};
      } else {
        v1 = f32x4{0.f, 0.f, 0.f, 1.f};
      }
      dst = L.PK + ((size_t)(k * 3) * 2 + hh) * TM * 16 + row * 16;
      pstride = 2 * TM * 16;
    }
    uint4 h, m, l;
    e16_split8(v0, v1, h, m, l);
    *reinterpret_cast<uint4*>(dst) = h;
    *reinterpret_cast<uint4*>(dst + pstride) = m;
    *reinterpret_cast<uint4*>(dst + 2 * pstride) = l;
  }
}

// the wave's weight fragments: lane (c32 = hidden column of the wave's group, half) holds k = 8 half .. 8 half + 7
struct E16W { bf16x8 ah, am, al, bh, bm, bl; };      // a*: W1a (x_i columns), b*: W1bc (x_j | edge_attr | b1 | kill)
__device__ __forceinline__ E16W e16_weights(const float* __restrict__ W1, const float* __restrict__ b1, int j, int half) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0, b1v;
  const float* w = W1 + (size_t)j * FC;
  if (half == 0) {
    a0 = f32x4{w[0], w[1], w[2], w[3]}; a1 = f32x4{w[4], w[5], w[6], w[7]};
    b0 = f32x4{w[8], w[9], w[10], w[11]}; b1v = f32x4{w[12], w[13], w[14], w[15]};
  } else {
    b0 = f32x4{w[16], w[17], w[18], w[19]}; b1v = f32x4{w[20], w[21], b1[j], E16_KILL};
  }
  uint4 h, m, l;
  E16W r;
  e16_split8(a0, a1, h, m, l);
  r.ah = e16_frag(h); r.am = e16_frag(m); r.al = e16_frag(l);
  e16_split8(b0, b1v, h, m, l);
  r.bh = e16_frag(h); r.bm = e16_frag(m); r.bl = e16_frag(l);
  return r;
}

// six MFMAs, smallest terms first (the order of the other bf16x6 kernels)
__device__ __forceinline__ f32x16 e16_mma6(const bf16x8 ah, const bf16x8 am, const bf16x8 al, const bf16x8 bh, const bf16x8 bm,
                                           const bf16x8 bl, f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
  return c;
}

// C_i of row block rb: x_i W1a^T (the k = 8 .. 15 half of the step is zero on both sides)
template <int NRB>
__device__ __forceinline__ f32x16 e16_xterm(const E16Lds& L, const E16W& w, int rb, int c32, int half) {
  constexpr int TM = NRB * 32;
  const uint4 z = {0u, 0u, 0u, 0u};
  const char* pi = L.PI + (rb * 32 + c32) * 16;
  const uint4 h = half ? z : *reinterpret_cast<const uint4*>(pi);
  const uint4 m = half ? z : *reinterpret_cast<const uint4*>(pi + TM * 16);
  const uint4 l = half ? z : *reinterpret_cast<const uint4*>(pi + 2 * TM * 16);
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
  return e16_mma6(e16_frag(h), e16_frag(m), e16_frag(l), w.ah, w.am, w.al, c);
}

// pre-activation of slot k, row block rb (bias included; hugely negative on empty slots): THE definition, forward and backward
template <int NRB>
__device__ __forceinline__ f32x16 e16_z(const E16Lds& L, const E16W& w, int k, int rb, int c32, int half, const f32x16 ci) {
  constexpr int TM = NRB * 32;
  const char* pk = L.PK + ((size_t)(k * 3) * 2 + half) * TM * 16 + (rb * 32 + c32) * 16;
  const uint4 h = *reinterpret_cast<const uint4*>(pk);
  const uint4 m = *reinterpret_cast<const uint4*>(pk + 2 * TM * 16);
  const uint4 l = *reinterpret_cast<const uint4*>(pk + 4 * TM * 16);
  return e16_mma6(e16_frag(h), e16_frag(m), e16_frag(l), w.bh, w.bm, w.bl, ci);
}

constexpr int E16_ATN = 16;                                   // per-slot transposed columns: x_j (8) | edge_attr (6) | 1 | 0
__host__ __device__ constexpr int e16_cs(int TM) { return TM * 2 + 16; }      // bytes per transposed column and plane (+16: the b128 reads of 32 columns spread over the banks)
__device__ __forceinline__ int e16_qpos(int row) {            // position of a row inside its transposed row block: bits 2 and 3 swapped
  return (row & ~12) | ((row & 4) << 1) | ((row & 8) >> 1);
}

struct E16Bwd {
  EdgeStage s;      // xs, eaL, other (Ak / st unused)
  const float* xi;  // the x rows of this part's own rows
  char* PI;         // [3 planes][TM][16 B]: x_i, the recomputation's row operand
  char* PK;         // [3 planes][2 halves][TM][16 B]: ONE slot
  char* ATI;        // [3 planes][8 columns][CS]: x_i transposed
  char* ATK;        // [3 planes][16 columns][CS]: the slot's x_j | edge_attr | 1 | 0 transposed
};

template <int NRB>
__device__ __forceinline__ E16Bwd e16_bwd_ptrs(float* esm, int D, int XT) {
  constexpr int TM = NRB * 32, CS = e16_cs(TM);
  E16Bwd L;
  L.s.xs = esm;
  L.xi = esm;
  L.s.eaL = L.s.xs + XT * FN;
  L.s.other = reinterpret_cast<int*>(L.s.eaL + D * TM * 8);
  L.s.Ak = nullptr; L.s.st = nullptr;
  L.PI = reinterpret_cast<char*>(L.s.other + D * TM);
  L.PK = L.PI + 3 * TM * 16;
  L.ATI = L.PK + 6 * TM * 16;
  L.ATK = L.ATI + 3 * FN * CS;
  return L;
}

inline size_t e16_bwd_lds_bytes(int TM, int D, int XT) {
  return ((size_t)XT * FN + (size_t)D * TM * 8) * 4 + (size_t)D * TM * 4 + 3 * (size_t)TM * 16 + 6 * (size_t)TM * 16 +
         3 * (size_t)(FN + E16_ATN) * e16_cs(TM);
}

// rows (2 rp, 2 rp + 1) x four columns c0 .. c0 + 3 of a transposed image with NC columns
template <int NRB>
__device__ __forceinline__ void e16_store_t(char* img, int NC, int c0, int rp, const f32x4 v0, const f32x4 v1) {
  constexpr int CS = e16_cs(NRB * 32);
  const int row = 2 * rp;
  char* dst = img + c0 * CS + (row >> 5) * 64 + 2 * e16_qpos(row & 31);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t h, m, l;
    split3_pair(v0[q], v1[q], h, m, l);
    *reinterpret_cast<uint32_t*>(dst + q * CS) = h;
    *reinterpret_cast<uint32_t*>(dst + (NC + q) * CS) = m;
    *reinterpret_cast<uint32_t*>(dst + (2 * NC + q) * CS) = l;
  }
}

// once per tile: x_i as the recomputation's row planes and as transposed columns
template <int NRB>
__device__ __forceinline__ void e16_bwd_build_tile(const E16Bwd& L, int tid, int nthreads) {
  constexpr int TM = NRB * 32;
  for (int row = tid; row < TM; row += nthreads) {
    uint4 h, m, l;
    e16_split8(*reinterpret_cast<const f32x4*>(L.xi + row * FN), *reinterpret_cast<const f32x4*>(L.xi + row * FN + 4), h, m, l);
    char* dst = L.PI + row * 16;
    *reinterpret_cast<uint4*>(dst) = h;
    *reinterpret_cast<uint4*>(dst + TM * 16) = m;
    *reinterpret_cast<uint4*>(dst + 2 * TM * 16) = l;
  }
  for (int u = tid; u < (TM / 2) * 2; u += nthreads) {
    const int rp = u >> 1, q4 = u & 1;
    const float* src = L.xi + (2 * rp) * FN + 4 * q4;
    e16_store_t<NRB>(L.ATI, FN, 4 * q4, rp, *reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + FN));
  }
}

// per slot: the recomputation's planes (exactly the forward's values: same inputs, same split) and the transposed columns
template <int NRB>
__device__ __forceinline__ void e16_bwd_build_slot(const E16Bwd& L, int k, int tid, int nthreads) {
  constexpr int TM = NRB * 32;
  const EdgeStage& s = L.s;
  for (int u = tid; u < 2 * TM; u += nthreads) {
    const int hh = u / TM, row = u - hh * TM;
    const int o = s.other[k * TM + row];
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if (hh == 0) {
      if (o >= 0) { v0 = *reinterpret_cast<const f32x4*>(s.xs + o * FN); v1 = *reinterpret_cast<const f32x4*>(s.xs + o * FN + 4); }
    } else if (o >= 0) {
      v0 = *reinterpret_cast<const f32x4*>(s.eaL + (k * TM + row) * 8);
      const f32x4 t = *reinterpret_cast<const f32x4*>(s.eaL + (k * TM + row) * 8 + 4);
      v1 = f32x4{t[0], t[1], 1.f, 0.f};
    } else {
      v1 = f32x4{0.f, 0.f, 0.f, 1.f};
    }
    uint4 h, m, l;
    e16_split8(v0, v1, h, m, l);
    char* dst = L.PK + (size_t)hh * TM * 16 + row * 16;
    *reinterpret_cast<uint4*>(dst) = h;
    *reinterpret_cast<uint4*>(dst + 2 * TM * 16) = m;
    *reinterpret_cast<uint4*>(dst + 4 * TM * 16) = l;
  }
  for (int u = tid; u < (TM / 2) * 4; u += nthreads) {
    const int rp = u >> 2, q4 = u & 3;
    f32x4 v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int row = 2 * rp + e;
      const int o = s.other[k * TM + row];
      v[e] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (o >= 0) {
        if (q4 < 2) v[e] = *reinterpret_cast<const f32x4*>(s.xs + o * FN + 4 * q4);
        else if (q4 == 2) v[e] = *reinterpret_cast<const f32x4*>(s.eaL + (k * TM + row) * 8);
        else { const f32x4 t = *reinterpret_cast<const f32x4*>(s.eaL + (k * TM + row) * 8 + 4); v[e] = f32x4{t[0], t[1], 1.f, 0.f}; }
      }
    }
    e16_store_t<NRB>(L.ATK, E16_ATN, 4 * q4, rp, v[0], v[1]);
  }
}

// S of row block rb: the sum over the tile's slots of relu_nan(Z_k), slots in order -- THE forward (edge16_fwd_kernel, and the
// forward chain's edge phase in dss2_gemm_chain_sp.hip)
template <int NRB>
__device__ __forceinline__ f32x16 e16_fwd_rb(const E16Lds& L, const E16W& w, int D, int rb, int c32, int half) {
  const f32x16 ci = e16_xterm<NRB>(L, w, rb, c32, half);
  f32x16 Sacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) Sacc[r] = 0.f;
  for (int k = 0; k < D; ++k) {
    const f32x16 c = e16_z<NRB>(L, w, k, rb, c32, half, ci);
#pragma unroll
    for (int r = 0; r < 16; ++r) Sacc[r] += relu_nan(c[r]);
  }
  return Sacc;
}

// the gates of the recomputed pre-activation c as masks over the two bf16 halves of the plane words of registers (2 j, 2 j + 1)
__device__ __forceinline__ void e16_gate_masks(const f32x16 c, uint32_t (&mk)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) mk[j] = (relu_open(c[2 * j]) ? 0x0000ffffu : 0u) | (relu_open(c[2 * j + 1]) ? 0xffff0000u : 0u);
}

// one k-step of dW += dZ_k^T A_k: A operand (ah, am, al) = the dZ planes of registers 8 st .. 8 st + 7 of row block rb, B operand = this
// lane's transposed column (bcol, plane stride bps; none beyond the 24 + 1 columns)
template <int NRB>
__device__ __forceinline__ void e16_dw_step(const uint4 ah, const uint4 am, const uint4 al, const char* bcol, int bps, bool bcol_ok, int rb, int st,
                                            int half, f32x16& dWacc) {
  const char* bp = bcol + rb * 64 + 32 * st + 16 * half;
  const uint4 z4 = {0u, 0u, 0u, 0u};
  const uint4 bh = bcol_ok ? *reinterpret_cast<const uint4*>(bp) : z4;
  const uint4 bm = bcol_ok ? *reinterpret_cast<const uint4*>(bp + bps) : z4;
  const uint4 bl = bcol_ok ? *reinterpret_cast<const uint4*>(bp + 2 * bps) : z4;
  dWacc = e16_mma6(e16_frag(ah), e16_frag(am), e16_frag(al), e16_frag(bh), e16_frag(bm), e16_frag(bl), dWacc);
}

// the dW1 | db1 slab of one workgroup: [h][FC] then [h]
__device__ __forceinline__ void e16_store_slab(float* out, int h, int cg, int c32, int half, const f32x16 dWacc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = cg * 32 + acc_row(r, half);
    if (c32 < FC) out[(size_t)o * FC + c32] = dWacc[r];
    else if (c32 == FC) out[(size_t)h * FC + o] = dWacc[r];
  }
}

}  // namespace dss2
