// bf16x6 instantiations of the layer-chain kernel (dss2_gemm_chain_kernel.hpp, B16 = true).
//
// A translation unit of its own because it is compiled WITHOUT packed fp32 VALU ops (build.sh: -packed-fp32-ops for this
// file, dss2_wgrad16.hip and dss2_stack.hip; the build disassembles them and fails if one v_pk_*_f32 is left).
// Root cause (round 3, profiles/r03_pk_fma_investigation.txt, tools/micro/pkfma_beside_mfma.hip): on MI355X a v_pk_fma_f32
// / v_pk_add_f32 / v_pk_mul_f32 of one wave occasionally returns wrong values in lanes 48..63 -- the last 16-lane pass of the
// op -- while ANOTHER wave of the same SIMD streams v_mfma_f32_32x32x16_bf16, with two or more workgroups per CU.  An 87-line
// kernel without LDS whose failing wave executes no MFMA at all reproduces it (fp32 MFMAs or plain VALU work beside it: never;
// one workgroup per CU: never), so it is neither an LDS race of this kernel nor a missed MFMA -> VALU hazard of the compiler.
// Round 2 met it as run-to-run different values of the epilogue's `v += prebias[m] * rowscale[row][m]`; with today's paired
// operand split (split3_pair -> v_pk_add_f32) a packed build returns garbage in every lane (tools/pk_stress.py).  Plain VALU
// ops are also the cheaper fillers beside MFMAs (MI355X_MICROARCH.md).
#include "dss2_gemm_chain_kernel.hpp"

namespace dss2 {

ChainLauncher chain16_launcher(int nrb, int nmat, int nw, int rs) {
#define DSS2_CASE16(NRB, NMAT, RS)                                                        \
  if (nrb == NRB && nmat == NMAT && rs == RS) return nw == 4 ? launch_chain<NRB, NMAT, 4, RS, true> : nw == 8 ? launch_chain<NRB, NMAT, 8, RS, true> : nullptr;
  DSS2_CASE16(1, 2, 1) DSS2_CASE16(1, 3, 1) DSS2_CASE16(1, 4, 1) DSS2_CASE16(2, 2, 1) DSS2_CASE16(2, 3, 1)      // (2, 4, 1) would spill
  DSS2_CASE16(3, 2, 1) DSS2_CASE16(4, 2, 1)
  DSS2_CASE16(2, 2, 2) DSS2_CASE16(2, 3, 2) DSS2_CASE16(2, 4, 2) DSS2_CASE16(4, 2, 2)
#undef DSS2_CASE16
  // 96-row tiles: three waves per column group (one row block each, twelve waves = three per SIMD) instead of one wave per SIMD
  // with three row blocks -- the VALU-issue-bound phases of a wave run beside the other waves' MFMAs (DSS2_CHAIN_RS3=0: four waves)
  if (nrb == 3 && nmat == 3 && rs == 3 && nw == 12) return launch_chain<3, 3, 12, 3, true>;
  if (nrb == 3 && nmat == 3 && rs == 1 && nw == 4) return launch_chain<3, 3, 4, 1, true>;   // (8 waves would spill)
  return nullptr;
}

}  // namespace dss2

#ifdef DSS2_CHAIN_STAMPS
extern "C" int dss2_debug_read_cstamps(unsigned long long* host_out, int n) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(dss2::g_cstamps), sizeof(unsigned long long) * n);
}
#endif
