// Layer-chained variant of gemm_prop: host side and the fp32 instantiations (kernel: dss2_gemm_chain_kernel.hpp).  Which kernel a
// chain runs and with which geometry is decided in ONE function, chain_select; the exported queries and the dispatch read its record.
#include "dss2_gemm_chain_kernel.hpp"

namespace dss2 {

// every environment switch of the selection, read once per process
struct ChainSwitches { int rs, rs3, sp, sp_f16, ncg1_tiles; };
static const ChainSwitches& chain_switches() {
  static const ChainSwitches sw = [] {
    auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    // (ncg1_tiles, round 6: ONE column group on 96- / 192-row tiles as single-wave split-plane workgroups pays where there are enough
    //  tiles to fill the chip that way -- measured on the driver's model line, 2.47 -> 2.33 ms per step at 1024 tiles against the
    //  three-waves-per-column-group bf16x6 chain, but 1.55 -> 1.63 at 512 and 1.06 -> 1.15 ms at 64 tiles, where a tile's latency counts)
    return ChainSwitches{env("DSS2_CHAIN_RS", 0), env("DSS2_CHAIN_RS3", 1), env("DSS2_CHAIN_SP", 1), env("DSS2_CHAIN_SP_F16", 1),
                         env("DSS2_CHAIN_SP6_NCG1", 1) ? 768 : -1};
  }();
  return sw;
}

// row split: two waves per column group for narrow layers on two-row-block tiles (DSS2_CHAIN_RS overrides: 1 or 2)
static int chain_row_split(int nrb, int ncg) {
  const int forced = chain_switches().rs;
  if (nrb % 2 != 0 || 2 * ncg > 8) return 1;
  if (forced == 1 || forced == 2) return forced;
  return ncg <= 2 ? 2 : 1;
}

// the fp32 instantiations (the bf16x6 ones: chain16_launcher, dss2_gemm_chain16.hip)
ChainLauncher chain_launcher(int nrb, int nmat, int nw, int rs) {
#define DSS2_CASE(NRB, NMAT, RS) \
  if (nrb == NRB && nmat == NMAT && rs == RS) return nw == 4 ? launch_chain<NRB, NMAT, 4, RS> : nw == 8 ? launch_chain<NRB, NMAT, 8, RS> : nullptr;
  DSS2_CASE(1, 2, 1) DSS2_CASE(1, 3, 1) DSS2_CASE(1, 4, 1) DSS2_CASE(2, 2, 1) DSS2_CASE(2, 3, 1) DSS2_CASE(2, 4, 1)
  DSS2_CASE(3, 2, 1) DSS2_CASE(3, 3, 1) DSS2_CASE(4, 2, 1)
  DSS2_CASE(2, 2, 2) DSS2_CASE(2, 3, 2) DSS2_CASE(2, 4, 2) DSS2_CASE(4, 2, 2)
#undef DSS2_CASE
  return nullptr;
}

// The ONE place a chain launch gets its kernel and geometry, per weight format (dss2_chain_plan_t in include/dss2_hip.h).  ntiles = 0:
// for the capability; nout / edge_width = 0: no head / no edge phase asked.
static dss2_chain_plan_t chain_select(int nrb, int nmat, int kreal, int hout, int ell_width, int ntiles, int nout, int edge_width) {
  dss2_chain_plan_t p = {};
  if (kreal != hout || (hout & 3) != 0 || ell_width <= 0) return p;      // what every chain kernel asks of a shape
  const ChainSwitches& sw = chain_switches();
  const int ncg = (hout + 31) / 32, rs = chain_row_split(nrb, ncg), nw = rs * ncg <= 4 ? 4 : 8;
  auto args = [&](int b_format) {      // the shape as the kernel families read it
    dss2_gemm_prop_args a = {};
    a.b_format = b_format; a.nrb = nrb; a.nmat = nmat; a.kreal = kreal; a.kpad = b_format ? (kreal + 15) / 16 * 16 : (kreal + 7) / 8 * 8;
    a.hout = hout; a.ncg = ncg; a.ell_width = ell_width;
    return a;
  };
  auto kernel = [&](dss2_chain_kernel_t& k, int family, int row_split, int waves, size_t lds) {
    k.family = family; k.row_split = row_split; k.waves = waves; k.block = 64 * ncg * row_split; k.lds_bytes = (int32_t)lds;
  };
  // the multi-wave kernels (dss2_gemm_chain_kernel.hpp): fp32, and bf16x6 where the instantiation exists (96-row tiles at K = 2: three
  // waves per column group, DSS2_CHAIN_RS3=0: one)
  const size_t lds0 = chain_lds_bytes(nrb, args(0).kpad, ncg, ell_width);
  const bool fp32 = hout <= 256 && ell_width <= 32 && chain_launcher(nrb, nmat, nw, rs) && lds0 <= (size_t)kMaxLdsBytes;
  const bool rs3 = sw.rs3 && nrb == 3 && nmat == 3 && ncg <= 4;
  const int rs16 = rs3 ? 3 : rs, nw16 = rs3 ? 12 : nw;
  const size_t lds16 = chain_lds_bytes(nrb, args(1).kpad, ncg, ell_width, chain_rm(nrb, rs, true, nmat) ? nmat : 0);
  const bool multi16 = fp32 && chain16_launcher(nrb, nmat, nw16, rs16) && lds16 <= (size_t)kMaxLdsBytes;
  // the split-plane kernels of a 16-bit format: 64-row tiles with one wave per column group, 96- / 192-row tiles from the policy's tile
  // count on where they have ONE column group
  size_t lds_sp[3] = {};
  auto split_plane = [&](int f) {
    const dss2_gemm_prop_args a = args(f);
    if (!sw.sp || (f == 2 && !sw.sp_f16)) return (int)DSS2_CHAIN_NONE;
    if (rs == 1 && chain_sp_shape(a, &lds_sp[f])) return (int)DSS2_CHAIN_SP;
    const bool too_few = ncg == 1 && (sw.ncg1_tiles < 0 || (ntiles > 0 && ntiles < sw.ncg1_tiles));
    return !too_few && chain_sp6_shape(a, &lds_sp[f]) ? (int)DSS2_CHAIN_SP6 : (int)DSS2_CHAIN_NONE;
  };
  const int sp1 = split_plane(1), sp2 = split_plane(2);
  const int words = ncg * 32 * ((4 * nrb + 7) / 8);      // per wave (column group): 64 lanes x ceil(row pieces / 8) 32-bit words (dss2_gemm_chain_sp6.hip, _sp.hip)
  const bool b16 = nrb == 6 ? sp1 == DSS2_CHAIN_SP6 : multi16;      // (192-row tiles: only the split-plane form exists)
  const bool f16 = sp2 == DSS2_CHAIN_SP6 || (sp2 == DSS2_CHAIN_SP && (hout & 31) == 0 && b16);

  if (fp32) kernel(p.fmt[0], DSS2_CHAIN_FP32, rs, nw, lds0);
  if (b16 && sp1) kernel(p.fmt[1], sp1, 1, sp1 == DSS2_CHAIN_SP ? nw : ncg, lds_sp[1]);
  else if (b16) kernel(p.fmt[1], DSS2_CHAIN_BF16X6, rs16, nw16, lds16);
  if (f16 && (fp32 || b16)) kernel(p.fmt[2], sp2, 1, sp2 == DSS2_CHAIN_SP ? nw : ncg, lds_sp[2]);
  p.fmt[1].gate_words = sp1 ? words : 0;
  p.fmt[2].gate_words = f16 ? words : 0;
  // the fused head rides on the split-plane kernels: forward (bit 0) and backward (bit 1) on 64-row tiles, the backward head only on
  // 96- / 192-row tiles; its weight gradient from the backward head's staging up to nout = 2
  const int head = nout < 1 || nout > 4 ? 0 : p.fmt[1].family == DSS2_CHAIN_SP ? 3 : p.fmt[1].family == DSS2_CHAIN_SP6 ? 2 : 0;
  for (int f = 1; f <= 2; ++f) {
    p.fmt[f].head_modes = p.fmt[f].family ? head : 0;
    p.fmt[f].head_wgrad = nout <= 2 && (p.fmt[f].head_modes & 2) ? 1 : 0;
  }
  if (f16 && sp2 == DSS2_CHAIN_SP && edge_width > 0 && edge_width <= 32) p.fmt[2].edge_modes = chain_sp_edge_modes(args(2), edge_width);
  return p;
}

}  // namespace dss2

extern "C" int dss2_chain_sp6_single_group_min_tiles(void) { return dss2::chain_switches().ncg1_tiles; }

extern "C" int dss2_gemm_prop_chain_plan(int nrb, int nmat, int hid, int ell_width, int ntiles, int nout, int edge_width, dss2_chain_plan_t* out) {
  if (!out) { dss2::set_error("dss2_gemm_prop_chain_plan: null argument"); return 2; }
  *out = dss2::chain_select(nrb, nmat, hid, hid, ell_width, ntiles, nout, edge_width);
  return 0;
}

// The older queries: readers of the record, for the capability (no tile count).
#define DSS2_CHAIN_QUERY(...) dss2::chain_select(nrb, nmat, kreal, hout, ell_width, 0, __VA_ARGS__)
extern "C" int dss2_gemm_prop_chain_supported(int nrb, int nmat, int kreal, int hout, int ell_width) { return DSS2_CHAIN_QUERY(0, 0).fmt[0].family != 0; }
extern "C" int dss2_gemm_prop_chain16_supported(int nrb, int nmat, int kreal, int hout, int ell_width) { return DSS2_CHAIN_QUERY(0, 0).fmt[1].family != 0; }
extern "C" int dss2_gemm_prop_chain_f16_supported(int nrb, int nmat, int kreal, int hout, int ell_width) { return DSS2_CHAIN_QUERY(0, 0).fmt[2].gate_words > 0; }
extern "C" int dss2_gemm_prop_chain_gate_words(int nrb, int nmat, int kreal, int hout, int ell_width) { return DSS2_CHAIN_QUERY(0, 0).fmt[1].gate_words; }
extern "C" int dss2_gemm_prop_chain_head_supported(int nrb, int nmat, int kreal, int hout, int ell_width, int nout) { return DSS2_CHAIN_QUERY(nout, 0).fmt[1].head_modes; }
extern "C" int dss2_gemm_prop_chain_head_wgrad_supported(int nrb, int nmat, int kreal, int hout, int ell_width, int nout) { return DSS2_CHAIN_QUERY(nout, 0).fmt[1].head_wgrad; }
extern "C" int dss2_gemm_prop_chain_edge_supported(int nrb, int nmat, int kreal, int hout, int ell_width, int edge_width) { return DSS2_CHAIN_QUERY(0, edge_width).fmt[2].edge_modes; }
#undef DSS2_CHAIN_QUERY

// the record of a launch: its real tile count, and the head and edge phase it carries
static dss2_chain_plan_t chain_plan_of(const dss2_gemm_prop_args& a, const dss2_chain_head* head) {
  return dss2::chain_select(a.nrb, a.nmat, a.kreal, a.hout, a.ell_width, a.ntiles > 0 ? a.ntiles : 0, head ? head->nout : 0, head && head->edge.W1 ? head->edge.width : 0);
}
static int chain_impl(const dss2_gemm_prop_args* ap, const dss2_chain_layer* layers, int n_layers, const dss2_chain_head* head, const dss2_chain_plan_t& p, void* stream);

static int dss2_gemm_prop_chain_launch(const dss2_gemm_prop_args* ap, const dss2_chain_layer* layers, int n_layers, void* stream) {
  return chain_impl(ap, layers, n_layers, nullptr, chain_plan_of(*ap, nullptr), stream);
}
extern "C" int dss2_gemm_prop_chain(const dss2_gemm_prop_args* ap, const dss2_chain_layer* layers, int n_layers, void* stream) {
  return dss2::entry(dss2_gemm_prop_chain_launch, stream, dss2::copied(ap, "dss2_gemm_prop_chain"), dss2::kept(layers, n_layers), n_layers);
}

static int dss2_gemm_prop_chain_head_launch(const dss2_gemm_prop_args* ap, const dss2_chain_layer* layers, int n_layers, const dss2_chain_head* head, void* stream) {
  using namespace dss2;
  if (!head || (head->mode != 1 && head->mode != 2)) { set_error("gemm_prop_chain_head: head.mode must be 1 or 2"); return 2; }
  const dss2_chain_plan_t p = chain_plan_of(*ap, head);
  const dss2_chain_kernel_t none = {}, &k = ap->b_format == 1 || ap->b_format == 2 ? p.fmt[ap->b_format] : none;
  if (!(k.head_modes & head->mode)) {
    set_error("gemm_prop_chain_head: unsupported shape (nrb=%d nmat=%d hid=%d nout=%d b_format=%d)", ap->nrb, ap->nmat, ap->hout, head->nout, ap->b_format);
    return 2;
  }
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  for (int m = 0; m < ap->nmat; ++m)
    if (!head->W[m] || !al16(head->W[m])) { set_error("gemm_prop_chain_head: W[%d] missing or misaligned", m); return 2; }
  if (head->mode == 1 && !head->Y) { set_error("gemm_prop_chain_head: forward head needs Y"); return 2; }
  if (head->mode == 2 && (!head->G || !head->Xout || !al16(head->Xout) || !al16(head->gate) || (head->ldxo & 3) || (head->ld_gate & 3))) {
    set_error("gemm_prop_chain_head: backward head needs G, a 16-byte aligned Xout (and gate)"); return 2;
  }
  if (head->drop_id && !ap->drop_state) { set_error("gemm_prop_chain_head: drop_id without drop_state"); return 2; }
  if (head->wg_slab && (head->mode != 2 || !head->gate || !k.head_wgrad)) {
    set_error("gemm_prop_chain_head: wg_slab needs mode 2, gate and a shape dss2_gemm_prop_chain_head_wgrad_supported accepts"); return 2;
  }
  const dss2_chain_edge& e = head->edge;
  if (e.W1) {
    if (!(k.edge_modes & head->mode)) {
      set_error("gemm_prop_chain_head: no edge phase for this shape (nrb=%d nmat=%d hid=%d ell=%d edge ell=%d b_format=%d mode=%d)",
                ap->nrb, ap->nmat, ap->hout, ap->ell_width, e.width, ap->b_format, head->mode);
      return 2;
    }
    if (!e.x || !e.ea || !e.b1 || !e.ell_ent || (head->mode == 1 && (!e.S || !al16(e.S))) || (head->mode == 2 && !e.slab)) {
      set_error("gemm_prop_chain_head: the edge phase needs x, edge_attr, W1, b1, ell_ent and S (mode 1, 16-byte aligned) / slab (mode 2)"); return 2;
    }
  }
  return chain_impl(ap, layers, n_layers, head, p, stream);
}
extern "C" int dss2_gemm_prop_chain_head(const dss2_gemm_prop_args* ap, const dss2_chain_layer* layers, int n_layers, const dss2_chain_head* head, void* stream) {
  if (ap && !head) { dss2::set_error("dss2_gemm_prop_chain_head: head is NULL"); return 2; }      // (a null ap: entry()'s "null argument" comes first)
  return dss2::entry(dss2_gemm_prop_chain_head_launch, stream, dss2::copied(ap, "dss2_gemm_prop_chain_head"), dss2::kept(layers, n_layers), n_layers, dss2::copied(head));
}

static int chain_impl(const dss2_gemm_prop_args* ap, const dss2_chain_layer* layers, int n_layers, const dss2_chain_head* head, const dss2_chain_plan_t& p, void* stream) {
  using namespace dss2;
  const dss2_gemm_prop_args& a = *ap;
  if (n_layers < 1 || n_layers > CHAIN_MAX || !layers) { set_error("gemm_prop_chain: 1..%d layers, got %d", CHAIN_MAX, n_layers); return 2; }
  if (a.ntiles <= 0) return 0;
  if (a.b_format < 0 || a.b_format > 2) { set_error("gemm_prop_chain: unknown b_format %d", a.b_format); return 2; }
  const dss2_chain_kernel_t& k = p.fmt[a.b_format];
  const bool any = p.fmt[0].family || (a.b_format && a.nrb == 6 && p.fmt[1].family);      // (192-row tiles: the 16-bit split-plane forms only)
  if (!any || !a.ell_tiles || a.prop_in || a.narrow_h || a.rowscale || a.kpad != (a.b_format >= 1 ? (a.kreal + 15) / 16 * 16 : (a.kreal + 7) / 8 * 8) ||
      a.ncg != (a.hout + 31) / 32) {
    set_error("gemm_prop_chain: unsupported shape (nrb=%d nmat=%d k=%d hout=%d ell=%d); use dss2_gemm_prop per layer",
              a.nrb, a.nmat, a.kreal, a.hout, a.ell_width);
    return 2;
  }
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (((!a.X || !al16(a.X)) && !(head && head->mode == 2)) || (a.ldx & 3) || (a.ldy & 3) || (a.ld_relu & 3) || (a.ld_dmask & 3) || (a.ld_add & 3)) {
    set_error("gemm_prop_chain: operands must be 16-byte aligned with leading dimensions divisible by 4"); return 2;
  }
  ChainTable ct = {};
  ct.n = n_layers;
  bool any_pre = false;
  for (int i = 0; i < n_layers; ++i) {
    const dss2_chain_layer& L = layers[i];
    if (!L.Bp || !L.Y || !al16(L.Y) || !al16(L.bias) || !al16(L.relu_src) || !al16(L.dmask) || !al16(L.add_src) || !al16(L.prebias)) {
      set_error("gemm_prop_chain: layer %d has a missing or misaligned operand", i); return 2;
    }
    any_pre = any_pre || L.prebias;
    if (L.drop_id && !a.drop_state) { set_error("gemm_prop_chain: layer %d asks for in-kernel dropout without drop_state", i); return 2; }
    ct.l[i] = L;
  }
  if (any_pre && !a.pre_rowscale) { set_error("gemm_prop_chain: prebias needs pre_rowscale"); return 2; }
  hipStream_t s = as_stream(stream);
  switch (k.family) {
    case DSS2_CHAIN_SP: return launch_chain_sp(a, ct, head, k, s);
    case DSS2_CHAIN_SP6: return launch_chain_sp6(a, ct, head, k, s);
    case DSS2_CHAIN_BF16X6: return chain16_launcher(a.nrb, a.nmat, k.waves, k.row_split)(a, ct, k, s);      // (non-null, and no head: chain_select asked)
    case DSS2_CHAIN_FP32: return chain_launcher(a.nrb, a.nmat, k.waves, k.row_split)(a, ct, k, s);
  }
  if (a.b_format == 2) set_error("gemm_prop_chain(f16x3): unsupported shape (nrb=%d nmat=%d k=%d hout=%d)", a.nrb, a.nmat, a.kreal, a.hout);
  else set_error("gemm_prop_chain(bf16x6): unsupported shape (nrb=%d nmat=%d k=%d kpad=%d hout=%d)", a.nrb, a.nmat, a.kreal, a.kpad, a.hout);
  return 2;
}
