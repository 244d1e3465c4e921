// fieldtab.hpp -- what rcmdyn_put / rcmdyn_get know about each rcmdyn_field (include/rcmdyn.h),
// one row per id in enum order.  Host-only.  A new field is added here (its row), in
// rcmdyn_engine::field_ptr (its buffer) and in regcm_amd/config.py (its name and level set);
// put, get and the lazy allocations read the row.
#pragma once
#include <cstddef>

#include "../../include/rcmdyn.h"

namespace fieldtab {

enum Lev { KZ, KZ1, ONE, NSPLIT };       // levels: kz, kz + 1 (full levels), 2-D, nsplit
enum Acc { RW, RO };                     // put and get, or get only
// what the configuration must offer.  put refuses on every unmet need; get tests NQX5 and UW
// and, once the slice exists, HYD_Z, and answers 'unknown field' for a buffer the engine lacks
enum Need {
  ANY,
  NH,        // idynamic = 2
  HYD_PS,    // XPSB_B1: no put on the NH core, which reads no ps record
  HYD_Z,     // zq, za, dzq: mkslice computes them for idynamic = 1 only
  NQX5,      // nqx = 5 (ipptls = 2)
  UW         // ibltyp = 2
};
// buffers that exist from an event on: the first put of a field of the group (PHYSICS, BDYIN,
// TKEPHY), rcmdyn_tend_pre_physics (SLICE); DIAG is readable while rcmdyn_set_diagnostics is on
enum Lazy { NONE, PHYSICS, BDYIN, TKEPHY, SLICE, DIAG };
// what a put leaves to do: refresh the derived statics, the boundary ghost rings, kpbl's ghost
// ring; drop the captured graphs (NH statics are graph constants); DPRD / PR0 do that too and
// arm check_dprd (PR0 only once dprddx / dprddy were put)
enum After { NOTHING, STATICS, BDY, KPBL_RING, GRAPHS, DPRD, PR0 };

struct Row {
  rcmdyn_field id;
  Lev lev;
  Acc acc = RW;
  Need need = ANY;
  Lazy lazy = NONE;
  After after = NOTHING;
};

#define F(name) RCMDYN_##name
constexpr Row TAB[] = {
  // prognostic state
  {F(ATM1_U), KZ}, {F(ATM1_V), KZ}, {F(ATM1_T), KZ}, {F(ATM1_QV), KZ}, {F(ATM1_QC), KZ},
  {F(ATM2_U), KZ}, {F(ATM2_V), KZ}, {F(ATM2_T), KZ}, {F(ATM2_QV), KZ}, {F(ATM2_QC), KZ},
  {F(PSA), ONE}, {F(PSB), ONE}, {F(DSTOR), NSPLIT}, {F(HSTOR), NSPLIT},
  // statics
  {F(MSFX), ONE, RW, ANY, NONE, STATICS}, {F(MSFD), ONE, RW, ANY, NONE, STATICS},
  {F(CORIOL), ONE, RW, ANY, NONE, STATICS}, {F(HT), ONE, RW, ANY, NONE, STATICS},
  // lateral boundary data
  {F(XUB_B0), KZ, RW, ANY, NONE, BDY}, {F(XUB_BT), KZ, RW, ANY, NONE, BDY},
  {F(XVB_B0), KZ, RW, ANY, NONE, BDY}, {F(XVB_BT), KZ, RW, ANY, NONE, BDY},
  {F(XTB_B0), KZ, RW, ANY, NONE, BDY}, {F(XTB_BT), KZ, RW, ANY, NONE, BDY},
  {F(XQB_B0), KZ, RW, ANY, NONE, BDY}, {F(XQB_BT), KZ, RW, ANY, NONE, BDY},
  {F(XPSB_B0), ONE, RW, ANY, NONE, BDY}, {F(XPSB_BT), ONE, RW, ANY, NONE, BDY},
  // diagnostics of the last tend
  {F(PSC), ONE, RO}, {F(PTEN), ONE, RO}, {F(PSDOTA), ONE, RO},
  {F(TTEN), KZ, RO, ANY, DIAG}, {F(UTEN), KZ, RO, ANY, DIAG}, {F(VTEN), KZ, RO, ANY, DIAG},
  {F(QVTEN), KZ, RO, ANY, DIAG}, {F(QCTEN), KZ, RO, ANY, DIAG},
  {F(OMEGA), KZ, RO, ANY, DIAG}, {F(QDOT), KZ1, RO}, {F(XKC), KZ, RO, ANY, DIAG}, {F(PHI), KZ, RO},
  // non-hydrostatic state and its boundary data
  {F(ATM1_PP), KZ, RW, NH}, {F(ATM2_PP), KZ, RW, NH}, {F(ATM1_W), KZ1, RW, NH}, {F(ATM2_W), KZ1, RW, NH},
  {F(XPPB_B0), KZ, RW, NH, NONE, BDY}, {F(XPPB_BT), KZ, RW, NH, NONE, BDY},
  {F(XWWB_B0), KZ1, RW, NH, NONE, BDY}, {F(XWWB_BT), KZ1, RW, NH, NONE, BDY},
  // non-hydrostatic reference state and statics
  {F(ATM0_PS), ONE, RW, NH, NONE, GRAPHS}, {F(ATM0_PR), KZ, RW, NH, NONE, PR0},
  {F(ATM0_T), KZ, RW, NH, NONE, GRAPHS}, {F(ATM0_RHO), KZ, RW, NH, NONE, GRAPHS},
  {F(ATM0_Z), KZ, RW, NH, NONE, GRAPHS}, {F(ATM0_PF), KZ1, RW, NH, NONE, GRAPHS},
  {F(ATM0_RHOF), KZ1, RW, NH, NONE, GRAPHS}, {F(ATM0_ZF), KZ1, RW, NH, NONE, GRAPHS},
  {F(DPSDXM), ONE, RW, NH, NONE, GRAPHS}, {F(DPSDYM), ONE, RW, NH, NONE, GRAPHS},
  {F(DPRDDX), KZ, RW, NH, NONE, DPRD}, {F(DPRDDY), KZ, RW, NH, NONE, DPRD},
  {F(EF), ONE, RW, NH, NONE, GRAPHS}, {F(DDX), ONE, RW, NH, NONE, GRAPHS}, {F(DDY), ONE, RW, NH, NONE, GRAPHS},
  {F(DMDX), ONE, RW, NH, NONE, GRAPHS}, {F(DMDY), ONE, RW, NH, NONE, GRAPHS}, {F(EX), ONE, RW, NH, NONE, GRAPHS},
  {F(CRX), ONE, RW, NH, NONE, GRAPHS}, {F(CRY), ONE, RW, NH, NONE, GRAPHS},
  // physics tendencies
  {F(TPHY), KZ, RW, ANY, PHYSICS}, {F(QVPHY), KZ, RW, ANY, PHYSICS}, {F(QCPHY), KZ, RW, ANY, PHYSICS},
  {F(UPHY), KZ, RW, ANY, PHYSICS}, {F(VPHY), KZ, RW, ANY, PHYSICS},
  {F(PPPHY), KZ, RW, NH, PHYSICS}, {F(WPHY), KZ1, RW, NH, PHYSICS},
  // mkslice export
  {F(ATMS_UBX3D), KZ, RO, ANY, SLICE}, {F(ATMS_VBX3D), KZ, RO, ANY, SLICE}, {F(ATMS_UBD3D), KZ, RO, ANY, SLICE},
  {F(ATMS_VBD3D), KZ, RO, ANY, SLICE}, {F(ATMS_TB3D), KZ, RO, ANY, SLICE}, {F(ATMS_QVB3D), KZ, RO, ANY, SLICE},
  {F(ATMS_QCB3D), KZ, RO, ANY, SLICE}, {F(ATMS_TV3D), KZ, RO, ANY, SLICE}, {F(ATMS_PB3D), KZ, RO, ANY, SLICE},
  {F(ATMS_PF3D), KZ1, RO, ANY, SLICE}, {F(ATMS_PS2D), ONE, RO, ANY, SLICE}, {F(ATMS_RHOX2D), ONE, RO, ANY, SLICE},
  {F(ATMS_TH3D), KZ, RO, ANY, SLICE}, {F(ATMS_RHOB3D), KZ, RO, ANY, SLICE}, {F(ATMS_TP3D), KZ, RO, ANY, SLICE},
  {F(ATMS_WPX3D), KZ, RO, ANY, SLICE}, {F(ATMS_WB3D), KZ1, RO, ANY, SLICE}, {F(ATMS_ZQ), KZ1, RO, HYD_Z, SLICE},
  {F(ATMS_ZA), KZ, RO, HYD_Z, SLICE}, {F(ATMS_DZQ), KZ, RO, HYD_Z, SLICE}, {F(ATMS_QSB3D), KZ, RO, ANY, SLICE},
  {F(ATMS_RHB3D), KZ, RO, ANY, SLICE},
  // the ICBC record of the device bdyin
  {F(XUB_B1), KZ, RW, ANY, BDYIN}, {F(XVB_B1), KZ, RW, ANY, BDYIN}, {F(XTB_B1), KZ, RW, ANY, BDYIN},
  {F(XQB_B1), KZ, RW, ANY, BDYIN}, {F(XPSB_B1), ONE, RW, HYD_PS, BDYIN}, {F(XPPB_B1), KZ, RW, NH, BDYIN},
  {F(XWWB_B1), KZ1, RW, NH, BDYIN}, {F(ATM0_PSDOT), ONE, RW, NH, BDYIN},
  // UW PBL
  {F(ATM1_TKE), KZ1, RW, UW}, {F(ATM2_TKE), KZ1, RW, UW}, {F(TKEPHY), KZ1, RW, UW, TKEPHY},
  {F(KPBL), ONE, RW, UW, NONE, KPBL_RING},
  // nqx = 5: qi, qr, qs
  {F(ATM1_QI), KZ, RW, NQX5}, {F(ATM1_QR), KZ, RW, NQX5}, {F(ATM1_QS), KZ, RW, NQX5},
  {F(ATM2_QI), KZ, RW, NQX5}, {F(ATM2_QR), KZ, RW, NQX5}, {F(ATM2_QS), KZ, RW, NQX5},
  {F(QIPHY), KZ, RW, NQX5, PHYSICS}, {F(QRPHY), KZ, RW, NQX5, PHYSICS}, {F(QSPHY), KZ, RW, NQX5, PHYSICS},
  {F(ATMS_QXB3D_QI), KZ, RO, NQX5, SLICE}, {F(ATMS_QXB3D_QR), KZ, RO, NQX5, SLICE},
  {F(ATMS_QXB3D_QS), KZ, RO, NQX5, SLICE},
};
#undef F

constexpr bool every_id_once_in_order() {
  if (sizeof(TAB) / sizeof(TAB[0]) != RCMDYN_NFIELDS) return false;
  for (int f = 0; f < RCMDYN_NFIELDS; f++)
    if (TAB[f].id != f) return false;
  return true;
}
static_assert(every_id_once_in_order(), "fieldtab: one row per rcmdyn_field, in enum order");

// the row of a field id, null for an id outside the enum
constexpr const Row* row(int f) { return f >= 0 && f < RCMDYN_NFIELDS ? &TAB[f] : nullptr; }
constexpr int levels(Lev l, int kz, int nsplit) { return l == KZ ? kz : l == KZ1 ? kz + 1 : l == ONE ? 1 : nsplit; }

// n consecutive ids from `first` on are the members of one lazily allocated group: the engine
// keeps such a group in one array indexed by id - first
constexpr bool group(rcmdyn_field first, int n, Lazy lazy) {
  for (int q = 0; q < n; q++)
    if (TAB[first + q].lazy != lazy) return false;
  return true;
}
constexpr int count(Lazy lazy) {
  int n = 0;
  for (const Row& r : TAB) n += r.lazy == lazy;
  return n;
}
constexpr int NATMS = 22, NPHY = 7, NBIN = 7;   // Tile::atms, Tile::phy, Tile::bin (then ATM0_PSDOT)
static_assert(group(RCMDYN_ATMS_UBX3D, NATMS, SLICE) && group(RCMDYN_ATMS_QXB3D_QI, 3, SLICE) &&
              count(SLICE) == NATMS + 3 && group(RCMDYN_TPHY, NPHY, PHYSICS) && group(RCMDYN_QIPHY, 3, PHYSICS) &&
              count(PHYSICS) == NPHY + 3 && group(RCMDYN_XUB_B1, NBIN + 1, BDYIN) && count(BDYIN) == NBIN + 1 &&
              count(TKEPHY) == 1,
              "fieldtab: the lazily allocated groups are contiguous runs of the enum");

// the levels k_slice writes (slice.hip), which run_slice allocates from the rows: pf3d, wb3d and
// zq up to kz + 1, ps2d and rhox2d as planes
constexpr bool slice_levels_match() {
  for (int f = RCMDYN_ATMS_UBX3D; f < RCMDYN_ATMS_UBX3D + NATMS; f++) {
    const bool full = f == RCMDYN_ATMS_PF3D || f == RCMDYN_ATMS_WB3D || f == RCMDYN_ATMS_ZQ;
    const bool plane = f == RCMDYN_ATMS_PS2D || f == RCMDYN_ATMS_RHOX2D;
    if (TAB[f].lev != (full ? KZ1 : plane ? ONE : KZ)) return false;
  }
  return true;
}
static_assert(slice_levels_match(), "fieldtab: the ATMS_* rows size the buffers k_slice fills");

}  // namespace fieldtab
