// kernels_nh.hpp -- device kernels of the non-hydrostatic step (kernels_nh.hip) and the
// argument block they share.
#pragma once
#include "engine.hpp"

namespace rcm {

// Every buffer of the non-hydrostatic step of one tile.  The NH core updates its state in
// place (no ping-pong), one kernel per reference loop nest or per column recurrence, with
// the intermediates the reference keeps in module arrays held in HBM.  Passed by value.
struct NHFields {
  // state (coupled with p*, as the reference stores it)
  double *a1u, *a1v, *a1t, *a1qv, *a1qc, *a2u, *a2v, *a2t, *a2qv, *a2qc;
  double *a1pp, *a2pp, *a1w, *a2w, *psa, *psb;
  // statics
  const double *msfx, *msfd, *coriol, *ht, *xmsf, *dmsf, *hgfact;
  const int8_t *rgcr, *rgdt;
  const int16_t *ibcr, *ibdt;
  const double *ps0, *pr0, *t0, *rho0, *z0, *pf0, *rhof0, *zf0, *dpsdxm, *dpsdym, *dprddx, *dprddy;
  const double *ef, *ddx, *ddy, *dmdx, *dmdy, *ex, *crx, *cry;
  // boundary data
  const double *ub0, *ubt, *vb0, *vbt, *tb0, *tbt, *qb0, *qbt, *ppb0, *ppbt, *wwb0, *wwbt;
  // 2-D reciprocals (k_surface_pressures)
  const double *rpsa, *rpsb, *rpsda, *rpsdb, *psdota, *psdotb;
  // decoupled / derived fields of the step
  double *pr1, *rho1;
  // unread and null (k_nh_tend_c forms atmx%pr itself): the slot stays because an 8-byte shift
  // of the members after it regroups k_nh_tend_c's kernel-argument loads and changes its
  // schedule (5 771 -> 5 996 instructions); remove it with the next change to that kernel
  double *xpr;
  double *th;                    // potential temperature atmx%t*(p00/atm1%pr)**rovcp (ithadv = 1)
  double *cr, *qdot;
  double *xkcr;
  // total tendencies (pc_total; pc_dynamic stays in the tendency kernels' registers)
  double *tten, *qvten, *qcten, *uten, *vten;
  double *ppten, *wten;
  // physics tendencies of the coupling seam (null: physics stubbed, the terms are 0)
  const double *tphy, *qvphy, *qcphy, *uphy, *vphy, *ppphy, *wphy;
  // semi-Lagrangian qv/qc tendency starts (isladvec = 1, k_sladv; null otherwise)
  const double *slqv, *slqc;
  // idiffu = 3: the column terms of k_nh_diffu6 (u, v, t, qv, qc, pp, w; null otherwise)
  double *d6u, *d6v, *d6t, *d6qv, *d6qc, *d6pp, *d6w;
  // iuwvadv = 1 (ibltyp = 2): the PBL-top level of vadv4d ind = 3 (null otherwise)
  const double* kpbl;
  // forecasts (atmc) and fixed moisture
  double *ct, *cqv, *cqc, *fqv, *fqc, *cu, *cv, *cpp, *cw, *cdt;
  unsigned* depplane;
  // sound work (Main/mod_sound.F90:40-60) that crosses a kernel boundary: the sweep's e, f
  // (k_nh_sound_bc -> k_nh_sound_cd), pi, the radiative condition's inputs and mask
  double *se, *sf, *spi, *estore, *astore, *tmask;
  unsigned long long* cfl;       // NH_CFL_SLOTS partial maxima of the step's CFL (non-negative
                                 // doubles as ordered bits), reduced by k_nh_advance
  unsigned long long* cfll;      // the same for the last acoustic sub-step alone (the value
                                 // the reference reports, Main/mod_sound.F90:634-646)
  // nqx = 5: atm1 qi, qr, qs (the water load of the adiabatic w term; null for nqx = 2)
  const double* qxa1[NQXH];
  // tfuse = 1: the time filters of t, qv, qc (Main/mod_tendency.F90:422-427) write the other
  // parity b* of those fields (k_nh_tend_c at non-negative forecasts, the negative-moisture fix
  // at the fixed points; k_nh_tend_c copies the points no filter writes); tfuse = 0: in place
  // in k_nh_tfilter_a1
  double *b1t, *b1qv, *b1qc, *b2t, *b2qv, *b2qc;
  int tfuse;
  // k_nh_tend_c lists its negative qv/qc forecasts (entry (k-1)*plane + ix, times 2,
  // plus the species bit) for k_nh_negfix, which visits the list instead of every point
  unsigned* neglist;
  int* negcnt;
};
constexpr int NH_CFL_SLOTS = 1024;
// k_nh_tend_c block: TC_J x TC_I cross points of one level
#ifndef TC_J
#define TC_J 32
#endif
#ifndef TC_I
#define TC_I 8
#endif
// rows of dot points per k_nh_tend_d block (64 x TD_I threads)
#ifndef TD_I
#define TD_I 8
#endif

struct QxArgs;
__global__ void k_nh_diffu6(Geom g, const Consts* __restrict__ c, NHFields f, QxArgs q);
__global__ void k_nh_decouple(Geom g, const Consts* __restrict__ c, NHFields f);
__global__ void k_nh_omega(Geom g, const Consts* __restrict__ c, NHFields f);
__global__ void k_nh_coeff_raw(Geom g, const Consts* __restrict__ c, NHFields f);
// B: the extra argument blocks (kernels.hpp): empty, Budget, and for QX = false Condtq or Budget, Condtq
template <bool QX, class... B>
__global__ void k_nh_tend_c(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, NHFields f, int wdiag, int istep, B... b);
__global__ void k_nh_tend_d(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, NHFields f, int istep);
__global__ void k_nh_negfix(Geom g, const Consts* __restrict__ c, NHFields f);
__global__ void k_nh_negfix_serial(Geom g, const Consts* __restrict__ c, NHFields f);
__global__ void k_nh_tfilter_a1(Geom g, const Consts* __restrict__ c, NHFields f);
__global__ void k_nh_a1_col(Geom g, const Consts* __restrict__ c, NHFields f);
__global__ void k_nh_check_dprd(Geom g, NHFields f, int* bad);
__global__ void k_nh_sound_uv(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, NHFields f, int istep, int fin, int first, int part);
__global__ void k_nh_sound_bc(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, NHFields f, int istep, int it);
__global__ void k_nh_tmask_gather(Geom g, const Consts* __restrict__ c, NHFields f, double* gbuf);
__global__ void k_nh_tmask(Geom g, const Consts* __restrict__ c, const double* __restrict__ gbuf, double* tmask);
__global__ void k_nh_sound_cd(Geom g, Geom ge, const double* __restrict__ est, const Consts* __restrict__ c, const StepState* __restrict__ s, NHFields f, int istep, int last, int nexta);
__global__ void k_nh_sound_final(Geom g, const Consts* __restrict__ c, NHFields f);
int nh_frame_ring(const Geom& g);     // k_nh_sound_final's points per level
__global__ void k_nh_advance(const Consts* __restrict__ c, StepState* s, NHFields f);
__global__ void k_nh_bdyval(Geom g, int kz, const StepState* __restrict__ s, NHFields f);
__global__ void k_nh_bdyval_w1(Geom g, NHFields f);

}  // namespace rcm
