// species.hip -- the hydrometeors beyond qc (nqx = 5: qi, qr, qs; physicsparam ipptls >= 2,
// Main/mod_params.F90:1358-1366), gfx950.
//
// The reference runs every hydrometeor n = iqfrst..iqlst through qc's chain of the dyn step:
// hadvqx (Main/mod_advection.F90:607-662, Main/mod_tendency.F90:1382), vadv4d ind 1 or 3
// (:847-966, :1388), diffu_x4d (Main/mod_diffusion.F90:792-947, :1526), the sums with qxphy
// (:332-335), the forecast, the exchange of atmc%qx and the negative-moisture fix (:375-393),
// filter_raw_4d with the zero floor (:426-427), and bdyval's boundary copies (Main/mod_bdycod.F90:
// 1143-1284) and inflow/outflow lines (:2153-2220).  The species never feed back into the other
// prognostics except through the total water load (k_columns' tvfac, the NH water loading),
// so they run in kernels of their own after the qv/qc update, with qc's operation order:
//
//  k_qx_tend   one level per block of 64 x 8 cross points, the cell's mass fluxes and every
//              species' decoupled atm1 (halo 1) and mkslice atm2 (halo 2) staged in LDS; the
//              forecast atmc%qx into cq (atm2 on the ring jce \ jci);
//  k_qx_fix    the negative-value fix and the RAW filter into the next buffers (points with a
//              serially dependent negative predecessor flag their plane), and the copies of the
//              points the update does not write (qfuse's keep copies of qv, qc);
//  k_qx_serial one wavefront per flagged (species, level) plane: the sweep in the reference's
//              i-major, j-minor order;
//  k_bdyval_qx bdyval's atm2 = atm1 boundary copies, then the inflow/outflow lines.
//
// The non-hydrostatic core (k_nh_qx_tend) adds the atmx%qx * cr term of adiabatic
// (Main/mod_tendency.F90:1615-1617) and updates the state in place: k_qx_fix / k_qx_serial then
// filter into the same buffers (each thread reads and writes only its own point's levels).
//
// The chemical tracers (rcmdyn_set_tracers) take the same chain with the differences of the
// family FamTr (kernels.hpp): no decoupling floor, vadv4d ind = 2, the fix factor 0.1, no NH cr
// term, nudge_chiten between advection and diffusion; k_bdyval_chi is chem_bdyval_coupled and
// k_tr_slice the chib3d export.  Up to NQXH tracers share a block, the group on the grid's z.
// Two switches complete tend's tracer chain: k_tr_cumtran (rcmdyn_set_cumtran) mixes the filtered
// levels over the convective column, and the TrBudget instances of the two tendency kernels
// (rcmdyn_set_tracer_budget) book the ichdiag terms.
//
// Transcendental-free: every result is bit-identical to the oracle's restatement
// (-ffp-contract=off).
#include "engine.hpp"
#include "kernels.hpp"
#include "kernels_nh.hpp"
#include "devcommon.hpp"
#include "qxcommon.hpp"

namespace rcm {

namespace {
// QBJ x QBI (kernels.hpp): the launch's grid and block come from the same constants
constexpr int QDW = QBJ + 1, QDH = QBI + 1;    // dot points j..j+QBJ, i..i+QBI
constexpr int QW1 = QBJ + 2, QH1 = QBI + 2;    // halo 1
constexpr int QW2 = QBJ + 4, QH2 = QBI + 4;    // halo 2
}  // namespace

// K_QX1.  The tendencies and forecast of the hydrometeors beyond qc at the cross points of the
// tile and its ghost ring (jcx x icx, as k_scalars: the ring is what the exchange of atmc%qx
// would deliver), one level per block.  Reads the scaled diffusion coefficient k_scalars
// stored (xkc * rdxsq * p*b at the interior points) and qdot of k_columns.
// F: the family (kernels.hpp).  A tracer launch carries its groups on z = group * kz + level.
// B...: TrBudget for the tracers' budget instance (rcmdyn_set_tracer_budget): it snapshots the
// running chidyn around each stage as tend does with chiten0 (Main/mod_tendency.F90:1403-1412,
// 1503-1511, 1540-1542) and adds the difference times rw to the stage's accumulator
// (extracttenchi, :2177-2207) at the tile's own jci x ici; the ring's forecasts book nothing.
template <class F, class... B>
__global__ __launch_bounds__(QBT) void k_qx_tend(Geom g, const Consts* __restrict__ c,
                                                 const StepState* __restrict__ s, Fields f, typename F::Args fa,
                                                 B... xb) {
  constexpr bool BUD = pack_has<TrBudget, B...>;
  const TrBudget bd = pack_get<TrBudget>(xb...);
  __shared__ double sUMC[QDH][QDW], sVMC[QDH][QDW];
  __shared__ double sX[NQXH][QH1][QW1];          // atmx%qx = max(atm1 * rpsa, 0) (tracers: no floor), halo 1
  __shared__ double sB[NQXH][QH2][QW2];          // qxb3d = max(atm2 * (1/psb), 0), halo 2
  const int tid = threadIdx.x;
  const int kz = c->kz;
  const int grp = F::grouped ? (int)blockIdx.z / kz : 0, k = (F::grouped ? (int)blockIdx.z % kz : (int)blockIdx.z) + 1;
  const QxArgs& q = F::group(fa, grp);
  const int J0 = g.jcx1() + (int)blockIdx.x * QBJ, I0 = g.icx1() + (int)blockIdx.y * QBI;
  const uint32_t P8 = g.P8, L8 = g.L8, kof = (uint32_t)(k - 1) * L8;
  (void)P8;
  const int jlo = g.j0, jhi = g.j0 + g.nj - 1, ilo = g.i0, ihi = g.i0 + g.ni - 1;
  const int nsp = q.nsp;
  const int tj = tid % QBJ, ti = tid / QBJ;
  const int j = J0 + tj, i = I0 + ti;
  const bool valid = j <= g.jcx2() && i <= g.icx2();
  const uint32_t o2 = valid ? g.o2(j, i) : g.o2(g.jce1, g.ice1), o3 = o2 + kof;
  // ---- stage (every load of a set before its LDS writes; lanes past the frame stage zero)
  for (int t = tid; t < QDW * QDH; t += QBT) {
    const int jj = t % QDW, ii = t / QDW, jg = J0 + jj, ig = I0 + ii;
    const bool ok = jg <= jhi && ig <= ihi;
    const uint32_t q2 = ok ? g.o2(jg, ig) : o2;
    const double m = LD(f.msfd, q2), u = LD(f.a1u, q2 + kof), v = LD(f.a1v, q2 + kof);
    sUMC[ii][jj] = ok ? u * m : 0.0;
    sVMC[ii][jj] = ok ? v * m : 0.0;
  }
  for (int t = tid; t < QW1 * QH1; t += QBT) {
    const int jj = t % QW1, ii = t / QW1, jg = J0 - 1 + jj, ig = I0 - 1 + ii;
    const bool ok = jg >= jlo && jg <= jhi && ig >= ilo && ig <= ihi;
    const uint32_t q2 = ok ? g.o2(jg, ig) : o2;
    const double rp = LD(f.rpsa, q2);
    double x[NQXH];
#pragma unroll
    for (int n = 0; n < NQXH; n++) x[n] = n < nsp ? LD(q.a1[n], q2 + kof) : 0.0;
#pragma unroll
    for (int n = 0; n < NQXH; n++) sX[n][ii][jj] = ok ? (F::floor ? dmax(x[n] * rp, d_zero) : x[n] * rp) : 0.0;
  }
  for (int t = tid; t < QW2 * QH2; t += QBT) {
    const int jj = t % QW2, ii = t / QW2, jg = J0 - 2 + jj, ig = I0 - 2 + ii;
    const bool ok = jg >= jlo && jg <= jhi && ig >= ilo && ig <= ihi;
    const uint32_t q2 = ok ? g.o2(jg, ig) : o2;
    const double r = LD(f.rpsb, q2);
    double x[NQXH];
#pragma unroll
    for (int n = 0; n < NQXH; n++) x[n] = n < nsp ? LD(q.a2[n], q2 + kof) : 0.0;
#pragma unroll
    for (int n = 0; n < NQXH; n++) sB[n][ii][jj] = ok ? dmax(x[n] * r, d_zero) : 0.0;
  }
  __syncthreads();
  if (!valid) return;
  if (!g.gci(j, i)) {
    // the ring jce \ jci: atmc%qx = atm2%qx (:375-377)
    for (int n = 0; n < nsp; n++) ST(q.cq[n], o3, LD(q.a2[n], o3));
    return;
  }
  const double dt = s->dt;
  const double ps = LD(f.psa, o2), xm = LD(f.xmsf, o2), xkcs = LD(f.xkcs, o3);
  const double q0 = LD(f.qdot, o3), q1 = LD(f.qdot, o3 + L8);
  // start_advect's mass fluxes of the cell (Main/mod_advection.F90:111-120)
  const double uavg1 = sUMC[ti + 1][tj] + sUMC[ti][tj];
  const double uavg2 = sUMC[ti + 1][tj + 1] + sUMC[ti][tj + 1];
  const double vavg1 = sVMC[ti][tj + 1] + sVMC[ti][tj];
  const double vavg2 = sVMC[ti + 1][tj + 1] + sVMC[ti + 1][tj];
  const int kpb = f.kpbl ? (int)LD(f.kpbl, o2) : 0;
  const bool bown = BUD && in(j, g.jci1, g.jci2) && in(i, g.ici1, g.ici2);
  for (int n = 0; n < nsp; n++) {
    const int b1 = tj + 1, a1 = ti + 1, b2 = tj + 2, a2 = ti + 2;
    // the budget instance: acc = acc + (after - before) * rw of term m for this tracer
    auto bud = [&](int m, double x) {
      if (bown) {
        double* acc = bd.acc[m * bd.ntr + grp * NQXH + n];
        ST(acc, o3, LD(acc, o3) + x * bd.rw);
      }
    };
    [[maybe_unused]] double t0 = d_zero;     // chiten0: the running chidyn before the stage
#define X1(dj, di) sX[n][a1 + (di)][b1 + (dj)]
    // hadvqx (:639-653), or the semi-Lagrangian start of qxdyn (:1378-1380)
    double tq = c->isladvec ? LD(q.sl[n], o3)
                            : d_zero + hadv_flux(c, xm, ps, uavg1, uavg2, vavg1, vavg2, X1(0, 0), X1(-1, 0),
                                                 X1(1, 0), X1(0, -1), X1(0, 1), 0);
#undef X1
    if constexpr (BUD) { bud(RCMDYN_TRDIAG_ADVH, tq); t0 = tq; }
    // vadv4d (:859-961): ind = 1, or 3 with iuwvadv = 1 (the PBL-top rule at kpbl)
    const double* qa = q.a1[n];
    const double c0 = LD(qa, o3);
    const double cm = (k >= 2) ? LD(qa, o3 - L8) : 0.0, cp = (k < kz) ? LD(qa, o3 + L8) : 0.0;
    if (f.kpbl) {
      auto fk = [&](int kk) { return LD(qa, o2 + (uint32_t)(kk - 1) * L8); };
      if (k >= 2) tq = tq + (uw_fg(c, k, kpb, c0, cm, fk) * q0) * c->xds[k];
      if (k + 1 <= kz) tq = tq - (uw_fg(c, k + 1, kpb, cp, c0, fk) * q1) * c->xds[k];
    } else {
      const double thr = F::thr(ps);
      if (k >= 2) {
        const double fl = (q0 > d_zero) ? ((cm > thr) ? q0 * (c->twt1[k] * c0 + c->twt2[k] * cm) : d_zero)
                                        : ((c0 > thr) ? q0 * (c->twt1[k] * c0 + c->twt2[k] * cm) : d_zero);
        tq = tq + fl * c->xds[k];
      }
      if (k + 1 <= kz) {
        const double fl = (q1 > d_zero) ? ((c0 > thr) ? q1 * (c->twt1[k + 1] * cp + c->twt2[k + 1] * c0) : d_zero)
                                        : ((cp > thr) ? q1 * (c->twt1[k + 1] * cp + c->twt2[k + 1] * c0) : d_zero);
        tq = tq - fl * c->xds[k];
      }
    }
    if constexpr (BUD) { bud(RCMDYN_TRDIAG_ADVV, tq - t0); t0 = tq; }
    // nudge_chiten, ichebdy = 1 (Main/chemlib/mod_che_bdyco.F90:898-982), on atm2 (Main/
    // mod_tendency.F90:1507) between the advection and the diffusion: the band's south / north
    // points sum fls1..4 as west, east, south, north, its west / east points as south, north,
    // west, east
    if constexpr (F::relax) {
      const int rg = fa.relax ? (int)f.rgcr[o2 >> 3] : 0;
      if (rg > 0) {
        const double xt = s->xbctime + dt;
        const int ib = f.ibcr[o2 >> 3];
        const double xf = fa.cefc[(k - 1) * c->nspgx + ib - 1], xg = fa.cegc[(k - 1) * c->nspgx + ib - 1];
#define FLS(dj, di) bdy_minus_state(LD(q.b0[n], O3(dj, di)), LD(q.bt[n], O3(dj, di)), LD(q.a2[n], O3(dj, di)), xt)
        if (rg <= 2) tq = relax(tq, xf, xg, FLS(0, 0), FLS(-1, 0), FLS(1, 0), FLS(0, -1), FLS(0, 1));
        else tq = relax(tq, xf, xg, FLS(0, 0), FLS(0, -1), FLS(0, 1), FLS(-1, 0), FLS(1, 0));
#undef FLS
      }
    }
    // cbdydiag is booked on every iboudy (:1503-1511): + 0.0 where nothing was relaxed
    if constexpr (BUD) { bud(RCMDYN_TRDIAG_BDY, tq - t0); t0 = tq; }
    // diffu_x4d on the mkslice field qxb3d; idiffu = 3: k_diffu6's column term (as k_scalars)
    if (c->idiffu == 3) {
      if (j == g.jci2 || (!g.bl && j == g.jce1 - 1)) tq = tq + LD(q.d6[n], o3);
    } else {
      tq = diffu_x(g, c, j, i, tq, xkcs, [&](int dj, int di) { return sB[n][a2 + di][b2 + dj]; });
    }
    if constexpr (BUD) bud(RCMDYN_TRDIAG_DIFH, tq - t0);
    // qxten = (0 + qxdyn) + qxphy (:332-335); the forecast (:375-380)
    tq = (d_zero + tq) + (q.phy[n] ? LD(q.phy[n], o3) : d_zero);
    ST(q.cq[n], o3, LD(q.a2[n], o3) + dt * tq);
  }
}

// K_QX1 (non-hydrostatic).  The hydrometeor chains of k_nh_tend_c's qc (kernels_nh.hip) for
// qi, qr, qs at the interior cross points (owned points only, as the NH tendency kernels):
// hadvqx, vadv4d ind 1 / 3, + atmx%qx * cr (:1615-1617), diffu_x4d on the scaled xkcr, the
// sums with qxphy, the forecast; the ring jce \ jci takes atm2.
// B...: TrBudget for the tracers' budget instance, the same four stages as k_qx_tend (no tracer has
// an adiabatic term).
template <class F, class... B>
__global__ __launch_bounds__(256) void k_nh_qx_tend(Geom g, const Consts* __restrict__ c,
                                                    const StepState* __restrict__ s, NHFields f, typename F::Args fa,
                                                    B... xb) {
  constexpr bool BUD = pack_has<TrBudget, B...>;
  const TrBudget bd = pack_get<TrBudget>(xb...);
  const int j = g.jce1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ice1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int kz = c->kz;
  const int grp = F::grouped ? (int)blockIdx.z / kz : 0, k = (F::grouped ? (int)blockIdx.z % kz : (int)blockIdx.z) + 1;
  const QxArgs& q = F::group(fa, grp);
  if (!(in(j, g.jce1, g.jce2) && in(i, g.ice1, g.ice2))) return;
  const int nsp = q.nsp;
  if (!(in(j, g.jci1, g.jci2) && in(i, g.ici1, g.ici2))) {
    for (int n = 0; n < nsp; n++) F3(q.cq[n], j, i, k) = F3(q.a2[n], j, i, k);
    return;
  }
  const double dt = s->dt;
  const double xmf = F2(f.xmsf, j, i), ps = F2(f.psa, j, i), pbs = F2(f.psb, j, i);
  const double m00 = F2(f.msfd, j, i), m01 = F2(f.msfd, j, i + 1), m10 = F2(f.msfd, j + 1, i),
               m11 = F2(f.msfd, j + 1, i + 1);
  // start_advect's mass fluxes (umc = atm1 u * msfd)
  const double u1 = F3(f.a1u, j, i + 1, k) * m01 + F3(f.a1u, j, i, k) * m00;
  const double u2 = F3(f.a1u, j + 1, i + 1, k) * m11 + F3(f.a1u, j + 1, i, k) * m10;
  const double v1 = F3(f.a1v, j + 1, i, k) * m10 + F3(f.a1v, j, i, k) * m00;
  const double v2 = F3(f.a1v, j + 1, i + 1, k) * m11 + F3(f.a1v, j, i + 1, k) * m01;
  const double r0 = F2(f.rpsa, j, i), rw = F2(f.rpsa, j - 1, i), re = F2(f.rpsa, j + 1, i),
               rs = F2(f.rpsa, j, i - 1), rn = F2(f.rpsa, j, i + 1);
  const double cr = F3(f.cr, j, i, k);
  const double xkc = F3(f.xkcr, j, i, k) * c->rdxsq * pbs;      // calc_coeff's xkc
  const double thr = F::thr(ps);
  const int kpb = f.kpbl ? (int)F2(f.kpbl, j, i) : 0;
  // atmx of the family: the species' floor at zero, the tracers' plain product
  auto dec = [](double x, double r) { return F::floor ? dmax(x * r, d_zero) : x * r; };
  for (int n = 0; n < nsp; n++) {
    const double* a = q.a1[n];
    double cd;
    auto bud = [&](int m, double x) {
      double* acc = bd.acc[m * bd.ntr + grp * NQXH + n];
      F3(acc, j, i, k) = F3(acc, j, i, k) + x * bd.rw;
    };
    [[maybe_unused]] double t0 = d_zero;     // chiten0: the running chidyn before the stage
    if (c->isladvec) {
      cd = d_zero + F3(q.sl[n], j, i, k);
    } else {
      const double xc = dec(F3(a, j, i, k), r0), xw = dec(F3(a, j - 1, i, k), rw);
      const double xe = dec(F3(a, j + 1, i, k), re), xs = dec(F3(a, j, i - 1, k), rs);
      const double xn = dec(F3(a, j, i + 1, k), rn);
      cd = d_zero + hadv_flux(c, xmf, ps, u1, u2, v1, v2, xc, xw, xe, xs, xn, 0);
    }
    if constexpr (BUD) { bud(RCMDYN_TRDIAG_ADVH, cd); t0 = cd; }
    auto cflux = [&](int kk) {
      const double svv = F3(f.qdot, j, i, kk);
      const double fk = F3(a, j, i, kk), fkm = F3(a, j, i, kk - 1);
      if (f.kpbl) return uw_fg(c, kk, kpb, fk, fkm, [&](int qq) { return F3(a, j, i, qq); }) * svv;
      if (svv > d_zero) return (fkm > thr) ? svv * (c->twt1[kk] * fk + c->twt2[kk] * fkm) : d_zero;
      return (fk > thr) ? svv * (c->twt1[kk] * fk + c->twt2[kk] * fkm) : d_zero;
    };
    if (k >= 2) cd = cd + cflux(k) * c->xds[k];
    if (k + 1 <= kz) cd = cd - cflux(k + 1) * c->xds[k];
    if constexpr (F::cr) cd = cd + dmax(F3(a, j, i, k) * r0, d_zero) * cr;
    if constexpr (BUD) { bud(RCMDYN_TRDIAG_ADVV, cd - t0); t0 = cd; }
    if constexpr (F::relax) {     // nudge_chiten, as in k_qx_tend
      const int rg = fa.relax ? (int)F2(f.rgcr, j, i) : 0;
      if (rg > 0) {
        const double xt = s->xbctime + dt;
        const int ib = F2(f.ibcr, j, i);
        const double xf = fa.cefc[(k - 1) * c->nspgx + ib - 1], xg = fa.cegc[(k - 1) * c->nspgx + ib - 1];
#define FLS(dj, di) \
  bdy_minus_state(F3(q.b0[n], j + (dj), i + (di), k), F3(q.bt[n], j + (dj), i + (di), k), F3(q.a2[n], j + (dj), i + (di), k), xt)
        if (rg <= 2) cd = relax(cd, xf, xg, FLS(0, 0), FLS(-1, 0), FLS(1, 0), FLS(0, -1), FLS(0, 1));
        else cd = relax(cd, xf, xg, FLS(0, 0), FLS(0, -1), FLS(0, 1), FLS(-1, 0), FLS(1, 0));
#undef FLS
      }
    }
    if constexpr (BUD) { bud(RCMDYN_TRDIAG_BDY, cd - t0); t0 = cd; }
    if (c->idiffu == 3) {
      if (j == g.jci2) cd = cd + F3(q.d6[n], j, i, k);
    } else {
      // diffu_x4d on mkslice's qxb3d = max(atm2 * (1/psb), 0), Main/mod_diffusion.F90:792-947 (an
      // owned interior point, where diffu_x's global index tests are the tile's)
      const double* b = q.a2[n];
      auto fb = [&](int dj, int di) {
        return dmax(F3(b, j + dj, i + di, k) * F2(f.rpsb, j + dj, i + di), d_zero);
      };
      cd = diffu_x(g, c, j, i, cd, xkc, fb);
    }
    if constexpr (BUD) bud(RCMDYN_TRDIAG_DIFH, cd - t0);
    const double qt = d_zero + cd + (q.phy[n] ? F3(q.phy[n], j, i, k) : d_zero);
    F3(q.cq[n], j, i, k) = F3(q.a2[n], j, i, k) + dt * qt;
  }
}

// K_QX2.  The negative-moisture fix (:382-393) and filter_raw_4d (:426-427, gnu2, the zero
// floor) of the hydrometeors beyond qc on the owned interior jci x ici, into the next buffers; the
// copies of the column box's other points (atm1, and atm2 on owned points: bdyval and the next
// step's exchange read them).  A negative point with a negative sweep-predecessor flags its
// (species, level) plane for k_qx_serial; the others read original values only.
template <class F>
__global__ void k_qx_fix(Geom g, const Consts* __restrict__ c, typename F::Args fa) {
  const int j = g.jdx1() + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.idx1() + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int grp = F::grouped ? (int)blockIdx.z / c->kz : 0;
  const int k = (F::grouped ? (int)blockIdx.z % c->kz : (int)blockIdx.z) + 1;
  const QxArgs& q = F::group(fa, grp);
  if (j > g.jdx2() || i > g.idx2()) return;
  const uint32_t o3 = g.o3(j, i, k);
  const bool ci = in(j, g.jci1, g.jci2) && in(i, g.ici1, g.ici2);
  const bool own = in(j, g.jde1, g.jde2) && in(i, g.ide1, g.ide2);
  for (int n = 0; n < q.nsp; n++) {
    const double a1 = LD(q.a1[n], o3), a2 = LD(q.a2[n], o3);
    if (!ci) {
      if (q.b1[n] != q.a1[n]) {             // the NH core filters in place: nothing to keep
        ST(q.b1[n], o3, a1);
        if (own) ST(q.b2[n], o3, a2);
      }
      continue;
    }
    double v = LD(q.cq[n], o3);
    // a dependent point flags its row with a plain store (every writer stores the same 1, so
    // it holds for any block shape; the lanes of one row store one address, a single
    // transaction; device-scope atomics on the few bitmap words serialised at the memory side:
    // 190 of this kernel's 215 us at C3)
    const bool dp = v < d_zero && negfix_dependent(g, q.cq[n], j, i, k);
    if (dp) {
      q.depf[(n * c->kz + (k - 1)) * (g.ici2 - g.ici1 + 1) + (i - g.ici1)] = 1u;
      continue;
    }
    if (v < d_zero) {
      v = negfix_sum<F>(g, q.cq[n], q.fq[n], j, i, k, false);
      ST(q.fq[n], o3, v);
    }
    double n1, n2;
    raw_qc(c, a1, a2, v, n1, n2);
    ST(q.b2[n], o3, n2);
    ST(q.b1[n], o3, n1);
  }
}

// K_QX3.  The serial sweep of one (species, level) plane by one wavefront (negfix_sweep,
// qxcommon.hpp): the marked rows' dependent negative points in i-major, j-minor order, each
// fixed from its already-fixed predecessors, then RAW-filtered; dynamic LDS negfix_lds(g)
// filter_raw_4d of a fixed point (gnu2, the zero floor) from its atm1, atm2 (x)
struct QxRaw {
  static constexpr int NI = 2;
  Geom g;
  const Consts* c;
  const double *a1, *a2;
  double *b1, *b2;
  int k;
  __device__ void load(int j, int i, double* x) const { x[0] = F3(a1, j, i, k); x[1] = F3(a2, j, i, k); }
  __device__ void apply(int j, int i, double v, const double* x) const {
    double n1, n2;
    raw_qc(c, x[0], x[1], v, n1, n2);
    F3(b2, j, i, k) = n2;
    F3(b1, j, i, k) = n1;
  }
};
// one (species, level) plane of k_qx_serial (lds: negfix_lds(g) doubles)
template <class F>
__device__ __forceinline__ void qx_serial_plane(const Geom& g, const Consts* __restrict__ c, const QxArgs& q,
                                                int plane, double* lds) {
  const int kz = c->kz;
  if (plane >= q.nsp * kz) return;
  const int n = plane / kz, k = plane % kz + 1;
  {
    // k_qx_fix's row flags into this plane's bitmap words (negfix_resolve reads those), flags
    // cleared for the next step.  negfix_collect's loop, but every word is stored where the
    // helper ORs the non-zero ones in (the words are zero here: zero at allocation, marked by
    // nothing else, cleared by negfix_resolve): the OR's load ahead of the barrier measured
    // 0.5 us on k_negfix_serial_qx's serial chain (C3: 195.2-195.6 against 194.5-195.0 us)
    const int R = g.ici2 - g.ici1 + 1, T = (int)(blockDim.x * blockDim.y * blockDim.z);
    const int tid = (int)(threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z));
    unsigned* fl = q.depf + plane * R;
    unsigned* words = q.dep + plane * negfix_rowwords(g);
    for (int b = 0; b < R; b += T) {
      const int r = b + tid;
      const bool f = r < R && fl[r] != 0u;
      if (f) fl[r] = 0u;
      const unsigned long long m = __ballot(f);
      if (r < R && (r & 31) == 0) words[r >> 5] = (unsigned)(m >> (r & 32));
    }
    __syncthreads();
  }
  negfix_resolve<F>(g, q.cq[n], q.fq[n], q.dep, plane, k, lds, negfix_lds(g), NoPost{}, [](int, int, double) {}, c->negfix_mode);
}
// a block per plane; the tracers: NQXH * kz blocks per group
template <class F>
__global__ __launch_bounds__(512) void k_qx_serial(Geom g, const Consts* __restrict__ c, typename F::Args fa) {
  extern __shared__ double lds[];
  const int per = NQXH * c->kz, b = (int)blockIdx.x;
  qx_serial_plane<F>(g, c, F::group(fa, F::grouped ? b / per : 0), F::grouped ? b % per : b, lds);
}
// hydrostatic qfuse: the serial chains of the qv / qc planes (blocks [0, 2 kz), as
// k_negfix_serial) and of the species planes (k_qx_serial) in one launch after the split
// corrections: the two sets of planes are independent, so the launch takes the longer chain's
// time instead of the sum (k_qx_fix's flags wait for it; nothing of the split reads the species)
__global__ __launch_bounds__(512) void k_negfix_serial_qx(Geom g, const Consts* __restrict__ c, QFix qf, QxArgs q) {
  extern __shared__ double lds[];
  const int b = (int)blockIdx.x, kz = c->kz;
  if (b >= 2 * kz) {
    qx_serial_plane<FamQx>(g, c, q, b - 2 * kz, lds);
    return;
  }
  const int n = b / kz, k = b % kz + 1;
  if (qf.depf) {
    negfix_collect(g, qf.depf, qf.depplane, b, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
  }
  negfix_resolve(g, n ? qf.cqc : qf.cqv, n ? qf.fqc : qf.fqv, qf.depplane, b, k, lds, negfix_lds(g), NoPost{},
                 [](int, int, double) {}, c->negfix_mode);
}

// filter_raw_4d of the points k_qx_serial fixed, a thread per interior point of a
// (species, level) plane (z = plane)
template <class F>
__global__ void k_qx_post(Geom g, const Consts* __restrict__ c, typename F::Args fa) {
  const int j = g.jci1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ici1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int kz = c->kz, per = NQXH * kz, z = (int)blockIdx.z;
  const QxArgs& q = F::group(fa, F::grouped ? z / per : 0);
  const int plane = F::grouped ? z % per : z, n = plane / kz, k = plane % kz + 1;
  if (j > g.jci2 || i > g.ici2 || n >= q.nsp) return;
  if (!negfix_is_dependent(g, q.cq[n], j, i, k)) return;
  const QxRaw acc{g, c, q.a1[n], q.a2[n], q.b1[n], q.b2[n], k};
  double x[2];
  acc.load(j, i, x);
  acc.apply(j, i, F3(q.fq[n], j, i, k), x);
}

// K_QX4.  bdyval for the hydrometeors beyond qc, one block per (level, species): while
// integrating, atm2 = atm1 on the cross boundary lines (Main/mod_bdycod.F90:1143-1284: west /
// east on ici, south / north on jce), then (not present_qc) the inflow/outflow lines of qc's
// rule (:2153-2220), which read the bdyuv slices and the boundary p* of this bdyval.
__global__ void k_bdyval_qx(Geom g, const StepState* __restrict__ s, QxArgs q, int integ, int do_qc,
                            const double* __restrict__ psa, Slices sl, long slen) {
  const int k = (int)blockIdx.x + 1, n = (int)blockIdx.y;
  if (n >= q.nsp) return;
  double* a1 = q.a1[n];
  double* a2 = q.a2[n];
  if (integ > 0 || (integ < 0 && s->lcount > 0)) {
    for (int i = g.ici1 + (int)threadIdx.x; i <= g.ici2; i += (int)blockDim.x) {
      if (g.bl) F3(a2, g.jce1, i, k) = F3(a1, g.jce1, i, k);
      if (g.br) F3(a2, g.jce2, i, k) = F3(a1, g.jce2, i, k);
    }
    for (int j = g.jce1 + (int)threadIdx.x; j <= g.jce2; j += (int)blockDim.x) {
      if (g.bb) F3(a2, j, g.ice1, k) = F3(a1, j, g.ice1, k);
      if (g.bt) F3(a2, j, g.ice2, k) = F3(a1, j, g.ice2, k);
    }
    __syncthreads();
  }
  bdyval_qc_level(g, do_qc, 0, a1, nullptr, [&](int j, int i) { return F2(psa, j, i); }, sl, slen, k);
}

// K_TR4.  chem_bdyval_coupled with ichebdy = 1 (Main/chemlib/mod_che_bdyco.F90:565-758), one
// block per (level, tracer): while integrating, chib = chia on the boundary lines (west / east
// on ice, south / north on jci: the corners go with west / east, where qx's copies take them with
// south / north), then chia = chib0 + xt * chibt (west / east on ici, south / north on jce).
__global__ void k_bdyval_chi(Geom g, const StepState* __restrict__ s, TrArgs a, int ntr, int integ, int pre_clock,
                             double dtsec) {
  const int k = (int)blockIdx.x + 1, n = (int)blockIdx.y;
  if (n >= ntr) return;
  const QxArgs& q = a.tab[n / NQXH];
  const int m = n % NQXH;
  double* a1 = q.a1[m];
  double* a2 = q.a2[m];
  const double* b0 = q.b0[m];
  const double* bt = q.bt[m];
  if (integ > 0 || (integ < 0 && s->lcount > 0)) {
    for (int i = g.ice1 + (int)threadIdx.x; i <= g.ice2; i += (int)blockDim.x) {
      if (g.bl) F3(a2, g.jce1, i, k) = F3(a1, g.jce1, i, k);
      if (g.br) F3(a2, g.jce2, i, k) = F3(a1, g.jce2, i, k);
    }
    for (int j = g.jci1 + (int)threadIdx.x; j <= g.jci2; j += (int)blockDim.x) {
      if (g.bb) F3(a2, j, g.ice1, k) = F3(a1, j, g.ice1, k);
      if (g.bt) F3(a2, j, g.ice2, k) = F3(a1, j, g.ice2, k);
    }
    __syncthreads();
  }
  const double dt = pre_clock ? ((s->lcount + 1 == 2) ? d_two * dtsec : s->dt) : s->dt;
  const double xt = s->xbctime + dt;
  for (int i = g.ici1 + (int)threadIdx.x; i <= g.ici2; i += (int)blockDim.x) {
    if (g.bl) F3(a1, g.jce1, i, k) = F3(b0, g.jce1, i, k) + xt * F3(bt, g.jce1, i, k);
    if (g.br) F3(a1, g.jce2, i, k) = F3(b0, g.jce2, i, k) + xt * F3(bt, g.jce2, i, k);
  }
  for (int j = g.jce1 + (int)threadIdx.x; j <= g.jce2; j += (int)blockDim.x) {
    if (g.bb) F3(a1, j, g.ice1, k) = F3(b0, j, g.ice1, k) + xt * F3(bt, j, g.ice1, k);
    if (g.bt) F3(a1, j, g.ice2, k) = F3(b0, j, g.ice2, k) + xt * F3(bt, j, g.ice2, k);
  }
}

// mkslice's chib3d (Main/mod_slice.F90:196-200) on the tile's cross points, z = tracer * kz + level
__global__ void k_tr_slice(Geom g, int kz, int ntr, TrArgs a, const double* __restrict__ rpsb, double* const* out) {
  const int j = g.jce1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ice1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int n = (int)blockIdx.z / kz, k = (int)blockIdx.z % kz + 1;
  if (j > g.jce2 || i > g.ice2 || n >= ntr) return;
  const double* a2 = a.tab[n / NQXH].a2[n % NQXH];
  F3(out[n], j, i, k) = dmax(F3(a2, j, i, k) * F2(rpsb, j, i), d_zero);
}

// K_TR5.  cumtran2 (Main/chemlib/mod_che_cumtran.F90:132-156; tend calls it on atm1%chi, atm2%chi
// after timefilter_apply and before the clock advance, Main/mod_tendency.F90:595-603): the mixing of
// every tracer over the convective column, on the two filtered time levels b1 / b2 (the NH core: a1 /
// a2 in place) at the tile's own jci x ici.  A thread per (j, i, tracer), lanes along j; the sums run
// serially in k in the text's order.  The launch sits in the captured step, so the act test (rcmtimer%
// integrating and syncro_cum%act on the clock of the tend being completed, wave-uniform) comes ahead of
// every other load, and a wave whose columns are all non-convective leaves after the two 2-D loads.
// cu.conv: cconvdiag (:159-166), the pseudo-tendency of atm2 with the tend's dt; every point of an
// acting tend books it, the untouched ones (x - x) / dt * 2 * cfdout = + 0.0.
__global__ __launch_bounds__(256) void k_tr_cumtran(Geom g, const Consts* __restrict__ c,
                                                    const StepState* __restrict__ s, TrArgs a, int ntr, TrCum cu) {
  const long long lc = s->lcount;
  if (!(lc > 0 && lc % cu.ncum == 0)) return;
  const int j = g.jci1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ici1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int n = (int)blockIdx.z;
  if (j > g.jci2 || i > g.ici2 || n >= ntr) return;
  const int kz = c->kz;
  const bool mix = F2(cu.dotran, j, i) != d_zero;
  const int ktop = (int)F2(cu.ktop, j, i);
  const int kctop = mix && ktop > 0 ? (ktop > 4 ? ktop : 4) : kz + 1;
  double* conv = cu.conv ? cu.conv[n] : nullptr;
  if (kctop > kz && !conv) return;
  const QxArgs& q = a.tab[n / NQXH];
  double* xa = q.b1[n % NQXH];
  double* xb = q.b2[n % NQXH];
  // both passes walk the column in chunks of CK levels, the chunk's loads issued together (levels
  // past kz load level kz and are not used): the sums still add one level after the other
  constexpr int CK = 4;
  double deltas = d_zero, chiabar = d_zero, chibbar = d_zero;
  for (int k0 = kctop; k0 <= kz; k0 += CK) {
    double va[CK], vb[CK];
#pragma unroll
    for (int u = 0; u < CK; u++) {
      const int k = k0 + u <= kz ? k0 + u : kz;
      va[u] = F3(xa, j, i, k);
      vb[u] = F3(xb, j, i, k);
    }
#pragma unroll
    for (int u = 0; u < CK; u++) {
      if (k0 + u > kz) break;
      const double ds = c->dsigma[k0 + u];
      deltas = deltas + ds;
      chiabar = chiabar + va[u] * ds;
      chibbar = chibbar + vb[u] * ds;
    }
  }
  const double dt = s->dt;
  for (int k0 = conv ? 1 : kctop; k0 <= kz; k0 += CK) {
    double va[CK], vb[CK], vf[CK], vc[CK];
#pragma unroll
    for (int u = 0; u < CK; u++) {
      const int k = k0 + u <= kz ? k0 + u : kz;
      va[u] = F3(xa, j, i, k);
      vb[u] = F3(xb, j, i, k);
      vf[u] = F3(cu.cldfra, j, i, k);
      vc[u] = conv ? F3(conv, j, i, k) : d_zero;
    }
#pragma unroll
    for (int u = 0; u < CK; u++) {
      const int k = k0 + u;
      if (k > kz) break;
      const double b0 = vb[u];
      double bn = b0;
      if (k >= kctop) {
        const double cumfrc = vf[u];
        F3(xa, j, i, k) = va[u] * (d_one - cumfrc) + cumfrc * chiabar / deltas;
        bn = b0 * (d_one - cumfrc) + cumfrc * chibbar / deltas;
        F3(xb, j, i, k) = bn;
      }
      if (conv) F3(conv, j, i, k) = vc[u] + (bn - b0) / dt * d_two * cu.cfdout;
    }
  }
}

// the instances of both families
#define RCM_QX_TEND(F, ...)                                                                                        \
  template __global__ void k_qx_tend<F, ##__VA_ARGS__>(Geom, const Consts* __restrict__,                           \
                                                       const StepState* __restrict__, Fields, typename F::Args,   \
                                                       ##__VA_ARGS__);                                             \
  template __global__ void k_nh_qx_tend<F, ##__VA_ARGS__>(Geom, const Consts* __restrict__,                        \
                                                          const StepState* __restrict__, NHFields,                 \
                                                          typename F::Args, ##__VA_ARGS__);
#define RCM_QX_INSTANCES(F)                                                                                        \
  RCM_QX_TEND(F)                                                                                                   \
  template __global__ void k_qx_fix<F>(Geom, const Consts* __restrict__, typename F::Args);                         \
  template __global__ void k_qx_serial<F>(Geom, const Consts* __restrict__, typename F::Args);                      \
  template __global__ void k_qx_post<F>(Geom, const Consts* __restrict__, typename F::Args);
RCM_QX_INSTANCES(FamQx)
RCM_QX_INSTANCES(FamTr)
RCM_QX_TEND(FamTr, TrBudget)          // the tracers' budget instance
#undef RCM_QX_INSTANCES
#undef RCM_QX_TEND

}  // namespace rcm
