// subex.hpp -- the per-point statements of the SUBEX cloud fraction and rain columns (ipptls = 1):
// cldfrac with subex_cldfrac (Main/mod_micro_interface.F90:211-362, Main/cloudlib/
// mod_cloud_subex.F90:46-107; icldfrac = 0, icldmstrat = 0) and subex (Main/microlib/
// mod_micro_subex.F90:99-393; the non-aerosol dqc, l_lat_hack = .false., the idynamic 1 / 2 form
// with the * psb tendencies), stated once for the kernels of subex.hip.
//
// The one transcendental of a step is 10**(-0.48911 + 0.01344 * tcel) of qcth: rcm_pow10 of
// fastmath.hpp, which is plain + - * /, one FMA, rint and ldexp and so gives the host and the
// device equal bits (rcm_powpos(10.0, x) would too, but rounds x * log(10) first: up to 8 ulp).
// The chis table of allocate_micro (:117-120) is formed with rcm_exp for the same reason.
// Everything else is + - * /, sqrt, min / max in the Fortran text's order; with
// -ffp-contract=off every line rounds as the text does, and the header compiles for the host as
// well (tests/subex/subex_point.cpp holds it against a transcription of the Fortran, bit for bit).
#pragma once
#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "condtq.hpp"      // pfwsat, wlh, the constants and dmin / dmax
#include "fastmath.hpp"    // rcm_pow10, rcm_exp

namespace rcm {

namespace sx {
constexpr double LOWCLD = 0.0001, HICLD = 0.9999;        // Share/mod_constants.F90:371-372
constexpr double MINQC = 1.0e-10;                        // :58
constexpr double REGRAV = 1.0 / 9.80665;                 // :85, 182
constexpr double D_R1000 = 0.001;                        // :44
constexpr int NCHI = 256;                                // Main/mod_micro_interface.F90:56
// Main/microlib/mod_micro_subex.F90:53-57
constexpr double REMFRC = 0.0, PPTMIN = 0.0, ACTCLD = 0.0, ACCRFRC = 0.5;
}  // namespace sx

// the run's scalars: rhmax, rhmin (the clamps of subex_cldfrac and of the clear-sky humidity), tc0,
// larcticcorr, iconvlwp
struct SubexPar {
  double rhmax, rhmin, tc0;
  int larcticcorr, iconvlwp;
};

// chis(i), i = 0 .. nchi - 1 (allocate_micro, Main/mod_micro_interface.F90:117-120)
RCM_CQ_HD double subex_chis(int i) {
  const double cf = (double)i / (double)(sx::NCHI - 1);
  return 0.97 * rcm_exp(-((cf - 0.098) * (cf - 0.098)) / 0.0365) + 0.255;
}

// totc of ipptls = 1 with its floor (Main/mod_micro_interface.F90:241, 249)
RCM_CQ_HD double subex_totc(double qc) { return qc <= 1.0e-10 ? 0.0 : qc; }

// subex_cldfrac at one point (Main/cloudlib/mod_cloud_subex.F90:62-101) and cldfrac's clamp of it
// (Main/mod_micro_interface.F90:301).  qc is totc.
RCM_CQ_HD double subex_fcc(double t, double p, double qv, double qc, double rh, double rh0, const SubexPar& s) {
  double fcc;
  if (qc > 1.0e-7) {
    const double rhrng = cq::dmin(cq::dmax(rh, s.rhmin), s.rhmax);
    double rh0adj;
    if (t > s.tc0) rh0adj = rh0;
    else rh0adj = 0.99999 - (1.0 - rh0) / (1.0 + 0.15 * (s.tc0 - t));     // high cloud
    if (rhrng <= rh0adj) fcc = 0.0;
    else if (rhrng > 0.99999) fcc = 1.0;
    else fcc = 1.0 - sqrt((1.0 - rhrng) / (1.0 - rh0adj));                // Sundqvist (1989)
  } else {
    fcc = 0.0;
  }
  if (s.larcticcorr) {
    if (p >= 75000.0 && qv <= 0.003) fcc = fcc * cq::dmax(0.15, cq::dmin(1.0, qv / 0.003));
  }
  return cq::dmax(cq::dmin(fcc, sx::HICLD), 0.0);
}

// clwfromt (Share/clwfromt.inc), g/m3
RCM_CQ_HD double clwfromt(double t) {
  const double tcel = t - cq::TZERO;
  if (tcel < -50.0) return 0.001;
  return 0.127 + 6.78e-03 * tcel + 1.29e-04 * (tcel * tcel) + 8.68e-07 * (tcel * tcel * tcel);
}

// The merge of the large-scale and the convective cloud (Main/mod_micro_interface.F90:314-348) and
// rh0adj (:354-355).  cldfra / cldlwc come in as cucloud left them and go out merged; chis is the
// table of subex_chis.
RCM_CQ_HD void subex_cloud(double fcc, double totc, double t, double rho, double rh, const double* chis,
                           const SubexPar& s, double& cldfra, double& cldlwc, double& rh0adj) {
  double exlwc = 0.0;
  if (fcc > sx::LOWCLD) {
    if (s.iconvlwp == 1) {
      exlwc = clwfromt(t);
    } else {
      exlwc = (totc * 1000.0) * rho;
      exlwc = exlwc / fcc;
    }
    const int ichi = (int)(fcc * (double)(sx::NCHI - 1));
    exlwc = exlwc * chis[ichi];
  }
  if (cldfra > sx::LOWCLD) {
    cldlwc = (exlwc * fcc + cldlwc * cldfra) / (cldfra + fcc);
    cldfra = cq::dmax(cldfra, fcc);
  } else {
    cldfra = fcc;
    cldlwc = exlwc;
  }
  if (cldlwc > 0.0) cldfra = cq::dmin(cq::dmax(cldfra, 0.0), sx::HICLD);
  else cldfra = 0.0;
  rh0adj = 1.0 - (1.0 - rh) / ((1.0 - cldfra) * (1.0 - cldfra));
  rh0adj = cq::dmax(0.0, cq::dmin(rh0adj, 0.99999));
}

// qcth of Gultepe & Isaac (Main/microlib/mod_micro_subex.F90:161-163), the argument of the power
// and the threshold from the power's value (so a test can hand the transcription the same power)
RCM_CQ_HD double subex_qcth_arg(double t) { return -0.48911 + 0.01344 * (t - cq::TZERO); }
RCM_CQ_HD double subex_pow10(double x) { return rcm_pow10(x); }

// dqc of the non-aerosol branch (:156-170); qcth is 0 where the gate is closed
RCM_CQ_HD double subex_dqc(double afc, double qcw, double t, double cgul, double& qcth) {
  if (qcw > sx::MINQC && afc > sx::ACTCLD) {
    const double qcincl = qcw / afc;
    qcth = cgul * subex_pow10(subex_qcth_arg(t)) * sx::D_R1000;
    return cq::dmax(qcincl - qcth, 0.0);
  }
  qcth = 0.0;
  return 0.0;
}

// what one level of a rain column reads
struct SubexLevel {
  double afc, qcw, dqc, rho;      // fcc, qcn, dqc, rhob3d
  double t, p, qv, rh;            // tb3d, pb3d, qvn, rhb3d (levels 2 .. kz only)
  double pf, pfn;                 // pf3d of k and k + 1
};
// and the column's 2-D inputs
struct SubexColumn {
  double psb, qck1, cevap, caccr, dt;
};
// what one level writes: the three coupled increments (each the text's update of a zero tendency)
// and the cloud removal rate
struct SubexOut {
  double lsc_t, lsc_qv, lsc_qc, remrat;
};

// 1a. the top layer (:196-240); sets pptsum
RCM_CQ_HD void subex_rain_top(const SubexLevel& l, const SubexColumn& c, double& pptsum, SubexOut& o) {
  o.lsc_t = o.lsc_qv = o.lsc_qc = o.remrat = 0.0;
  pptsum = 0.0;
  const double afc = l.afc, qcw = l.qcw;
  double pptnew = 0.0;
  if (qcw > sx::MINQC && afc > sx::ACTCLD) {
    const double pptmax = (1.0 - sx::REMFRC) * qcw / c.dt;
    pptnew = cq::dmin(pptmax, c.qck1 * l.dqc * afc);
    const double qcleft = cq::dmax(qcw - pptnew * c.dt, 0.0);
    const double pptkm1 = sx::ACCRFRC * pptnew / afc * l.rho * c.dt;
    const double pptacc = c.caccr * qcleft * pptkm1;
    pptnew = cq::dmin(pptmax, pptacc + pptnew);
    if (pptnew > sx::PPTMIN) {
      const double dpovg = (l.pfn - l.pf) * sx::REGRAV;
      pptsum = pptnew * dpovg;
      o.lsc_qc = 0.0 - pptnew * c.psb;
      o.remrat = pptnew / qcw;
    }
  }
}

// 1b. a layer from the second to the surface (:252-345); updates pptsum
RCM_CQ_HD void subex_rain_level(const SubexLevel& l, const SubexColumn& c, const SubexPar& s, double& pptsum,
                                SubexOut& o) {
  o.lsc_t = o.lsc_qv = o.lsc_qc = o.remrat = 0.0;
  const double dpovg = (l.pfn - l.pf) * sx::REGRAV;
  const double afc = l.afc, qcw = l.qcw;
  double pptnew = 0.0, pptkm1;
  if (pptsum > 0.0) pptkm1 = pptsum / dpovg;
  else pptkm1 = 0.0;
  // 1bc. raindrop evaporation in the clear portion of the gridcell
  if (pptkm1 > sx::PPTMIN) {
    const double qs = pfwsat(l.t, l.p, cq::EP2);
    const double dqv = (qs - l.qv) / c.dt;
    if (dqv > 0.0) {
      double rhcs = (l.rh - afc * s.rhmax) / (1.0 - afc);
      rhcs = cq::dmax(cq::dmin(rhcs, s.rhmax), s.rhmin);
      double rdevap = c.cevap * (s.rhmax - rhcs) * sqrt(pptsum) * (1.0 - afc);
      rdevap = cq::dmin(rdevap, dqv);
      rdevap = cq::dmin(rdevap, pptkm1);
      if (rdevap > cq::DLOWVAL) {
        pptsum = cq::dmax(pptsum - rdevap * dpovg, 0.0);
        pptkm1 = pptkm1 - rdevap;
        o.lsc_qv = 0.0 + rdevap * c.psb;
        o.lsc_t = 0.0 - wlh(l.t) * cq::RCPD * rdevap * c.psb;
      }
    }
  }
  // 1bd. autoconversion and accretion
  if (qcw > sx::MINQC && afc > sx::ACTCLD) {
    const double pptmax = (1.0 - sx::REMFRC) * qcw / c.dt;
    pptnew = cq::dmin(pptmax, c.qck1 * l.dqc * afc);
    const double qcleft = cq::dmax(qcw - pptnew * c.dt, 0.0);
    pptkm1 = (pptkm1 + sx::ACCRFRC * pptnew / afc) * l.rho * c.dt;
    const double pptacc = c.caccr * qcleft * pptkm1;
    pptnew = cq::dmin(pptmax, pptacc + pptnew);
    if (pptnew > sx::PPTMIN) {
      pptsum = pptsum + pptnew * dpovg;
      o.lsc_qc = 0.0 - pptnew * c.psb;
      o.remrat = pptnew / qcw;
    }
  }
}

// one term of rembc's kk loop (:369-371)
RCM_CQ_HD double subex_rembc_term(double remrat_kk, double qcw, double pf, double pfn) {
  return remrat_kk * qcw * (pfn - pf) * sx::REGRAV;
}

// 3. the surface (:386-391): whether the column's rain passes the gate, and prainx
RCM_CQ_HD bool subex_surface(double pptsum, double dtsec, double& prainx) {
  prainx = pptsum * dtsec;
  return prainx > cq::DLOWVAL;
}

}  // namespace rcm

#if defined(__HIP__) || defined(__HIPCC__)
#include "engine.hpp"

namespace rcm {

// argument block of the kernels of subex.hip: the mkslice fields and p*b, the host's 2-D tables and
// cucloud's output, the chis table, and what the kernels write (remrat / rembc null with rem off)
struct SubexArgs {
  const double *tb, *qv, *qc, *pb, *pf, *rho, *rh, *psb;
  const double *rh0, *qck1, *cgul, *cevap, *caccr, *cufra, *culwc, *chis;
  double *fcc, *cldfra, *cldlwc, *rh0adj, *dqc;
  double *lsc_t, *lsc_qv, *lsc_qc, *rainnc, *lsmrnc, *trrate, *remrat, *rembc;
  SubexPar par;
  double dtsec;
};

constexpr int SBX_COLW = 64;       // columns of one block of k_subex_column: one wavefront along j

__global__ void k_subex_point(Geom g, int kz, SubexArgs a);
__global__ void k_subex_column(Geom g, int kz, const StepState* __restrict__ ds, SubexArgs a);
// out = phy + lsc (phy null: never launched) over n doubles, for the three physics sums at once
__global__ void k_subex_sums(long n, const double* tphy, const double* qvphy, const double* qcphy, const double* lt,
                             const double* lqv, const double* lqc, double* st, double* sqv, double* sqc);

}  // namespace rcm
#endif
