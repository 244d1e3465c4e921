// condtq.hpp -- the SUBEX one-step condensation / evaporation adjustment with partial cloud
// cover (condtq, Main/mod_micro_interface.F90:382-493, the idynamic /= 3 branch), stated once per
// point for the hydrostatic scalars block (kernels.hip) and k_nh_tend_c (kernels_nh.hip), with the
// two functions it calls: pfwsat (Share/pfesat.inc, Share/pfwsat.inc; k_slice's ATMS_QSB3D uses
// the same copy) and wlh (Share/wlh.inc).
//
// No transcendental function: the Flatau polynomial, a cubic, + - * /, sqrt, min / max.  With
// -ffp-contract=off every line rounds as the Fortran text does, and the header compiles for the
// host as well (tests/condtq/condtq_point.cpp holds it against a transcription of the Fortran,
// bit for bit).
#pragma once
#include <cmath>

#if defined(__HIP__) || defined(__HIPCC__)
#define RCM_CQ_HD __host__ __device__ __forceinline__
#else
#define RCM_CQ_HD inline
#endif

namespace rcm {

namespace cq {
constexpr double TZERO = 273.15;                        // Share/mod_constants.F90:197
constexpr double MINQQ = 1.0e-8, DLOWVAL = 1.0e-20;     // :57, :68
constexpr double AMD = 28.96454, AMW = 18.01528;        // :107, :109
constexpr double RGASMOL = 6.02214129e23 * 1.3806504e-23;   // navgdr * boltzk, :130
constexpr double RWAT = (RGASMOL / AMW) * 1000.0;       // :137
constexpr double CPD = 3.5 * ((RGASMOL / AMD) * 1000.0);    // 3.5 * rgas, :132-144
constexpr double RCPD = 1.0 / CPD;                      // :183
constexpr double EP2 = AMW / AMD;                       // :306
constexpr double RHMAX = 0.99999;                       // the upper clamp of rh0adj (cldfrac, :355)
RCM_CQ_HD double dmax(double a, double b) { return (a > b) ? a : (b > a ? b : a); }
RCM_CQ_HD double dmin(double a, double b) { return (a < b) ? a : (b < a ? b : a); }
}  // namespace cq

// pfesat / pfwsat (Flatau et al. 1992 polynomials): saturation mixing ratio, kg/kg
RCM_CQ_HD double pfwsat(double t, double p, double ep2) {
  double tl = t - cq::TZERO;
  if (tl > 100.0) tl = 100.0;
  if (tl < -75.0) tl = -75.0;
  const double td = tl;
  double esat;
  if (td >= 0.0)
    esat = 6.11213476 + td * (0.444007856 + td * (0.143064234e-01 + td * (0.264461437e-03 + td * (0.305903558e-05 +
           td * (0.196237241e-07 + td * (0.892344772e-10 + td * (-0.373208410e-12 + td * 0.209339997e-15)))))));
  else
    esat = 6.11123516 + td * (0.503109514 + td * (0.188369801e-01 + td * (0.420547422e-03 + td * (0.614396778e-05 +
           td * (0.602780717e-07 + td * (0.387940929e-09 + td * (0.149436277e-11 + td * 0.262655803e-14)))))));
  const double es = esat * 100.0;
  return ep2 * (es / (p - es));
}

// wlh: latent heat of condensation / sublimation, J/kg (Rogers & Yau cubic above 0 C)
RCM_CQ_HD double wlh(double t) {
  const double tc = t - cq::TZERO;
  double lheat;
  if (tc > 0.0)
    lheat = 2500.79 - 2.36418 * tc + 1.58927e-3 * tc * tc - 6.14342e-5 * tc * tc * tc;
  else
    lheat = 2834.1 - 0.29 * tc - 0.004 * tc * tc;
  return lheat * 1.0e3;
}

// The adjustment at one point (:407-482).  t2, qv2, qc2: atm2 t, qv, qc (coupled with p*);
// tt, tqv, tqc: the step's total tendencies of the three (aten pc_total); psc: the new p*; pres:
// the pressure at tau + 1 (Pa); qs: atms%qsb3d of the step's start (mo2mc%qs; the mc2mo%qxten term
// of qvc_cld is zero, Main/mod_tendency.F90:341-343); rh0adj: cldfrac's adjusted threshold; conf:
// subexparam's condensation efficiency.  Gives tmp2 (1/s) and wwlh (J/kg).
RCM_CQ_HD void condtq_point(double t2, double qv2, double qc2, double tt, double tqv, double tqc, double psc,
                            double pres, double qs, double rh0adj, double dt, double conf, double& tmp2,
                            double& wwlh) {
  const double tmp3 = (t2 + dt * tt) / psc;
  double qvcs = qv2 + dt * tqv;
  double qccs = qc2 + dt * tqc;
  const double qvc_cld = cq::dmax(qs, 0.0);
  if (qvcs < cq::MINQQ * psc) qvcs = cq::MINQQ * psc;
  if (qccs < cq::DLOWVAL * psc) qccs = 0.0;
  qvcs = qvcs / psc;
  qccs = qccs / psc;
  // 2a. saturation mixing ratio and relative humidity at tau + 1
  const double qvs = pfwsat(tmp3, pres, cq::EP2);
  wwlh = wlh(tmp3);
  const double r1 = 1.0 / (1.0 + wwlh * wwlh * qvs / (cq::RWAT * cq::CPD * tmp3 * tmp3));
  const double rhc = cq::dmin(cq::dmax(qvcs / qvs, 0.0), 1.0);
  // 2b. low cover, high cover, partial cover
  double dqv;
  if (rhc < rh0adj) {
    dqv = conf * (qvcs - qvs);
  } else if (rhc > cq::RHMAX) {
    dqv = conf * (qvcs - qvs);
  } else {
    double fccc = 1.0 - sqrt((1.0 - rhc) / (1.0 - rh0adj));
    fccc = cq::dmin(cq::dmax(fccc, 0.0), 1.0);
    dqv = conf * fccc * (qvc_cld - qvs);
  }
  // 2c, 2d. the vapour in excess of saturation; the new cloud water + the old
  const double tmp1 = r1 * dqv;
  const double exces = qccs + tmp1;
  if (exces >= 0.0) tmp2 = tmp1 / dt;      // some cloud is left
  else tmp2 = -qccs / dt;                  // the cloud evaporates
}

// 3. the coupled increments of aten pc_physic (:475-480), zero where |tmp2| <= dlowval
RCM_CQ_HD void condtq_increments(double psc, double tmp2, double wwlh, double& dt_, double& dqv, double& dqc) {
  if (fabs(tmp2) > cq::DLOWVAL) {
    dqv = 0.0 - psc * tmp2;
    dqc = 0.0 + psc * tmp2;
    dt_ = 0.0 + psc * tmp2 * wwlh * cq::RCPD;
  } else {
    dt_ = dqv = dqc = 0.0;
  }
}

}  // namespace rcm
