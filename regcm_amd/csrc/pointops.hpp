// pointops.hpp -- the per-point formulas the three cores share, each stated once: the
// hydrostatic kernels (kernels.hip), the non-hydrostatic ones (kernels_nh.hip) and the
// hydrometeors of nqx = 5 (species.hip) call these with their own way of loading the operands.
// Every body keeps the reference's floating-point operation order (-ffp-contract=off).
#pragma once
#include "devcommon.hpp"
#include "optset.hpp"

namespace rcm {

// How a kernel reads a model option: every read of iboudy, idiffu, ipgf, isladvec and every
// test of an optional pointer of Fields (the exports tten .. xkcs, the seam's physics
// tendencies, kpbl) in the hydrostatic tendency kernels goes through a policy.  OptGeneric
// reads Consts and tests the pointer (any option, the code as it always was); OptDefault
// returns the constants of the default set and ignores its argument, so the compiler drops the
// code, pointers and registers of the alternatives.  The host picks the instance per launch
// (optset.hpp).  The non-hydrostatic kernels and the hydrometeors use OptGeneric.
struct OptGeneric {
  static __device__ __forceinline__ int iboudy(const Consts* c) { return c->iboudy; }
  static __device__ __forceinline__ int idiffu(const Consts* c) { return c->idiffu; }
  static __device__ __forceinline__ int ipgf(const Consts* c) { return c->ipgf; }
  static __device__ __forceinline__ int isladvec(const Consts* c) { return c->isladvec; }
  template <class T>
  static __device__ __forceinline__ bool has(const T* p) { return p != nullptr; }
};
struct OptDefault {
  static __device__ __forceinline__ int iboudy(const Consts*) { return OPT_IBOUDY; }
  static __device__ __forceinline__ int idiffu(const Consts*) { return OPT_IDIFFU; }
  static __device__ __forceinline__ int ipgf(const Consts*) { return OPT_IPGF; }
  static __device__ __forceinline__ int isladvec(const Consts*) { return OPT_ISLADVEC; }
  template <class T>
  static __device__ __forceinline__ bool has(const T*) { return false; }
};

// boundary relaxation contribution (nudge*, Main/mod_bdycod.F90:4262-4263): f0 the boundary
// data minus the state at the point, f1..f4 at its west, east, south and north neighbours
__device__ __forceinline__ double relax(double ften, double xf, double xg, double f0, double f1, double f2,
                                        double f3, double f4) {
  return ften + xf * f0 - xg * (f1 + f2 + f3 + f4 - d_four * f0);
}
// its operand: the boundary data at time xt of the interval minus the state a
__device__ __forceinline__ double bdy_minus_state(double b0, double bt, double a, double xt) {
  return (b0 + xt * bt) - a;
}
// the same on qv, both terms scaled by nfac first (nudge4d3d, Main/mod_bdycod.F90:4512-4532)
__device__ __forceinline__ double bdy_minus_state(double b0, double bt, double a, double xt, double nfac) {
  return nfac * (b0 + xt * bt) - nfac * a;
}

// upstream flux-form advection of one scalar (hadvt/hadvqv/hadvqx/hadv3d ind 0,
// Main/mod_advection.F90:337-386, 466-480, 547-596, 639-653) from the cell's mass fluxes and
// the advected field at the point (fc) and its west/east/south/north neighbours; limiter 0
// none, 1 t_extrema, 2 q_rel_extrema
__device__ __forceinline__ double hadv_flux(const Consts* c, double xm, double ps, double uavg1, double uavg2,
                                            double vavg1, double vavg2, double fc, double fw, double fe, double fs,
                                            double fn, int limiter) {
  const double ul = c->ul;
  const double f1 = d_half * ul * (uavg2 + uavg1) / ps;
  const double f2 = d_half * ul * (vavg2 + vavg1) / ps;
  const double fx1 = (d_one + f1) * fw + (d_one - f1) * fc;
  const double fx2 = (d_one + f1) * fc + (d_one - f1) * fe;
  const double fy1 = (d_one + f2) * fs + (d_one - f2) * fc;
  const double fy2 = (d_one + f2) * fc + (d_one - f2) * fn;
  double fg = -xm * (uavg2 * fx2 - uavg1 * fx1 + vavg2 * fy2 - vavg1 * fy1);
  if (limiter && c->stability_enhance) {
    double den, thr;
    if (limiter == 1) { den = ps; thr = c->t_extrema; } else { den = dmax(fc, DLOWVAL); thr = c->q_rel_extrema; }
    if (fabs(fn + fs - d_two * fc) / den > thr) {
      if (fc > fn && fc > fs) fg = dmin(fg, d_zero);
      else if (fc < fn && fc < fs) fg = dmax(fg, d_zero);
    }
    if (fabs(fe + fw - d_two * fc) / den > thr) {
      if (fc > fe && fc > fw) fg = dmin(fg, d_zero);
      else if (fc < fe && fc < fw) fg = dmax(fg, d_zero);
    }
  }
  return fg;
}

// time filters of one point (Main/mod_tendency.F90:420-427, Main/mod_timefilter.F90): o1, o2
// atm1, atm2 before the filter, v the forecast (qv, qc: fixed where negative), n1, n2 atm1, atm2
// after it.  RA of t; RAW of qv (gnu1, floors MINQQ * the filtered p* pa, pb) and of qc and the
// hydrometeors (gnu2, zero floor)
static constexpr double raw_beta = 0.53;
__device__ __forceinline__ void ra_t(const Consts* c, double o1, double o2, double v, double& n1, double& n2) {
  const double d = c->gnu1 * (v + o2 - d_two * o1);
  n2 = o1 + d;
  n1 = v;
}
__device__ __forceinline__ void raw_qv(const Consts* c, double o1, double o2, double v, double pa, double pb,
                                       double& n1, double& n2) {
  const double beta = raw_beta;
  const double d = c->gnu1 * (v + o2 - d_two * o1);
  n2 = dmax(o1 + beta * d, MINQQ * pa);
  n1 = dmax(v + (beta - d_one) * d, MINQQ * pb);
}
__device__ __forceinline__ void raw_qc(const Consts* c, double o1, double o2, double v, double& n1, double& n2) {
  const double beta = raw_beta;
  const double d = c->gnu2 * (v + o2 - d_two * o1);
  double m = o1 + beta * d, q = v + (beta - d_one) * d;
  if (m < d_zero) m = d_zero;
  if (q < d_zero) q = d_zero;
  n2 = m;
  n1 = q;
}
// species n = 0 (qv) or 1 (qc) by a run-time n
__device__ __forceinline__ void raw_filter(const Consts* c, int n, double v, double o1, double o2, double pa,
                                           double pb, double& n1, double& n2) {
  if (n == 0) raw_qv(c, o1, o2, v, pa, pb, n1, n2);
  else raw_qc(c, o1, o2, v, n1, n2);
}

// diffu_x at one cross point (diffu_x3d / diffu_x3df / diffu_x4d3d, Main/mod_diffusion.F90:
// 523-790): idiffu = 2 the 9-point scheme, idiffu = 1 the fourth-order one on the points two
// or more from the domain's edge plus the second-order adds of the first interior lines (west,
// east, south, north).  f(dj, di) reads the decoupled field at (j + dj, i + di), xk is the
// scaled coefficient.  The index tests are the global ones, so they hold on ghost-ring points
// too (equal to the tile ranges on owned points, engine.hpp).  The idiffu = 3 column term
// stays with the callers.  O: the option policy (idiffu).
template <class O = OptGeneric, class F>
__device__ __forceinline__ double diffu_x(const Geom& g, const Consts* __restrict__ c, int j, int i, double ften,
                                          double xk, F f) {
  if (O::idiffu(c) == 2)
    return ften + d_one * xk *
                      (o4_c1 * (f(1, 0) + f(-1, 0) + f(0, 1) + f(0, -1)) +
                       o4_c2 * (f(1, 1) + f(-1, -1) + f(-1, 1) + f(1, -1)) + o4_c3 * f(0, 0));
  if (g.gcii(j, i))
    ften = ften - d_one * xk *
                      (z4_c1 * (f(2, 0) + f(-2, 0) + f(0, 2) + f(0, -2)) +
                       z4_c2 * (f(1, 0) + f(-1, 0) + f(0, 1) + f(0, -1)) + z4_c3 * f(0, 0));
  auto lap = [&](double x) {
    return x + d_one * xk * (z4_c1 * (f(1, 0) + f(-1, 0) + f(0, 1) + f(0, -1)) + z4_c2 * f(0, 0));
  };
  if (g.gjeq(j, 2)) ften = lap(ften);
  if (g.gjeq(j, g.gjx - 2)) ften = lap(ften);
  if (g.gieq(i, 2)) ften = lap(ften);
  if (g.gieq(i, g.giy - 2)) ften = lap(ften);
  return ften;
}

// decoupled ud, vd of one dot point with the inflow/outflow rule of iboudy = 3/4 on the global
// boundary lines (Main/mod_tendency.F90:893-994): an outflow boundary point takes the adjacent
// interior value.  W/E run on the idi columns first, then S/N on the full jde rows, so a corner
// row point copies the (possibly already replaced) W/E value.  The slice values the reference
// multiplies (wui, wue, ...) equal atm1 there (bdyuv), so the default is atm1 * rpsda.  A ghost
// point on a boundary line carries the value its owner computes and the reference exchanges.
// u(jj, ii), v(jj, ii), r(jj, ii) load atm1 u, v and 1/p*dot at the caller's level.
template <class U, class V, class R>
__device__ __forceinline__ double2 udvd_rule(const Geom& g, int j, int i, U u, V v, R r) {
  auto base = [&](int jj, int ii) {
    const double rr = r(jj, ii);
    return make_double2(u(jj, ii) * rr, v(jj, ii) * rr);
  };
  auto we = [&](int jj, int ii) {
    if (in(ii, 2, g.giy - 1)) {
      if (g.gjeq(jj, 1) && u(jj, ii) <= d_zero) return base(2, ii);
      if (g.gjeq(jj, g.gjx) && u(jj, ii) >= d_zero) return base(g.gjx - 1, ii);
    }
    return base(jj, ii);
  };
  if (g.band || in(j, 1, g.gjx)) {
    if (g.gieq(i, 1) && v(j, i) >= d_zero) return we(j, 2);
    if (g.gieq(i, g.giy) && v(j, i) <= d_zero) return we(j, g.giy - 1);
  }
  return we(j, i);
}

// a word of the negative-forecast list (k_scalars, k_nh_tend_c: 2 * the element's index in
// its 3-D field + the species) as species n and point (j, i, k)
__device__ __forceinline__ void negfix_entry(const Geom& g, uint32_t w, int& n, int& k, int& j, int& i) {
  n = (int)(w & 1u);
  const long el = (long)(w >> 1);
  k = (int)(el / g.plane) + 1;
  const long r = el % g.plane;
  i = g.i0 + (int)(r / g.pitch);
  j = g.j0 + (int)(r % g.pitch);
}

// splitf's deld / delh: slot s (1..3) of vertical mode l (1..nsplit), planes of `plane` doubles
template <class T>
__device__ __forceinline__ T* split_slot(T* base, long plane, int nsplit, int l, int s) {
  return base + ((long)(s - 1) * nsplit + (l - 1)) * plane;
}

}  // namespace rcm
