// subex_point.cpp -- the per-point statements of regcm_amd/csrc/subex.hpp on the host, as a small
// shared library over arrays, so tests/test_subex_cpu.py can hold the header to a transcription of
// the Fortran bit for bit and the GPU tests can hand that transcription the header's own 10**x and
// chis table.  Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC.
#include <vector>

#include "../../regcm_amd/csrc/subex.hpp"

using namespace rcm;

extern "C" {

void sx_chis(double* out) {
  for (int i = 0; i < sx::NCHI; i++) out[i] = subex_chis(i);
}

void sx_pow10(long n, const double* x, double* out) {
  for (long q = 0; q < n; q++) out[q] = subex_pow10(x[q]);
}

// cldfrac with subex_cldfrac and subex's dqc at n points; par: rhmax, rhmin, tc0, larcticcorr, iconvlwp
void sx_point(long n, const double* par, const double* chis, const double* t, const double* p, const double* qv,
              const double* qc, const double* rh, const double* rho, const double* rh0, const double* cgul,
              const double* cufra, const double* culwc, double* fcc, double* cldfra, double* cldlwc, double* rh0adj,
              double* dqc, double* qcth) {
  const SubexPar s{par[0], par[1], par[2], (int)par[3], (int)par[4]};
  for (long q = 0; q < n; q++) {
    const double totc = subex_totc(qc[q]);
    fcc[q] = subex_fcc(t[q], p[q], qv[q], totc, rh[q], rh0[q], s);
    cldfra[q] = cufra[q];
    cldlwc[q] = culwc[q];
    subex_cloud(fcc[q], totc, t[q], rho[q], rh[q], chis, s, cldfra[q], cldlwc[q], rh0adj[q]);
    dqc[q] = subex_dqc(fcc[q], qc[q], t[q], cgul[q], qcth[q]);
  }
}

// the rain columns: 3-D arrays [k][col] (pf: kz + 1 levels), 2-D [col]; rem: also remrat / rembc
void sx_columns(long ncol, int kz, const double* par, double dt, double dtsec, int rem, const double* fcc,
                const double* dqc, const double* t, const double* p, const double* pf, const double* qv,
                const double* qc, const double* rh, const double* rho, const double* psb, const double* qck1,
                const double* cevap, const double* caccr, double* lsc_t, double* lsc_qv, double* lsc_qc, double* rainnc,
                double* lsmrnc, double* trrate, double* remrat, double* rembc, double* pptsum_out) {
  const SubexPar s{par[0], par[1], par[2], (int)par[3], (int)par[4]};
  std::vector<double> remr(kz);
  for (long c = 0; c < ncol; c++) {
    const SubexColumn col{psb[c], qck1[c], cevap[c], caccr[c], dt};
    double pptsum = 0.0;
    for (int k = 1; k <= kz; k++) {
      const long o = (long)(k - 1) * ncol + c;
      const SubexLevel l{fcc[o], qc[o], dqc[o], rho[o], t[o], p[o], qv[o], rh[o], pf[o], pf[o + ncol]};
      SubexOut w;
      if (k == 1) subex_rain_top(l, col, pptsum, w);
      else subex_rain_level(l, col, s, pptsum, w);
      lsc_t[o] = w.lsc_t; lsc_qv[o] = w.lsc_qv; lsc_qc[o] = w.lsc_qc;
      if (rem) {
        double rb = 0.0;
        if (k >= 2 && w.remrat > 0.0)
          for (int kk = 1; kk <= k - 1; kk++) rb = rb + subex_rembc_term(remr[kk - 1], l.qcw, l.pf, l.pfn);
        remr[k - 1] = w.remrat;
        remrat[o] = w.remrat;
        rembc[o] = rb;
      }
    }
    pptsum_out[c] = pptsum;
    double prainx;
    if (subex_surface(pptsum, dtsec, prainx)) {
      rainnc[c] = rainnc[c] + prainx;
      lsmrnc[c] = lsmrnc[c] + pptsum;
      trrate[c] = pptsum;
    }
  }
}

}  // extern "C"
