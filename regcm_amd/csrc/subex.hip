// subex.hip -- the SUBEX cloud fraction and rain columns on the device (subex.hpp has the
// statements; rcmdyn_set_subex).
//
// k_subex_point: cldfrac with subex_cldfrac and the dqc loop of subex, one thread per interior cross
// point and level, laid out as k_slice's launch.  k_subex_column: the rain column of subex, one lane
// per column with the lanes of a wavefront adjacent in j (every load and store is one coalesced
// row segment), pptsum in a register.  The chain of a level is a few dozen flops, two divisions and
// a sqrt, and a grid has few wavefronts to hide it behind, so the loads of level k + 1 are issued
// before the dependent arithmetic of level k, and a block is one wavefront, which spreads a grid's
// rows over the most compute units.  k_subex_sums: the physics sums the tendency kernels read.
#include "subex.hpp"
#include "devcommon.hpp"

namespace rcm {

__global__ __launch_bounds__(256) void k_subex_point(Geom g, int kz, SubexArgs a) {
  const int j = g.jci1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ici1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int k = (int)blockIdx.z + 1;
  if (j > g.jci2 || i > g.ici2 || k > kz) return;
  const long o2 = g.ix(j, i), o = (long)(k - 1) * g.plane + o2;
  const double t = a.tb[o], qcn = a.qc[o], rh = a.rh[o];
  const double totc = subex_totc(qcn);
  const double fcc = subex_fcc(t, a.pb[o], a.qv[o], totc, rh, a.rh0[o2], a.par);
  double cldfra = a.cufra[o], cldlwc = a.culwc[o], rh0adj;
  subex_cloud(fcc, totc, t, a.rho[o], rh, a.chis, a.par, cldfra, cldlwc, rh0adj);
  double qcth;
  a.dqc[o] = subex_dqc(fcc, qcn, t, a.cgul[o2], qcth);
  a.fcc[o] = fcc;
  a.cldfra[o] = cldfra;
  a.cldlwc[o] = cldlwc;
  a.rh0adj[o] = rh0adj;
}

namespace {

// level k of the column at frame offset o2; pf of k comes from the level above (its pfn)
__device__ __forceinline__ SubexLevel load_level(const Geom& g, const SubexArgs& a, long o2, int k, double pf) {
  const long o = (long)(k - 1) * g.plane + o2;
  SubexLevel l;
  l.afc = a.fcc[o]; l.qcw = a.qc[o]; l.dqc = a.dqc[o]; l.rho = a.rho[o];
  l.t = a.tb[o]; l.p = a.pb[o]; l.qv = a.qv[o]; l.rh = a.rh[o];
  l.pf = pf; l.pfn = a.pf[o + g.plane];
  return l;
}

}  // namespace

// dynamic LDS: kz x SBX_COLW doubles with rem on (the column's remrat for rembc's kk loop), else none
__global__ __launch_bounds__(SBX_COLW) void k_subex_column(Geom g, int kz, const StepState* __restrict__ ds, SubexArgs a) {
  extern __shared__ double remr[];
  const int lane = (int)threadIdx.x;
  const int j = g.jci1 + (int)blockIdx.x * SBX_COLW + lane;
  const int i = g.ici1 + (int)blockIdx.y;
  if (j > g.jci2 || i > g.ici2) return;
  const long o2 = g.ix(j, i);
  const bool rem = a.remrat != nullptr;
  SubexColumn c;
  c.psb = a.psb[o2]; c.qck1 = a.qck1[o2]; c.cevap = a.cevap[o2]; c.caccr = a.caccr[o2]; c.dt = ds->dt;
  double pptsum = 0.0;
  SubexLevel cur = load_level(g, a, o2, 1, a.pf[o2]);
  for (int k = 1; k <= kz; k++) {
    SubexLevel nxt = cur;
    if (k < kz) nxt = load_level(g, a, o2, k + 1, cur.pfn);      // in flight under level k's chain
    SubexOut w;
    if (k == 1) subex_rain_top(cur, c, pptsum, w);
    else subex_rain_level(cur, c, a.par, pptsum, w);
    const long o = (long)(k - 1) * g.plane + o2;
    a.lsc_t[o] = w.lsc_t;
    a.lsc_qv[o] = w.lsc_qv;
    a.lsc_qc[o] = w.lsc_qc;
    if (rem) {
      // 2. the below-cloud removal (:359-373), the kk sum in the text's order
      double rembc = 0.0;
      if (k >= 2 && w.remrat > 0.0)
        for (int kk = 1; kk <= k - 1; kk++)
          rembc = rembc + subex_rembc_term(remr[(kk - 1) * SBX_COLW + lane], cur.qcw, cur.pf, cur.pfn);
      remr[(k - 1) * SBX_COLW + lane] = w.remrat;
      a.remrat[o] = w.remrat;
      a.rembc[o] = rembc;
    }
    cur = nxt;
  }
  double prainx;
  if (subex_surface(pptsum, a.dtsec, prainx)) {
    a.rainnc[o2] = a.rainnc[o2] + prainx;
    a.lsmrnc[o2] = a.lsmrnc[o2] + pptsum;
    a.trrate[o2] = pptsum;
  }
}

__global__ __launch_bounds__(256) void k_subex_sums(long n, const double* tphy, const double* qvphy, const double* qcphy,
                                                    const double* lt, const double* lqv, const double* lqc, double* st,
                                                    double* sqv, double* sqc) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  st[q] = tphy[q] + lt[q];
  sqv[q] = qvphy[q] + lqv[q];
  sqc[q] = qcphy[q] + lqc[q];
}

}  // namespace rcm
