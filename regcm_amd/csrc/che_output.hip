// che_output.hip -- the CHE stream's tracer fields, formed on the device (enum rcmdyn_che_field,
// include/rcmdyn.h): fill_chem_outvars' mixing ratio, column burden and the five ichdiag terms the
// dyn core accumulates (Main/chemlib/mod_che_output.F90:74-83, 131-184, the idynamic /= 3 branch).
//
// One launch per tile and call: lanes along j, CHE_ROWS rows of i per block, (tracer of the batch,
// level) on blockIdx.z.  A thread loads psb once and per requested kz-level field does one load,
// one fp64 division and one store; the requested set is a bit mask in the argument block
// (wave-uniform: an unrequested field costs no load).  With the tracer budget on (a.acc) every one
// of the five sums at the thread's point is zeroed in the same pass, requested or not: the
// reference zeroes c*diag(:,:,:,itr) whenever ichdiag > 0.  The blocks of level 1 also walk the
// column for the burden (dtrace, Main/chemlib/mod_che_tend.F90:561-571): the loads of CK levels are
// issued together, the sum adds one level after the other in k order, each term
// chib3d * dzq * rhob3d left to right (-ffp-contract=off).  A value is rounded once, (T) of the
// finished double, when it is stored.
#include "che_output.hpp"
#include "devcommon.hpp"

namespace rcm {

namespace {
constexpr int CHE_ROWS = 4;
// the accumulator term behind a budget field
constexpr int CHE_TERM0 = RCMDYN_CHE_ADVH;
static_assert(RCMDYN_CHE_ADVH - CHE_TERM0 == RCMDYN_TRDIAG_ADVH && RCMDYN_CHE_ADVV - CHE_TERM0 == RCMDYN_TRDIAG_ADVV &&
              RCMDYN_CHE_BDY - CHE_TERM0 == RCMDYN_TRDIAG_BDY && RCMDYN_CHE_DIFH - CHE_TERM0 == RCMDYN_TRDIAG_DIFH &&
              RCMDYN_CHE_CONV - CHE_TERM0 == RCMDYN_TRDIAG_CONV && RCMDYN_NCHE - CHE_TERM0 == RCMDYN_NTRDIAG,
              "the budget fields follow rcmdyn_tracer_diag's order");
}  // namespace

template <class T>
__global__ __launch_bounds__(64 * CHE_ROWS) void k_output_che(Geom g, int kz, CheArgs a) {
  const int j = g.jci1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ici1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int b = (int)blockIdx.z / kz, k = (int)blockIdx.z % kz + 1;
  if (j > g.jci2 || i > g.ici2 || b >= a.nb) return;
  const int n = a.itr0 + b;
  const unsigned m = a.mask;
  const long ncj = g.jci2 - g.jci1 + 1, nci = g.ici2 - g.ici1 + 1;
  const long p2 = (long)(i - g.ici1) * ncj + (j - g.jci1);       // the point in a compact plane
  const long p3 = (long)(k - 1) * ncj * nci + p2;
  T* const out = (T*)a.out + (long)b * a.stride;
  auto has = [m](int f) { return (m >> f) & 1u; };
  const double psb = F2(a.psb, j, i);                             // cpsb, Main/mod_che_interface.F90:128

  if (has(RCMDYN_CHE_MIXRAT))                                     // Main/chemlib/mod_che_output.F90:76-77
    out[a.off[RCMDYN_CHE_MIXRAT] + p3] = (T)(F3(a.tab[n / NQXH].a1[n % NQXH], j, i, k) / psb);
  if (a.acc) {                                                    // :131-158, 178-184
#pragma unroll
    for (int t = 0; t < RCMDYN_NTRDIAG; t++) {
      double* const acc = a.acc[t * a.ntr + n];
      if (has(CHE_TERM0 + t)) out[a.off[CHE_TERM0 + t] + p3] = (T)(F3(acc, j, i, k) / psb);
      F3(acc, j, i, k) = d_zero;
    }
  }
  if (k != 1 || !has(RCMDYN_CHE_BURDEN)) return;
  const double* const chib = a.chib3d[n];
  constexpr int CK = 4;
  double dtrace = d_zero;
  for (int k0 = 1; k0 <= kz; k0 += CK) {
    double vc[CK], vz[CK], vr[CK];
#pragma unroll
    for (int u = 0; u < CK; u++) {                                // levels past kz load level kz and are not used
      const int kk = k0 + u <= kz ? k0 + u : kz;
      vc[u] = F3(chib, j, i, kk);
      vr[u] = F3(a.rhob3d, j, i, kk);
      vz[u] = a.dzq ? F3(a.dzq, j, i, kk) : F3(a.zf0, j, i, kk) - F3(a.zf0, j, i, kk + 1);
    }
#pragma unroll
    for (int u = 0; u < CK; u++) {
      if (k0 + u > kz) break;
      dtrace = dtrace + vc[u] * vz[u] * vr[u];                    // Main/chemlib/mod_che_tend.F90:566-567
    }
  }
  out[a.off[RCMDYN_CHE_BURDEN] + p2] = (T)(dtrace * 1.0e6);       // Main/chemlib/mod_che_output.F90:82
}

template __global__ void k_output_che<double>(Geom, int, CheArgs);
template __global__ void k_output_che<float>(Geom, int, CheArgs);

}  // namespace rcm
