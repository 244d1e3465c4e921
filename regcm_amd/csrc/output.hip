// output.hip -- the output stream's fields, formed on the device (enum rcmdyn_output_field,
// include/rcmdyn.h): the dyn-owned variables of the ATM stream and the dyn-owned parts of SRF / SHF
// that mod_output decouples from the coupled state every atmfrq / srffrq (Main/mod_output.F90:
// 224-660, 923-1154).
//
// One launch per tile and call: lanes along j, OUT_ROWS rows of i per block, one level per
// blockIdx.z; a thread forms every requested kz-level field at its (j, i, k) and, on the first
// level's blocks, the 2-D fields and the 100 m winds' walk up its column.  The requested set is a
// bit mask in the argument block (wave-uniform: an unrequested field costs no load).  Every
// expression is the reference's in its order (-ffp-contract=off), the log is the device libm's,
// pfwsat is condtq.hpp's; a value is rounded once, (T) of the finished double, when it is stored.
// Stores go to the tile's compact buffer over jci1:jci2 x ici1:ici2, j fastest.
#include "output.hpp"
#include "condtq.hpp"      // pfwsat (Share/pfesat.inc, Share/pfwsat.inc)

namespace rcm {

namespace {

constexpr double EGRAV_O = 9.80665;           // Share/mod_constants.F90:85
constexpr double d_10 = 10.0, d_100 = 100.0;
constexpr int OUT_ROWS = 4;

}  // namespace

template <class T>
__global__ __launch_bounds__(64 * OUT_ROWS) void k_output(Geom g, const Consts* __restrict__ c, OutArgs a) {
  const int j = g.jci1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = g.ici1 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int k = (int)blockIdx.z + 1;
  if (j > g.jci2 || i > g.ici2) return;
  const int kz = c->kz;
  const bool nh = c->idynamic == 2;
  const unsigned m = a.mask;
  const long ncj = g.jci2 - g.jci1 + 1, nci = g.ici2 - g.ici1 + 1;
  const long p2 = (long)(i - g.ici1) * ncj + (j - g.jci1);       // the point in a compact plane
  const long p3 = (long)(k - 1) * ncj * nci + p2;
  T* const out = (T*)a.out;
  auto has = [m](int f) { return (m >> f) & 1u; };
  auto put3 = [&](int f, double v) { out[a.off[f] + p3] = (T)v; };
  auto put2 = [&](int f, double v) { out[a.off[f] + p2] = (T)v; };
  const double ptop = c->ptop, rovg = c->rgas / EGRAV_O, ep1 = c->ep1;
  const double ps = F2(a.psa, j, i);                              // ps_out, :226
  // the four-point dot -> cross mean of a coupled wind over p* (:255-258, 1063-1065)
#define XWIND(U, K) (d_rfour * (F3(U, j, i, K) + F3(U, j + 1, i, K) + F3(U, j, i + 1, K) + F3(U, j + 1, i + 1, K)) / ps)

  if (has(RCMDYN_OUT_T)) put3(RCMDYN_OUT_T, F3(a.a1t, j, i, k) / ps);                        // :234
  if (has(RCMDYN_OUT_U)) put3(RCMDYN_OUT_U, XWIND(a.a1u, k));
  if (has(RCMDYN_OUT_V)) put3(RCMDYN_OUT_V, XWIND(a.a1v, k));
  if (has(RCMDYN_OUT_W)) put3(RCMDYN_OUT_W, d_half * (F3(a.a1w, j, i, k + 1) + F3(a.a1w, j, i, k)) / ps);   // :277
  if (has(RCMDYN_OUT_PP)) put3(RCMDYN_OUT_PP, F3(a.a1pp, j, i, k) / ps);                     // :291
  if (has(RCMDYN_OUT_QV)) {                                                                  // :301, 305
    const double q = F3(a.a1qv, j, i, k) / ps;
    put3(RCMDYN_OUT_QV, q / (d_one + q));
  }
  if (has(RCMDYN_OUT_QC)) put3(RCMDYN_OUT_QC, F3(a.a1qc, j, i, k) / ps);                     // :314
  if (has(RCMDYN_OUT_QI)) put3(RCMDYN_OUT_QI, F3(a.a1qx[0], j, i, k) / ps);                  // :336
  if (has(RCMDYN_OUT_QR)) put3(RCMDYN_OUT_QR, F3(a.a1qx[1], j, i, k) / ps);                  // :325
  if (has(RCMDYN_OUT_QS)) put3(RCMDYN_OUT_QS, F3(a.a1qx[2], j, i, k) / ps);                  // :347
  if (has(RCMDYN_OUT_TKE)) put3(RCMDYN_OUT_TKE, F3(a.a1tke, j, i, k));                       // :576
  if (has(RCMDYN_OUT_PH)) {
    double ph;
    if (!nh) ph = (c->sigma[k] * ps + ptop) * d_1000;                                        // :388
    else if (k == 1) ph = ptop * d_1000;                                                     // :409
    else ph = F3(a.pf0, j, i, k) + d_half * (F3(a.a1pp, j, i, k - 1) + F3(a.a1pp, j, i, k)) / ps;   // :413-414
    put3(RCMDYN_OUT_PH, ph);
  }
  if (has(RCMDYN_OUT_ZH)) {                                                                  // :396-403
    const double cell = ptop / ps;
    const double lay = rovg * F3(a.a1t, j, i, k) / ps * log((c->sigma[k + 1] + cell) / (c->sigma[k] + cell));
    put3(RCMDYN_OUT_ZH, k == kz ? lay : F3(a.zq, j, i, k + 1) + lay);
  }
  if (has(RCMDYN_OUT_RH)) {                                                                  // :366-368
    const double rh = (F3(a.a1qv, j, i, k) / ps) / pfwsat(F3(a.a1t, j, i, k) / ps, F3(a.pr, j, i, k), a.ep2);
    put3(RCMDYN_OUT_RH, d_100 * dmin(a.rhmax, dmax(a.rhmin, rh)));
  }
  if (has(RCMDYN_OUT_PF)) put3(RCMDYN_OUT_PF, F3(a.pf3d, j, i, k));                          // :378
  if (has(RCMDYN_OUT_ZF)) put3(RCMDYN_OUT_ZF, F3(a.zq, j, i, k));                            // :452
  if (has(RCMDYN_OUT_OMEGA)) put3(RCMDYN_OUT_OMEGA, F3(a.omega, j, i, k) * d_10);            // :268

  if (k != 1) return;
  if (has(RCMDYN_OUT_PS)) put2(RCMDYN_OUT_PS, ps);
  if (has(RCMDYN_OUT_PS_PA)) {                                                               // :933-941
    if (nh) put2(RCMDYN_OUT_PS_PA, F2(a.ps0, j, i) + ptop * d_1000 + F3(a.a1pp, j, i, kz) / ps);
    else put2(RCMDYN_OUT_PS_PA, d_1000 * (ps + ptop));
  }
  if (has(RCMDYN_OUT_UA100) || has(RCMDYN_OUT_VA100)) {                                      // :1057-1150
    // the height of the half levels from the ground up: atm0%z (NH), or the layers rebuilt from
    // the current t and qv (hydrostatic), until the first one above 100 m
    const double cell = ptop / ps;
    auto height = [&](int kk, double below) {
      if (nh) return F3(a.z0, j, i, kk);
      const double tv = F3(a.a1t, j, i, kk) / ps * (d_one + ep1 * F3(a.a1qv, j, i, kk) / ps);
      const double lay = rovg * tv * log((c->sigma[kk + 1] + cell) / (c->sigma[kk] + cell));
      return kk == kz ? lay : below + lay;
    };
    double zz = height(kz, d_zero);
    if (zz > 100.0) {
      if (has(RCMDYN_OUT_UA100)) put2(RCMDYN_OUT_UA100, XWIND(a.a1u, kz));
      if (has(RCMDYN_OUT_VA100)) put2(RCMDYN_OUT_VA100, XWIND(a.a1v, kz));
    } else {
      // a column with no half level above 100 m: the text's loop ends without an assignment and the
      // stream buffer keeps its previous record; the compact buffer has none, so zero
      double ua = d_zero, va = d_zero;
      for (int kk = kz - 1; kk >= 1; kk--) {
        const double zz1 = height(kk, zz);
        if (zz1 > 100.0) {
          const double ww = (100.0 - zz) / (zz1 - zz);
          if (has(RCMDYN_OUT_UA100)) ua = ww * XWIND(a.a1u, kk) + (d_one - ww) * XWIND(a.a1u, kk + 1);
          if (has(RCMDYN_OUT_VA100)) va = ww * XWIND(a.a1v, kk) + (d_one - ww) * XWIND(a.a1v, kk + 1);
          break;
        }
        zz = zz1;
      }
      if (has(RCMDYN_OUT_UA100)) put2(RCMDYN_OUT_UA100, ua);
      if (has(RCMDYN_OUT_VA100)) put2(RCMDYN_OUT_VA100, va);
    }
  }
#undef XWIND
}

template __global__ void k_output<double>(Geom, const Consts* __restrict__, OutArgs);
template __global__ void k_output<float>(Geom, const Consts* __restrict__, OutArgs);

}  // namespace rcm
