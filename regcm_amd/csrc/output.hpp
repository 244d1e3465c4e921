// output.hpp -- argument block of the output-stream kernel (output.hip): the dyn-owned fields of
// mod_output's ATM stream and of SRF / SHF (enum rcmdyn_output_field, include/rcmdyn.h).
//
// Left on the host: uvrotate (wind_antirotate has one branch per projection; the host applies it
// to the fetched u, v), CAPE / CIN (getcape), every physics-owned variable of the streams, the
// idiag terms (rcmdyn_get_budget serves them) and NetCDF itself.
#pragma once
#include "devcommon.hpp"

namespace rcm {

// the levels of an output field: 2-D for the surface fields, kz for the others
__host__ __device__ __forceinline__ bool out_is_2d(int f) {
  return f == RCMDYN_OUT_PS || f == RCMDYN_OUT_PS_PA || f == RCMDYN_OUT_UA100 || f == RCMDYN_OUT_VA100;
}

// inputs: the state of the moment (atm1, sfs%psa; NH: pp, w and the atm0 fields), the leftovers of
// the last mkslice (atm1%pr, pf3d, zq) and the diagnostics export omega; null where the mask or
// the configuration leaves a field out.
// out: the tile's compact buffer; field f occupies off[f] .. off[f] + levels * nci * ncj elements
// (floats or doubles), j fastest over jci1:jci2, then i over ici1:ici2, then k.
struct OutArgs {
  const double *psa, *a1t, *a1u, *a1v, *a1qv, *a1qc, *a1tke;
  const double* a1qx[NQXH];
  const double *a1pp, *a1w, *ps0, *pf0, *z0;          // non-hydrostatic core only
  const double *pr, *pf3d, *zq, *omega;
  void* out;
  long off[RCMDYN_NOUT];
  unsigned mask;
  double ep2, rhmin, rhmax;
};

// T: double (prec = 8) or float (prec = 4).  grid (ceil(ncj / 64), nci, kz), block 64.
template <class T>
__global__ void k_output(Geom g, const Consts* __restrict__ c, OutArgs a);

}  // namespace rcm
