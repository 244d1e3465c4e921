// che_output.hpp -- argument block of the CHE output-stream kernel (che_output.hip): the tracer
// fields of mod_che_output's fill_chem_outvars that the dyn core owns (enum rcmdyn_che_field,
// include/rcmdyn.h).
//
// Left on the host: the cumulus scheme's own share of CHE_CONV, che_pp_out (OUT_PP serves it), the
// physics-owned CHE variables (deposition, emissions, ctbldiag, ...), the OPT stream and NetCDF.
#pragma once
#include "kernels.hpp"     // QxArgs: the tracer groups' table

namespace rcm {

// the levels of a CHE field: the burden is a plane, the others have kz levels
__host__ __device__ __forceinline__ int che_levels(int f, int kz) { return f == RCMDYN_CHE_BURDEN ? 1 : kz; }

// inputs, all read at the thread's own point: sfs%psb, the groups' table (chia = a1 of the tracer's
// group), the accumulator table [term][tracer] (null with the tracer budget off) and the leftovers
// of the last mkslice for the burden: chib3d's pointer table, rhob3d and dzq (hydrostatic) or the
// atm0%zf whose differences are the NH core's dzq (Main/mod_atm_interface.F90:977,
// Main/mod_params.F90:2636).
// out: the tile's compact buffer; tracer b of the batch occupies stride elements from b * stride,
// field f of it levels * nci * ncj elements from off[f] (floats or doubles), j fastest over
// jci1:jci2, then i over ici1:ici2, then k.
struct CheArgs {
  const double* psb;
  const QxArgs* tab;
  double* const* acc;
  double* const* chib3d;
  const double *dzq, *zf0, *rhob3d;
  void* out;
  long off[RCMDYN_NCHE];
  long stride;
  unsigned mask;
  int itr0, nb, ntr;           // the batch: tracers itr0 .. itr0 + nb - 1 (from 0) of ntr
};

// T: double (prec = 8) or float (prec = 4).  grid (ceil(ncj / 64), ceil(nci / 4), kz * nb), block
// (64, 4): z = tracer of the batch * kz + level - 1.
template <class T>
__global__ void k_output_che(Geom g, int kz, CheArgs a);

}  // namespace rcm
