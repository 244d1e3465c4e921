// massck.hpp -- the mass check of tend (Main/mod_massck.F90:190-306, idynamic /= 3) on the device.
#pragma once
#include "engine.hpp"

namespace rcm {

// k_massck's blocks (64 x 4 threads) of one tile, and the slots of its partial sums:
//   blocks 0 .. nbdy-1: the boundary-line items (line, chunk of 256 line points, level), item
//     b = (level * nbchunk + chunk) * 4 + line, lines west, east, south, north; two slots each,
//     the signed dry-air and water fluxes (zero for a line the tile does not have)
//   then (nqx * kz + 1) planes x nchunk row chunks of MCK_ROWS interior rows: plane p < nqx * kz
//     is species p / kz at level p % kz + 1, the last plane is p*; one slot each, the plain sum
constexpr int MCK_ROWS = 16;
constexpr int MCK_MAXQX = 2 + NQXH;
constexpr int MCK_NREC = 6;             // doubles per record: lcount, dt, drymass, dryadv, qmass, qadv

struct MassckArgs {
  const double *u, *v, *psa;            // atm1%u, atm1%v, sfs%psa of the tile's current parity
  const double* qx[MCK_MAXQX];          // atm1%qx: qv, qc (, qi, qr, qs)
  int nqx;
  double* part;                         // the tile's slots
  int nbdy, nbchunk, nchunk;
};
// where a tile's slots lie in the engine's partial buffer (k_massck_final's table)
struct MassckTile {
  int off, nbdy, nchunk, nbchunk;
};

__global__ void k_massck(Geom g, const Consts* c, const StepState* s, MassckArgs a);
__global__ void k_massck_final(const Consts* c, const StepState* s, const double* part, const MassckTile* tab,
                               int ntile, int nqx, double* log, long long* count, int cap);

}  // namespace rcm
