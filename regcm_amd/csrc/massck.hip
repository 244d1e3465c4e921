// massck.hip -- the mass check that ends tend's debug path (`if ( debug_level > 0 ) call massck`,
// Main/mod_tendency.F90:415; Main/mod_massck.F90:190-306, the idynamic /= 3 branch): the dry-air
// and water mass of the interior and their fluxes through the lateral boundary lines, summed on
// the device from atm1 and p* as they stand after tend's prologue exchange.
//
// k_massck (one launch per tile) writes one partial per block to the block's own slot;
// k_massck_final (one block, after the last tile's launch) adds the slots of every owned tile in
// slot order, scales, and appends one record to the log.  Every sum is a fixed tree: no
// floating-point atomics, so a record does not depend on how the blocks were scheduled.
#include "massck.hpp"

#include "devcommon.hpp"

namespace rcm {

// the sum of v over the block's 256 threads in a fixed order: the 64 lanes of each wavefront by a
// shuffle tree, then the four wavefronts through LDS; every thread returns it
__device__ __forceinline__ double mck_block_sum(double v, double* lds) {
  for (int w = 32; w > 0; w >>= 1) v += __shfl_down(v, w, 64);
  __syncthreads();                         // the previous sum's readers are done with lds
  if (threadIdx.x == 0) lds[threadIdx.y] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(256) void k_massck(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s,
                                                MassckArgs a) {
  __shared__ double lds[4];
  const int kz = c->kz;
  const int b = (int)blockIdx.x, t = (int)threadIdx.y * 64 + (int)threadIdx.x;
  if (b < a.nbdy) {
    // boundary input (:203-234, 269-304): west and east over i = ice1..ice2 with the dot-point
    // wind of the boundary column averaged to the cross row, south and north over j = jci1..jci2
    const int line = b & 3, chunk = (b >> 2) % a.nbchunk, k = (b >> 2) / a.nbchunk + 1;
    const bool we = line < 2;
    const bool has = line == 0 ? g.bl : line == 1 ? g.br : line == 2 ? g.bb : g.bt;
    const int p = chunk * 256 + t;
    const int np = we ? g.ice2 - g.ice1 + 1 : g.jci2 - g.jci1 + 1;
    double dry = d_zero, wat = d_zero;
    if (has && p < np) {
      const double coef = s->dt * 3.0e4 * c->dsigma[k] * c->dx * c->regrav;
      int jc, ic;
      double f;
      if (we) {
        const int jd = line == 0 ? g.jde1 : g.jde2;
        jc = line == 0 ? g.jce1 : g.jce2;
        ic = g.ice1 + p;
        f = F3(a.u, jd, ic + 1, k) + F3(a.u, jd, ic, k);
      } else {
        const int id = line == 2 ? g.ide1 : g.ide2;
        ic = line == 2 ? g.ice1 : g.ice2;
        jc = g.jci1 + p;
        f = F3(a.v, jc + 1, id, k) + F3(a.v, jc, id, k);
      }
      dry = coef * f;
      const double ps = F2(a.psa, jc, ic);
      for (int n = 0; n < a.nqx; n++) wat += coef * (f * (F3(a.qx[n], jc, ic, k) / ps));
    }
    dry = mck_block_sum(dry, lds);
    wat = mck_block_sum(wat, lds);
    if (t == 0) {                          // inflow counts positive: west and south add, east and north subtract
      a.part[2 * b] = (line & 1) ? -dry : dry;
      a.part[2 * b + 1] = (line & 1) ? -wat : wat;
    }
    return;
  }
  // interior sums (:190-198, 256-265): one row chunk of one plane; dsigma(k) is applied to the
  // whole level's sum in k_massck_final, as the reference applies it
  const int q = b - a.nbdy, chunk = q % a.nchunk, pl = q / a.nchunk;
  const double* f = pl < a.nqx * kz ? a.qx[pl / kz] + (long)(pl % kz) * g.plane : a.psa;
  const int i1 = g.ici1 + chunk * MCK_ROWS, i2 = min(i1 + MCK_ROWS - 1, g.ici2);
  double v = d_zero;
  for (int i = i1 + (int)threadIdx.y; i <= i2; i += 4)
    for (int j = g.jci1 + (int)threadIdx.x; j <= g.jci2; j += 64) v += F2(f, j, i);
  v = mck_block_sum(v, lds);
  if (t == 0) a.part[2 * a.nbdy + q] = v;
}

// One block.  The slots of every owned tile in slot order (a thread takes every 256th, then a
// fixed tree over the threads, as the Bleck noise sums of k_split_correct), the scaling of
// :235, 306, and the record {lcount, dt, drymass, dryadv, qmass, qadv} at log[count % cap]; the
// clock is the device's, before this tend advances it.
__global__ __launch_bounds__(256) void k_massck_final(const Consts* __restrict__ c, const StepState* __restrict__ s,
                                                      const double* __restrict__ part,
                                                      const MassckTile* __restrict__ tab, int ntile, int nqx,
                                                      double* __restrict__ log, long long* __restrict__ count,
                                                      int cap) {
  __shared__ double sm[4][256];
  const int t = (int)threadIdx.x, kz = c->kz, np = nqx * kz;
  double dm = d_zero, da = d_zero, qm = d_zero, qa = d_zero;
  for (int m = 0; m < ntile; m++) {
    const MassckTile T = tab[m];
    const double* p = part + T.off;
    for (int b = t; b < T.nbdy; b += 256) { da += p[2 * b]; qa += p[2 * b + 1]; }
    const double* in = p + 2 * T.nbdy;
    for (int q = t; q <= np; q += 256) {
      double v = d_zero;                   // the level's (p*'s) sum over the tile
      for (int ch = 0; ch < T.nchunk; ch++) v += in[q * T.nchunk + ch];
      if (q < np) qm += v * c->dsigma[q % kz + 1];
      else for (int k = 1; k <= kz; k++) dm += v * c->dsigma[k];
    }
  }
  sm[0][t] = dm; sm[1][t] = da; sm[2][t] = qm; sm[3][t] = qa;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
      for (int e = 0; e < 4; e++) sm[e][t] += sm[e][t + w];
    __syncthreads();
  }
  if (t == 0) {
    const long long n = *count;
    double* r = log + (n % cap) * MCK_NREC;
    r[0] = (double)s->lcount;
    r[1] = s->dt;
    r[2] = sm[0][0] * c->dxsq * d_1000 * c->regrav;
    r[3] = sm[1][0];
    r[4] = sm[2][0] * c->dxsq * d_1000 * c->regrav;
    r[5] = sm[3][0];
    *count = n + 1;
  }
}

}  // namespace rcm
