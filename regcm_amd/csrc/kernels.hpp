// kernels.hpp -- device kernels of kernels.hip and the argument blocks they share.
#pragma once
#include <type_traits>
#include "engine.hpp"

namespace rcm {

// one halo staging segment (see k_pack_segs)
struct Seg {
  double* p;
  long kstride;
  int pitch, j0, i0, j1, j2, i1, i2, nk;
  long off;
};
constexpr int MAXSEG = 64;
// k_split_project's extra blocks for the listed negative moisture forecasts (qfuse)
constexpr int NEGFIX_BLOCKS = 64;
// fused spstep tiling: SPB x SPB owned cross points + SPH halo (>= sub-steps per mode)
constexpr int SPB = 16, SPH = 8;
// k_update: XCD-aware tile placement within each level (xcd_tile2d, devcommon.hpp) on tiles of
// fewer points than this (rank tiles).  Alternating on one box (profiles/r05/tile_ab_uxcd.log,
// c3_uxcd_ab.log): 96x48 0.0792 -> 0.0773-0.0783 ms, 96x96 0.0962 -> 0.0936, 96x192 0.1325 ->
// 0.1310 ms; the 192x192 tile 2-5 us slower in k_update (99-101 -> 102-104 us), so off there
#ifndef UPD_XCD_BELOW
#define UPD_XCD_BELOW (192 * 192 / 2 + 1)
#endif
// the 8 x 8 form (k_spstep_fused<8>) below this many 16 x 16 blocks (engine.hip)
#ifndef SP8_BELOW
#define SP8_BELOW 128
#endif
constexpr int SPR = SPB + 2 * SPH, SPP = SPR + 1;  // region side, LDS row pitch
// k_columns: COLW columns x 8 level groups per block (COLT threads, 4 x kz x COLW doubles of LDS;
// 32 measured 1-2 us slower at C3 than 64, profiles/r05/tile_ab_colw.log)
#ifndef RCM_COLW
#define RCM_COLW 64
#endif
#ifndef RCM_COLG
#define RCM_COLG 8
#endif
constexpr int COLW = RCM_COLW, COLG = RCM_COLG, COLT = COLW * COLG;   // COLG level groups
// k_split_project: SPC dot columns x SPG level groups per block (256 threads, 4 x kz x SPC
// doubles of LDS).  At C3 one row of 64 columns x 8 groups (512 threads) gave 576 blocks, a
// round and an eighth on 256 CUs at two blocks each; 32 x 8 gives 1 152 blocks of 23 KB, five
// per CU, one round (the kernel's time did not change: its block life, not the tail, sets it;
// profiles/r05/tile_ab_colw.log)
#ifndef RCM_SPC
#define RCM_SPC 32
#endif
constexpr int SPC = RCM_SPC, SPG = 8;
// k_split_project / k_split_correct(_bdy) place their blocks XCD-contiguously (xcd_range,
// devcommon.hpp): the rows a projection block shares with the next row's block, and the 2-D
// split sums every level of a correction block column reads, stay in one L2.  k_columns does
// the same for its column blocks of a whole tile (part 0): the next row's column block, whose
// loads overlap this one's (atm1 at i + 1, p* at i +- 1), runs on the same XCD.  The
// measurements are in DESIGN.md section 4 (round 6)
// depth of the wide exchange: SPH plus the ghost ring the fused split step also produces
constexpr int SPX = SPH + 1;
// LDS-tiled momentum block (dot points j x i at one level).  32 x 8 (256 threads, 39 KB of
// LDS: four blocks per CU): at C3 k_update 108 -> 97 us and the step 214 -> 200-203 us; on
// the 96-point rows of the scaling runs' tiles no half-idle second block column, and 96 x 48
// fits one round of blocks (step 88.6 -> 81.1 us); 64 x 8, 32 x 16 and 64 x 4 measured slower
// (round 5, alternating on one box: profiles/r05/tile_ab_w32.log)
#ifndef RCM_MBI
#define RCM_MBI 8
#endif
#ifndef RCM_MBJ
#define RCM_MBJ 32
#endif
constexpr int MBJ = RCM_MBJ, MBI = RCM_MBI, MBT = MBJ * MBI;
// LDS-tiled scalar (t, qv, qc) block (cross points j x i at one level)
#ifndef RCM_SBI
#define RCM_SBI 8
#endif
#ifndef RCM_SBJ
#define RCM_SBJ 32
#endif
constexpr int SBJ = RCM_SBJ, SBI = RCM_SBI, SBT = SBJ * SBI;
// k_update runs a momentum block or a scalars block in every workgroup of one launch, so the
// two block kinds must have the same thread count (their heights may differ only with it)
static_assert(MBT == SBT, "k_update launches momentum and scalars blocks with one block size");
// LDS-tiled species block of k_qx_tend (cross points j x i at one level).  Independent of the
// scalars tile: the launch in tend_post uses these constants, and the engine checks at create
// that the kernel was compiled for QBT threads (check_block_sizes, engine.hip)
#ifndef RCM_QBI
#define RCM_QBI 8
#endif
#ifndef RCM_QBJ
#define RCM_QBJ 64
#endif
constexpr int QBJ = RCM_QBJ, QBI = RCM_QBI, QBT = QBJ * QBI;
struct SegList {
  Seg s[MAXSEG];
  int n;
};

// boundary slices, order documented at k_bdyval_set
struct Slices { double* s[16]; };

// Halo/compute overlap of a decomposed tile: while the prologue exchange is in
// flight on the second stream, part 1 runs the blocks of k_columns / k_momentum / k_scalars
// whose reads all lie in R = [ja, jb] x [ia, ib], points no exchange writes and whose k_columns
// outputs part 1 itself forms; part 2 runs the others after the join; part 0 every block.
// k_columns maps its part 1 blocks onto the rows of R (nxb blocks of 64 columns per row) and
// its part 2 blocks onto the rest of the column box as one list (rbase: part 1's block count,
// so each block keeps its own noise partial).
// mj0 / sj0: the j origin of k_momentum's / k_scalars' 64-wide block columns in parts 1 and 2,
// shifted on narrow tiles so that one block column lies wholly in R (part 0: jdi1 / jcx1).
struct Part {
  int part, ja, jb, ia, ib, nxb, rbase, mj0, sj0;
};

// Every device buffer of one tile for one ping-pong parity: a* are the current time levels,
// b* the buffers the fused update kernels write the next time levels into.  Passed by value
// (kernel argument segment -> SGPRs); all fields share the frame, so one 32-bit byte offset
// per point addresses every one of them.  Diagnostic pointers are null when diagnostics are
// off (rcmdyn_set_diagnostics).
struct Fields {
  double *a1u, *a1v, *a1t, *a1qv, *a1qc, *a2u, *a2v, *a2t, *a2qv, *a2qc, *psa, *psb;
  double *b1u, *b1v, *b1t, *b1qv, *b1qc, *b2u, *b2v, *b2t, *b2qv, *b2qc, *bpsa, *bpsb;
  double *msfx, *msfd, *coriol, *ht, *xmsf, *dmsf, *hgfact, *mapf;
  const int8_t *rgcr, *rgdt;
  const int16_t *ibcr, *ibdt;
  double *ub0, *ubt, *vb0, *vbt, *tb0, *tbt, *qb0, *qbt, *pb0, *pbt;
  double *rpsa, *rpsb, *rpsda, *rpsdb, *psc, *psdota, *psdotb, *pten, *ptenn;
  double *qdot, *phi, *cqv, *cqc, *fqv, *fqc;
  double *slqv, *slqc;         // semi-Lagrangian qv/qc tendency starts (isladvec = 1, k_sladv)
  double *d6u, *d6v, *d6t, *d6qv, *d6qc;   // idiffu = 3 column terms (k_diffu6)
  unsigned* depplane;
  double *tten, *uten, *vten, *qvten, *qcten, *omega, *xkcs;
  // physics tendencies of the coupling seam (null: physics stubbed, the terms are 0)
  const double *tphy, *qvphy, *qcphy, *uphy, *vphy;
  const double* kpbl;          // iuwvadv = 1 (ibltyp = 2): the PBL-top level, vadv4d ind = 3 of qc
  // qfuse (the step without k_qfilter): k_columns filters p* into bpsa/bpsb and copies the
  // points the update kernels do not write into the next buffers; k_scalars RAW-filters the
  // non-negative moisture forecasts into b1q/b2q and appends the negative ones to neglist
  // (element offset * 2 + n) for k_split_project's fix-up blocks
  int qfuse;
  int* negcnt;
  uint32_t* neglist;
  // nqx = 5: atm1 of the hydrometeors beyond qc (k_columns: the total water load of tvfac)
  const double* qxa1[NQXH];
  double* red;                 // engine-wide noise-sum partials (k_columns -> k_split_correct)
  int red_off;                 // this tile's first partial
  Part pt;                     // the launch's overlap part (k_columns, k_momentum, k_scalars)
};

// Tendency budget of t and qv (idiag = 1, rcmdyn_set_budget): the accumulators tdiag / qdiag
// %adh, adv, adi, bdy, dif of ten2diag (Main/mod_tendency.F90:2123-2175), frame planes like tten,
// and the host's alarm_out_atm%rw.  A trailing argument of its own of the budget instances of the
// tendency kernels (k_scalars, k_update, k_nh_tend_c with Budget in their pack); the other
// instances take none and hold no code for it.  Each term is the rounded difference of the
// running tendency around its stage, acc = acc + (after - before) * rw, on the tile's own
// interior cross points.
constexpr int NBUDTERM = 5;          // adh, adv, adi, bdy, dif
struct Budget {
  double *t[NBUDTERM], *q[NBUDTERM];
  double rw;
};

// SUBEX condensation (condtq, rcmdyn_set_condtq; condtq.hpp): the host's rh0adj, the three frame
// arrays that hold the last tend's coupled increments of t, qv, qc (aten pc_physic after condtq),
// and subexparam's conf.  A trailing argument of its own of the condtq instances of the tendency
// kernels (Condtq in their pack, after Budget); the other instances take none and hold no code
// for it.
struct Condtq {
  const double* rh0adj;
  double *it, *iqv, *iqc;
  double conf;
};

// The extra argument blocks of a tendency kernel are a trailing pack B... (empty, Budget, Condtq
// or Budget, Condtq): pack_has tells an instance whether a block is among them, pack_get returns
// it (a value-initialised one when it is not, for code that the instance does not hold)
template <class T, class... B>
constexpr bool pack_has = (std::is_same<T, B>::value || ...);
template <class T>
__host__ __device__ __forceinline__ T pack_get() { return T{}; }
template <class T, class B0, class... B>
__host__ __device__ __forceinline__ T pack_get(const B0& b0, const B&... b) {
  if constexpr (std::is_same<T, B0>::value) return b0;
  else return pack_get<T>(b...);
}

// nqx = 5: the hydrometeors beyond qc (qi, qr, qs) for the current (a*) and next (b*) time-level
// buffers (species.hip; the non-hydrostatic core updates a* in place and leaves b* null)
struct QxArgs {
  double *a1[NQXH], *a2[NQXH], *b1[NQXH], *b2[NQXH];
  double *cq[NQXH], *fq[NQXH];
  double *sl[NQXH], *d6[NQXH];
  const double* phy[NQXH];
  const double *b0[NQXH], *bt[NQXH];   // tracers: chib0, chibt of the boundary relaxation (null for the species)
  unsigned* dep;               // per (species, level) plane: row bitmap of the serially dependent negative points
  unsigned* depf;              // per (species, level) plane and row: k_qx_fix's flag of such a point (k_qx_serial
                               // turns the flags into the bitmap)
  int nsp;                     // hydrometeors beyond qc (0 for nqx = 2); tracers: those of the group
};

// The chemical tracers (rcmdyn_set_tracers) go through the hydrometeors' kernels in groups of up
// to NQXH: one QxArgs per group in a table in device memory, the group index on a grid dimension
// (z = group * kz + level, or group * NQXH * kz + plane), so a block stages the cell's mass
// fluxes once for its group.  cefc / cegc: nudge_chiten's tables, cefc(ib, k) at [(k - 1) *
// nspgx + ib - 1]; relax: the relaxation term runs (iboudy 1 or 5 and a table entry is non-zero)
struct TrArgs {
  const QxArgs* tab;
  const double *cefc, *cegc;
  int ngroups, relax;
};

// Tracer budget (ichdiag > 0, rcmdyn_set_tracer_budget): the accumulators cadvhdiag, cadvvdiag,
// cbdydiag, cdifhdiag of the five ten2diag calls on aten%chi (Main/mod_tendency.F90:1403-1412,
// 1503-1511, 1540-1542) and cconvdiag of cumtran (Main/chemlib/mod_che_cumtran.F90:159-166), one
// frame array of kz levels per (term, tracer): acc[term * ntr + tracer] in device memory.  A
// trailing argument of its own of the budget instances k_qx_tend<FamTr, TrBudget> and
// k_nh_qx_tend<FamTr, TrBudget> (as Budget of the t / qv kernels); the other instances take none
// and hold no code for it.  Each stage term is the rounded difference of the running chidyn around
// its stage, acc = acc + (after - before) * rw, on the tile's own jci x ici.
constexpr int NTRBUDTERM = RCMDYN_NTRDIAG;     // advh, advv, bdy, difh, conv
struct TrBudget {
  double* const* acc;
  double rw;                   // alarm_out_atm%rw (extracttenchi, :2177-2207)
  int ntr;
};

// Cumulus mixing of the tracers (cumtran, rcmdyn_set_cumtran): init_cumtran's mask (0 / 1) and
// kcumtop (2-D, doubles holding integers), convcldfra (kz levels); ncum: syncro_cum's period in
// steps; conv / cfdout: cconvdiag's accumulators [tracer] and alarm_out_che%rw, conv null with the
// tracer budget off
struct TrCum {
  const double *dotran, *ktop, *cldfra;
  double* const* conv;
  double cfdout;
  int ncum;
};

// The two families of the kernels of species.hip and of the serial negative-value fix
// (qxcommon.hpp), a compile-time parameter F: what differs between the reference's chain of a
// hydrometeor beyond qc and of a tracer.
//   floor   the decoupling max(atm1 * rpsa, 0) (Main/mod_tendency.F90:1022-1026) against the
//           plain product of the tracers (:1030-1032)
//   thr     vadv4d's threshold of ind = 1 against ind = 2 (Main/mod_advection.F90:878, 900)
//   fixfac  the factor of the negative-value fix (Main/mod_tendency.F90:389 against :576)
//   cr      the NH adiabatic term atmx%qx * cr (:1615-1617; n = 1..nqx only, no tracer)
//   relax   nudge_chiten (Main/chemlib/mod_che_bdyco.F90:898-982; the hydrometeors relax nothing)
//   Args    the argument block: the species' QxArgs by value, the tracers' table
static constexpr double MINTR = 1.0e-30;     // Share/mod_constants.F90:63 (double precision)
struct FamQx {
  using Args = QxArgs;
  static constexpr bool floor = true, cr = true, relax = false, grouped = false;
  static constexpr double fixfac = 0.01;
  static __host__ __device__ __forceinline__ double thr(double ps) { return 1.0e-8 * 1.0e-8 * ps; }
  static __device__ __forceinline__ const QxArgs& group(const Args& a, int) { return a; }
};
struct FamTr {
  using Args = TrArgs;
  static constexpr bool floor = false, cr = false, relax = true, grouped = true;
  static constexpr double fixfac = 0.1;
  static __host__ __device__ __forceinline__ double thr(double ps) { return MINTR * ps; }
  static __device__ __forceinline__ const QxArgs& group(const Args& a, int grp) { return a.tab[grp]; }
};

// serial negative-moisture fix-up of k_split_project's extra blocks: the q fields before
// (o*) and after (n*) the RAW filter, the unfiltered forecasts (c*) and fixed values (f*)
struct QFix {
  const double *cqv, *cqc;
  double *fqv, *fqc;
  const double *o1qv, *o1qc, *o2qv, *o2qc;
  double *n1qv, *n1qc, *n2qv, *n2qc;
  const double *psa, *psb;
  // the step's p* before its RA filter and psc: the serial sweep (in k_split_correct with
  // qfuse, beside the split corrections of psa/psb) forms the filtered p* from them
  const double *psc, *opsa, *opsb;
  unsigned* depplane;
  // qfuse: the negative forecasts k_scalars listed (k_split_project fixes the independent ones
  // in parallel; the serial sweeps of the flagged planes run in k_split_correct)
  const int* negcnt;
  const uint32_t* neglist;
  // qfuse: per (qv | qc, level) plane and row, the list pass's flag of a dependent point (a plain
  // store: atomics on the few bitmap words of a plane serialise at the memory side); the serial
  // passes OR the flags into depplane first (negfix_collect, qxcommon.hpp)
  unsigned* depf;
};

__global__ void k_surface_pressures(Geom g, Fields f);
template <bool QX>
__global__ void k_columns(Geom g, const Consts* __restrict__ c, StepState* s, Fields f, int nxb, int ncol);
__global__ void k_sladv(Geom g, const Consts* __restrict__ c, StepState* s, Fields f, QxArgs q);
// k_momentum, k_scalars, k_update: O the policy of the option reads (pointops.hpp; the engine
// picks OptDefault or OptGeneric per launch, optset.hpp), B... the extra argument blocks above.
// The instances are those kernels.hip instantiates: <OptDefault>, <OptGeneric>, and for the
// latter two kernels <OptGeneric, Budget>, <OptGeneric, Condtq>, <OptGeneric, Budget, Condtq>.
template <class O>
__global__ void k_momentum(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, Fields f);
__global__ void k_diffu6(Geom g, const Consts* __restrict__ c, Fields f, QxArgs q);
template <class O, class... B>
__global__ void k_scalars(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, Fields f, B... b);
template <class O, class... B>
__global__ void k_update(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, Fields fm, Fields fs,
                         int mnx, int mny, int snx, int sny, int xcd, B... b);
__global__ void k_qfilter(Geom g, const Consts* __restrict__ c, Fields f);
// the serial fix passes resolve the chain (qxcommon.hpp), k_negfix_post / k_qx_post apply the
// filters of the points they fixed
__global__ void k_negfix_serial(Geom g, const Consts* __restrict__ c, QFix q);
__global__ void k_negfix_post(Geom g, const Consts* __restrict__ c, QFix q);
__global__ void k_split_project(Geom g, const Consts* __restrict__ c, const double* __restrict__ a1u,
                                const double* __restrict__ a1v, const double* __restrict__ a2u,
                                const double* __restrict__ a2v, const double* __restrict__ a1t,
                                const double* __restrict__ a2t, const double* __restrict__ psa,
                                const double* __restrict__ psb, const double* __restrict__ msfd,
                                const double* __restrict__ mapf, double* dstor, double* hstor, double* deld,
                                double* delh, double* psdota, int nxp, int nproj, QFix qf, Geom gw,
                                double* wdeld, double* wdelh, double* wpsdota, double* wpsa,
                                const double* __restrict__ o2u, const double* __restrict__ o2v);
__global__ void k_spstep_init(Geom g, const Consts* __restrict__ c, const double* __restrict__ deld, const double* __restrict__ delh, double* ddsum, double* dhsum);
__global__ void k_spstep_grad(Geom g, const Consts* __restrict__ c, int l, int src, const double* __restrict__ delh, const double* __restrict__ msfx, const double* __restrict__ msfd, const double* __restrict__ psdota, double* uu, double* vv);
__global__ void k_spstep_update(Geom g, const Consts* __restrict__ c, int l, int n0, int n1, int nn, int leap, const double* __restrict__ uu, const double* __restrict__ vv, const double* __restrict__ mapf, const double* __restrict__ psa, double* deld, double* delh, double* ddsum, double* dhsum);
template <int SB>
__global__ void k_spstep_fused(Geom g, Geom w, const Consts* __restrict__ c, const double* __restrict__ deld, const double* __restrict__ delh, const double* __restrict__ msfx, const double* __restrict__ msfd, const double* __restrict__ psdota, const double* __restrict__ mapf, const double* __restrict__ psa, double* ddsum, double* dhsum);
template <int NS>
__global__ __launch_bounds__(256) void k_split_correct(Geom g, const Consts* __restrict__ c, const double* __restrict__ ddsum, const double* __restrict__ dhsum, const double* __restrict__ psdota, const double* __restrict__ msfd, double* psa, double* psb, double* a1t, double* a2t, double* a1u, double* a1v, double* a2u, double* a2v, StepState* s, int advance, const double* __restrict__ red, int red_total, FlagSnap* ring, QFix qf, int nser);
// pointers of bdyval (k_bdyval_set)
struct BdyArgs {
  double *a1u, *a1v, *a1t, *a1qv, *a1qc, *a2u, *a2v, *a2t, *a2qv, *a2qc, *psa, *psb;
  const double *ub0, *ubt, *vb0, *vbt, *tb0, *tbt, *qb0, *qbt, *pb0, *pbt;
  Slices sl;
  long slen;
  int set_ps;
};
__global__ void k_bdyval_set(Geom g, const StepState* __restrict__ s, BdyArgs a);
// 64-point chunks of the longest boundary line, one point past the tile included
__host__ __device__ __forceinline__ int bdy_chunks(const Geom& g) {
  const int nj = g.jde2 - g.jde1, ni = g.ide2 - g.ide1;
  return ((nj > ni ? nj : ni) + 65) / 64;
}
template <int NS>
__global__ __launch_bounds__(256) void k_split_correct_bdy(Geom g, const Consts* __restrict__ c, const double* __restrict__ ddsum, const double* __restrict__ dhsum, const double* __restrict__ psdota, const double* __restrict__ msfd, StepState* s, int advance, const double* __restrict__ red, int red_total, BdyArgs a, QFix qf, int nser);
__global__ void k_bdyval_qc(Geom g, int do_qc, int do_qv, double* a1qc, double* a1qv, const double* __restrict__ psa, Slices sl, long slen, StepState* s, double dtsec, int advance, FlagSnap* ring);
__global__ void k_flag_snapshot(const StepState* __restrict__ s, FlagSnap* ring);
__global__ void k_err_gather(const StepState* __restrict__ s, int32_t* derr);
__global__ void k_err_publish(const int32_t* __restrict__ derr, int32_t* hslot);
__global__ void k_prepare_static(Geom g, const Consts* __restrict__ c, int diffu_hgtf, const double* __restrict__ msfx, const double* __restrict__ msfd, const double* __restrict__ ht, double* xmsf, double* dmsf, double* hgfact, double* mapf);
__global__ void k_pack_segs(SegList L, double* __restrict__ buf, int unpack);
__global__ void k_copy_frame(Geom g, Geom w, int nplanes, const double* __restrict__ src, long sstride, double* dst, long dstride);

// species.hip: the hydrometeors beyond qc (nqx = 5), hydrostatic core (the ping-pong buffers)
// F: the family (FamQx, FamTr above); species.hip instantiates both of each kernel
// B...: empty, or TrBudget for the tracers' budget instance (k_qx_tend, k_nh_qx_tend)
template <class F, class... B>
__global__ void k_qx_tend(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, Fields f,
                          typename F::Args a, B... b);
template <class F>
__global__ void k_qx_fix(Geom g, const Consts* __restrict__ c, typename F::Args a);
template <class F>
__global__ void k_qx_serial(Geom g, const Consts* __restrict__ c, typename F::Args a);
template <class F>
__global__ void k_qx_post(Geom g, const Consts* __restrict__ c, typename F::Args a);
__global__ void k_negfix_serial_qx(Geom g, const Consts* __restrict__ c, QFix qf, QxArgs q);
struct NHFields;
// the non-hydrostatic chains of the same hydrometeors (in place; k_qx_fix / k_qx_serial then
// run with b* = a*)
template <class F, class... B>
__global__ void k_nh_qx_tend(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, NHFields f,
                             typename F::Args a, B... b);
// cumtran2 (Main/chemlib/mod_che_cumtran.F90:132-166) on the filtered time levels b1 / b2 of every
// tracer at the tile's own jci x ici, a thread per (j, i, tracer); acts when lcount > 0 and
// lcount % ncum == 0 (rcmtimer%integrating, syncro_cum%act)
__global__ void k_tr_cumtran(Geom g, const Consts* __restrict__ c, const StepState* __restrict__ s, TrArgs a, int ntr,
                             TrCum cu);
// chem_bdyval_coupled, ichebdy = 1 (Main/chemlib/mod_che_bdyco.F90:565-758), one block per
// (level, tracer); integ as k_bdyval_qx; pre_clock: the step's clock is not advanced yet (the
// bdyval lines ran in k_split_correct_bdy), so dt is the one the advance will set
__global__ void k_bdyval_chi(Geom g, const StepState* __restrict__ s, TrArgs a, int ntr, int integ, int pre_clock,
                             double dtsec);
// mkslice's chib3d = max(atm2 * rpsb, 0) (Main/mod_slice.F90:196-200) of every tracer on the
// tile's cross points (z = tracer * kz + level)
__global__ void k_tr_slice(Geom g, int kz, int ntr, TrArgs a, const double* __restrict__ rpsb, double* const* out);
// bdyval's boundary copies and inflow/outflow of the hydrometeors beyond qc (both cores);
// integ: 1 integrating, 0 the initial call, -1 from the step clock (lcount > 0)
__global__ void k_bdyval_qx(Geom g, const StepState* __restrict__ s, QxArgs q, int integ, int do_qc,
                            const double* __restrict__ psa, Slices sl, long slen);

}  // namespace rcm
