// engine.hip -- host side of the MI355X dynamical-core engine and the extern "C" ABI
// (include/rcmdyn.h).
//
// One engine instance owns one or more tiles of the set_nproc decomposition
// (Main/mpplib/mod_mppparam.F90:1053-1371) on one GPU.  A step is the reference sequence
// tend + bdyval (Main/mod_regcm_interface.F90:189,208) issued as ~30 kernels on one HIP
// stream; rcmdyn_step captures one step per ping-pong parity into a hipGraph and replays it.
// Halo exchanges mirror every mpplib exchange the reference performs; tiles on the same
// device exchange through a ghost-fill kernel, tiles on other ranks through RCCL
// (comm.hip).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <execinfo.h>
#include <csignal>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "comm.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "kernels_nh.hpp"
#include "slice.hpp"
#include "bdyin.hpp"
#include "tke.hpp"
#include "fieldtab.hpp"
#include "massck.hpp"
#include "output.hpp"
#include "che_output.hpp"
#include "optset.hpp"
#include "window.hpp"
#include "subex.hpp"
#include "pointops.hpp"   // the policies OptDefault / OptGeneric the tendency kernels are instantiated on

using namespace rcm;

namespace {

thread_local std::string g_last_error;

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess)                                                                \
      throw HipError(std::string(#x) + ": " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
  } while (0)

// constants, Share/mod_constants.F90 (same expressions as oracle/rcm_oracle.c)
constexpr double EGRAV = 9.80665, BOLTZK = 1.3806504e-23, NAVGDR = 6.02214129e23;
constexpr double AMD = 28.96454, AMW = 18.01528, VONKAR = 0.4;

// band (i_band = 1): periodic in j, so no tile has a west/east boundary and the cross grid
// takes every j (global_cross_jend = global_dot_jend, Main/mpplib/mod_mppparam.F90:1351-1354);
// crm (i_crm = 1): the same in i (dim_period(2), :1132, 1340-1342)
void tile_extent(int jx, int iy, int cj, int ci, int tile, int ext[8], int bdy[4], int band = 0, int crm = 0) {
  int lj = tile / ci, li = tile % ci;
  int jxp = jx / cj, iyp = iy / ci;
  int js = lj * jxp + 1, is = li * iyp + 1;
  if (jxp * cj < jx) {
    int imiss = jx - jxp * cj;
    if (lj < imiss) { js += lj; jxp += 1; } else { js += imiss; }
  }
  if (iyp * ci < iy) {
    int imiss = iy - iyp * ci;
    if (li < imiss) { is += li; iyp += 1; } else { is += imiss; }
  }
  int je = js + jxp - 1, ie = is + iyp - 1;
  ext[0] = js; ext[1] = je; ext[2] = is; ext[3] = ie;
  ext[4] = js; ext[5] = (je == jx && !band) ? je - 1 : je;
  ext[6] = is; ext[7] = (ie == iy && !crm) ? ie - 1 : ie;
  bdy[0] = (lj == 0) && !band; bdy[1] = (lj == cj - 1) && !band;
  bdy[2] = (li == 0) && !crm; bdy[3] = (li == ci - 1) && !crm;
}

Geom make_geom(int jx, int iy, int cj, int ci, int tile, int gh = G, int band = 0, int crm = 0) {
  int ext[8], bdy[4];
  tile_extent(jx, iy, cj, ci, tile, ext, bdy, band, crm);
  Geom g{};
  g.bl = bdy[0]; g.br = bdy[1]; g.bb = bdy[2]; g.bt = bdy[3];
  g.band = band;
  g.crm = crm;
  g.gjx = jx; g.giy = iy;
  g.jde1 = g.jdi1 = g.jdii1 = ext[0]; g.jde2 = g.jdi2 = g.jdii2 = ext[1];
  g.ide1 = g.idi1 = g.idii1 = ext[2]; g.ide2 = g.idi2 = g.idii2 = ext[3];
  if (g.bl) { g.jdi1 = g.jde1 + 1; g.jdii1 = g.jde1 + 2; }
  if (g.br) { g.jdi2 = g.jde2 - 1; g.jdii2 = g.jde2 - 2; }
  if (g.bb) { g.idi1 = g.ide1 + 1; g.idii1 = g.ide1 + 2; }
  if (g.bt) { g.idi2 = g.ide2 - 1; g.idii2 = g.ide2 - 2; }
  g.jce1 = g.jci1 = g.jcii1 = ext[4]; g.jce2 = g.jci2 = g.jcii2 = ext[5];
  g.ice1 = g.ici1 = g.icii1 = ext[6]; g.ice2 = g.ici2 = g.icii2 = ext[7];
  if (g.bl) { g.jci1 = g.jce1 + 1; g.jcii1 = g.jce1 + 2; }
  if (g.br) { g.jci2 = g.jce2 - 1; g.jcii2 = g.jce2 - 2; }
  if (g.bb) { g.ici1 = g.ice1 + 1; g.icii1 = g.ice1 + 2; }
  if (g.bt) { g.ici2 = g.ice2 - 1; g.icii2 = g.ice2 - 2; }
  int gl = g.bl ? 0 : 1, gr = g.br ? 0 : 1, gb = g.bb ? 0 : 1, gt = g.bt ? 0 : 1;
  g.jde1ga = g.jde1 - gl; g.jde2ga = g.jde2 + gr; g.ide1ga = g.ide1 - gb; g.ide2ga = g.ide2 + gt;
  g.jce1ga = g.jce1 - gl; g.jce2ga = g.jce2 + gr; g.ice1ga = g.ice1 - gb; g.ice2ga = g.ice2 + gt;
  g.jci1ga = g.jci1 - gl; g.jci2ga = g.jci2 + gr; g.ici1ga = g.ici1 - gb; g.ici2ga = g.ici2 + gt;
  g.jde1gb = g.jde1 - 2 * gl; g.jde2gb = g.jde2 + 2 * gr; g.ide1gb = g.ide1 - 2 * gb; g.ide2gb = g.ide2 + 2 * gt;
  g.jce1gb = g.jce1 - 2 * gl; g.jce2gb = g.jce2 + 2 * gr; g.ice1gb = g.ice1 - 2 * gb; g.ice2gb = g.ice2 + 2 * gt;
  g.j0 = g.jde1 - gh; g.i0 = g.ide1 - gh;
  g.nj = (g.jde2 - g.jde1 + 1) + 2 * gh;
  g.ni = (g.ide2 - g.ide1 + 1) + 2 * gh;
  g.pitch = (g.nj + 15) / 16 * 16;
  g.plane = (long)g.pitch * g.ni;
  g.P8 = (uint32_t)g.pitch * 8u;
  g.L8 = (uint32_t)(g.plane * 8);
  return g;
}

// setup_boundaries, Main/mod_atm_interface.F90:383-542 (global indices).  A band (i_band = 1,
// :435-455) has the south and north bands only, over every j.
void setup_boundaries(const Geom& g, int jx, int iy, int nsp, bool ldot, std::vector<int8_t>& rg,
                      std::vector<int16_t>& ib) {
  int icx = ldot ? 0 : 1, icy = ldot ? 0 : 1;
  int igbb1 = 2, igbb2 = nsp - 1, jgbl1 = 2, jgbl2 = nsp - 1;
  int igbt1 = iy - icy - nsp + 2, igbt2 = iy - icy - 1;
  int jgbr1 = jx - icx - nsp + 2, jgbr2 = jx - icx - 1;
  rg.assign(g.plane, 0);
  ib.assign(g.plane, -1);
  auto set = [&](int j, int i, int r, int b) { rg[g.ix(j, i)] = (int8_t)r; ib[g.ix(j, i)] = (int16_t)b; };
  // every frame point of the global domain (owned and ghost): the masks are functions of the
  // global index, so ghost points carry their owners' values
  const int fi1 = std::max(1, g.i0), fi2 = std::min(iy, g.i0 + g.ni - 1);
  const int fj1 = std::max(1, g.j0), fj2 = std::min(jx, g.j0 + g.nj - 1);
  if (g.crm) return;            // CRM: no relaxation band at all (:434, "if (.not. ma%crmflag)")
  if (g.band) {
    // periodic ghosts carry the band rows too
    for (int i = fi1; i <= fi2; i++)
      for (int j = g.j0; j < g.j0 + g.nj; j++) {
        if (i >= igbb1 && i <= igbb2) set(j, i, 1, i - igbb1 + 2);
        if (i >= igbt1 && i <= igbt2) set(j, i, 2, igbt2 - i + 2);
      }
    return;
  }
  for (int i = fi1; i <= fi2; i++)
    if (i >= igbb1 && i <= igbb2)
      for (int j = fj1; j <= fj2; j++)
        if (j >= jgbl1 && j <= jgbr2) {
          if (j <= jgbl2 && i >= j) continue;
          if (j >= jgbr1 && i >= (jgbr2 - j + 2)) continue;
          set(j, i, 1, i - igbb1 + 2);
        }
  for (int i = fi1; i <= fi2; i++)
    if (i >= igbt1 && i <= igbt2)
      for (int j = fj1; j <= fj2; j++)
        if (j >= jgbl1 && j <= jgbr2) {
          if (j <= jgbl2 && (igbt2 - i + 2) >= j) continue;
          if (j >= jgbr1 && (igbt2 - i) >= (jgbr2 - j)) continue;
          set(j, i, 2, igbt2 - i + 2);
        }
  for (int i = fi1; i <= fi2; i++) {
    if (i < igbb1 || i > igbt2) continue;
    for (int j = fj1; j <= fj2; j++)
      if (j >= jgbl1 && j <= jgbl2) {
        if (i < igbb2 && j > i) continue;
        if (i > igbt1 && j > (igbt2 - i + 2)) continue;
        set(j, i, 3, j - jgbl1 + 2);
      }
  }
  for (int i = fi1; i <= fi2; i++) {
    if (i < igbb1 || i > igbt2) continue;
    for (int j = fj1; j <= fj2; j++)
      if (j >= jgbr1 && j <= jgbr2) {
        if (i < igbb2 && (jgbr2 - j + 2) > i) continue;
        if (i > igbt1 && (jgbr2 - j) > (igbt2 - i)) continue;
        set(j, i, 4, jgbr2 - j + 2);
      }
  }
}

// Launch with an optional HIP event pair around the kernel (rcmdyn_kernel_times).
#define KLAUNCH(kern, ...) KLAUNCH_AS(#kern, kern, __VA_ARGS__)
// the same under a given name: the instances of one kernel (optset.hpp) report one name
#define KLAUNCH_AS(name, kern, ...)                         \
  do {                                                      \
    if (dry) break;                                         \
    hipEvent_t e0_ = prof ? prof->begin(stream) : nullptr;  \
    hipLaunchKernelGGL(kern, __VA_ARGS__);                  \
    if (prof) prof->end(stream, name, e0_);                 \
  } while (0)
// a stream-path HIP call that a plan-only engine (rcmdyn_exchange_plan) skips
#define DHIPCHK(x)           \
  do {                       \
    if (!dry) HIPCHK(x);     \
  } while (0)

// per-launch event pairs, aggregated by kernel name after the run
struct KernelProf {
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> rec;
  hipEvent_t get() {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) throw std::runtime_error("rcmdyn: hipEventCreate failed");
      pool.push_back(e);
    }
    return pool[used++];
  }
  hipEvent_t begin(hipStream_t s) {
    hipEvent_t e = get();
    (void)hipEventRecord(e, s);
    return e;
  }
  void end(hipStream_t s, const char* name, hipEvent_t e0) {
    hipEvent_t e1 = get();
    (void)hipEventRecord(e1, s);
    rec.push_back({name, {e0, e1}});
  }
  ~KernelProf() {
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  }
};

inline dim3 grid3(int nj, int ni, int nk) { return dim3((nj + 63) / 64, (ni + 3) / 4, nk); }
const dim3 BLK(64, 4, 1);

}  // namespace

// Buffers that exchanges refer to, resolved per tile.
enum class FK {
  A1U, A1V, A1T, A1QV, A1QC, A2U, A2V, A2T, A2QV, A2QC, PSA, PSB, PSDOTA, PSDOTB,
  RPSDA, RPSDB, QDOT, CQV, CQC, PHI, UU, VV, DHSUM, DELH, MSFX, MSFD, HT, CORIOL,
  UB0, UBT, VB0, VBT, TB0, TBT, QB0, QBT, PB0, PBT, DSTOR, HSTOR,
  // non-hydrostatic core
  A1PP, A2PP, A1W, A2W, NCR, NXKCR, NCDT, NCPP, NCU, NCV,
  // device bdyin: coupled boundary data at the interval end
  UB1, VB1, TB1, QB1, PB1, PPB1, WWB1,
  // semi-Lagrangian moisture tendency starts
  SLQV, SLQC,
  // UW PBL TKE (ibltyp = 2)
  A1TKE, A2TKE,
  // idiffu = 3 column terms
  D6U, D6V, D6T, D6QV, D6QC,
  // nqx = 5: the hydrometeors beyond qc (qi, qr, qs), each kind in species order
  A1QX0, A1QX1, A1QX2, A2QX0, A2QX1, A2QX2, CQX0, CQX1, CQX2, SLQX0, SLQX1, SLQX2, D6QX0, D6QX1, D6QX2,
  // iuwvadv = 1: the PBL-top level (2-D)
  KPBL,
  // chemical tracers (rcmdyn_set_tracers): chia, chib, the forecast, chib0, chibt of tracer XField::n
  TRA1, TRA2, TRCQ, TRB0, TRBT,
  // SUBEX on the device (rcmdyn_set_subex): rh0adj and the rain columns' increments for the rings
  SBX_RH0ADJ, SBX_LSCT, SBX_LSCQV, SBX_LSCQC
};
inline FK fkq(FK base, int n) { return (FK)((int)base + n); }

// The run-time switches, read from the environment by read() alone, once per engine
// at the start of create(): engines built under different environments in one process keep their own.
struct Switches {
  // steps per replayed graph in rcmdyn_step (RCMDYN_GRAPH_STEPS, 1 or 2): two steps per launch
  // return to the same ping-pong parity and halve the graph launches
  int graph_steps = 2;
  // RCMDYN_NO_GRAPH=1 runs rcmdyn_step eagerly (the path of RCCL-decomposed runs), for timing
  bool no_graph = false;
  // k_momentum and k_scalars as one launch (k_update); RCMDYN_NO_FUSE_UPDATE=1: two launches
  bool fuse_update = true;
  // NH: tend's time filters of t, qv, qc in k_nh_tend_c and the negative-moisture fix, into
  // the other parity (Tile::tq); RCMDYN_NH_NO_TFUSE=1: in place in k_nh_tfilter_a1
  bool nh_tfuse = true;
  // rcmdyn_step's hydrostatic bdyval runs inside k_split_correct_bdy (RCMDYN_NO_FUSE_BDY: two
  // launches of its own, as after rcmdyn_tend)
  bool no_fuse_bdy = false;
  // the drop-in pair (rcmdyn_tend, then rcmdyn_bdyval): tend leaves its split corrections
  // pending and bdyval launches them with its boundary lines (k_split_correct_bdy, the form of
  // rcmdyn_step); any other call in between launches them alone first (settle).
  // RCMDYN_NO_DEFER_CORR=1: tend launches them itself.
  bool no_defer_corr = false;
  // lazy tend (drop-in pair): rcmdyn_tend does the host bookkeeping and leaves the launch to
  // the next call: rcmdyn_bdyval replays the one-step graph of tend + bdyval (rcmdyn_step's),
  // any other call (settle) replays tend's own graph first.  RCMDYN_NO_LAZY_TEND=1: off
  bool lazy_tend = true;
  // the hydrostatic step without k_qfilter (its work in k_columns, k_scalars and the extra
  // blocks of k_split_project / k_split_correct); RCMDYN_NO_QFUSE=1 launches k_qfilter
  bool no_qfuse = false;
  // halo/compute overlap of the hydrostatic prologue exchange (Part, kernels.hpp) on a
  // decomposed domain; RCMDYN_NO_OVERLAP=1: the atm1/p* part first, then the atm2 part beside
  // k_columns only
  bool no_overlap = false;
  // RCMDYN_NO_OPTSET (present): the generic instances of k_momentum, k_scalars and k_update
  // everywhere, also where the default-set ones would fit (optset.hpp)
  bool no_optset = false;
  // RCMDYN_FORCE_RCCL=1: the halo messages between tiles held by this engine travel as RCCL
  // sends/receives to itself (one-rank communicator), not as device copies
  bool force_rccl = false;
  // RCMDYN_NEGFIX_MODE=1 (tests): the row sweep for every marked plane, dense ones included
  int negfix_mode = 0;
  // fault injection for the tests (RCMDYN_INJECT_LAUNCH_FAILURE=n): the n-th launch of a lazy
  // tend's graph fails before it is issued, as a failed hipGraphLaunch would
  int inject_launch_failure = 0;
  static Switches read() {
    // the two rules by which a switch counts as set: its variable exists, or holds something but "" and "0"
    auto present = [](const char* name) { return std::getenv(name) != nullptr; };
    auto nonzero = [](const char* name) { const char* v = std::getenv(name); return v && *v && std::strcmp(v, "0") != 0; };
    auto number = [](const char* name, int unset) { const char* v = std::getenv(name); return v ? std::atoi(v) : unset; };
    Switches s;
    s.graph_steps = std::max(1, std::min(2, number("RCMDYN_GRAPH_STEPS", 2)));
    s.no_graph = present("RCMDYN_NO_GRAPH");
    s.fuse_update = !present("RCMDYN_NO_FUSE_UPDATE");
    s.nh_tfuse = !present("RCMDYN_NH_NO_TFUSE");
    s.no_fuse_bdy = nonzero("RCMDYN_NO_FUSE_BDY");
    s.no_defer_corr = present("RCMDYN_NO_DEFER_CORR");
    s.lazy_tend = !present("RCMDYN_NO_LAZY_TEND");
    s.no_qfuse = nonzero("RCMDYN_NO_QFUSE");
    s.no_overlap = nonzero("RCMDYN_NO_OVERLAP");
    s.no_optset = optset_disabled_by_env();
    s.force_rccl = present("RCMDYN_FORCE_RCCL");
    s.negfix_mode = number("RCMDYN_NEGFIX_MODE", 0);
    s.inject_launch_failure = number("RCMDYN_INJECT_LAUNCH_FAILURE", 0);
    return s;
  }
};

struct rcmdyn_engine {
  rcmdyn_config cfg{};
  Consts hc{};
  Consts* dc = nullptr;
  StepState* ds = nullptr;
  StepState hs{};            // host mirror of the time state
  int ntiles = 0;
  std::vector<Geom> all;     // every tile of the decomposition
  std::vector<Tile> tiles;   // tiles owned here
  hipStream_t stream = nullptr;
  Switches sw;
  // tend in two phases split where the reference calls physical_parametrizations
  // (Main/mod_tendency.F90:271): TEND_PRE runs surface_pressures .. new_pressure (and the
  // mkslice export when `slice`), TEND_POST the rest; a step runs both.
  static constexpr int TEND_PRE = 1, TEND_POST = 2, TEND_ALL = 3;
  // what a tend does with its split corrections: launch them, launch them with bdyval's
  // boundary lines (k_split_correct_bdy: the bdyval that follows skips those), or leave them
  // to the next call
  enum class Corr { Launch, WithBdy, Defer };
  // the replay graphs, each captured per ping-pong parity (gpar)
  enum class Graph {
    Step,        // tend + bdyval (rcmdyn_step; a lazy tend with its rcmdyn_bdyval)
    TwoSteps,    // (tend + bdyval) x 2
    Tend,        // tend alone (the drop-in rcmdyn_tend), its corrections deferred where can_defer()
    Bdyval,      // bdyval alone (rcmdyn_bdyval)
    CorrBdyval,  // rcmdyn_bdyval with the deferred corrections
    Count
  };
  hipGraphExec_t graphs[(int)Graph::Count][2] = {};
  // what of the last rcmdyn_tend is not launched yet: the whole tend (a lazy tend: only its host
  // bookkeeping is done; recorded for the parity pend_par), or its split corrections.
  //   tend_call / tend_post_physics: None -> Tend or Corrections (or None: nothing deferred)
  //   settle (any call but rcmdyn_bdyval): Tend -> Corrections -> None
  //   bdyval_call: Tend -> None (the Step graph), Corrections -> None (with the boundary lines)
  // A transition happens only once its launch succeeded: a failed one leaves the state as it was.
  enum class Pending { None, Tend, Corrections };
  Pending pend = Pending::None;
  int pend_par = 0;
  // step error flags: host-mapped snapshot ring written by the last launch of every tend,
  // one event per slot; the host checks a step's flags once its event completed and keeps
  // at most FLAG_LAG steps unchecked, so no entry point synchronises the stream per step
  FlagSnap* hflags = nullptr;
  FlagSnap* dflags = nullptr;
  hipEvent_t fev[NFLAGSLOT] = {};
  std::deque<long long> pending;
  static constexpr int FLAG_LAG = 2;
  // with a communicator the flags are max-reduced over the ranks every GLOBAL_EVERY steps
  // (and at the end of every rcmdyn_step) and only the reduced word raises the error, so
  // every rank stops at the same step -- the reference's fatal aborts the whole job
  // (Main/abort.F90:20-36); a rank stopping alone would leave its neighbours waiting
  static constexpr int GLOBAL_EVERY = 8;
  int32_t* derr = nullptr;
  int32_t* hgerr = nullptr;
  int32_t* dgerr = nullptr;
  hipEvent_t gev[NFLAGSLOT] = {};
  std::deque<std::pair<long long, int>> gpending;   // (step, slot)
  int gslot = 0;
  bool statics_dirty = true;
  bool bdy_dirty = true;
  bool dprd_put = false;      // NH: a dprddx / dprddy check is pending (check_dprd); sticky until it passes
  bool dprd_any = false;      // NH: dprddx / dprddy were put (a later atm0%pr put re-arms the check)
  bool kpbl_dirty = false;    // kpbl put since the last tend: its ghost ring is stale
  bool ghosts_stale = true;   // state put since the last tend: ghost rings are not step results
  bool capturing = false;
  long slen = 0;
  long staging_cap = 0;
  double* red = nullptr;     // noise-sum partials of every tile (k_columns)
  int red_total = 0;
  bool halo = false;          // ghost rings come from exchanges: a decomposition, or a band (periodic in j)
  bool diag = false;         // write the per-tend diagnostic fields
  // tendency budget of t and qv (rcmdyn_set_budget): on, and the host's alarm_out_atm%rw
  bool budget = false;
  double bud_rw = 1.0;
  Budget budget_args(const Tile& t) const {
    Budget b{};
    for (int q = 0; q < NBUDTERM; q++) { b.t[q] = t.bud[q]; b.q[q] = t.bud[NBUDTERM + q]; }
    b.rw = bud_rw;
    return b;
  }
  // SUBEX condensation inside tend (rcmdyn_set_condtq; condtq.hpp): the switch, subexparam's
  // conf, and whether one put of the host covered rh0adj wherever condtq runs since the switch-on
  bool condtq = false, rh0_put = false;
  double ct_conf = 1.0;
  // with subex on as well, condtq reads the device's rh0adj of the same tend
  Condtq condtq_args(const Tile& t) const {
    return Condtq{subex ? t.sbx[RCMDYN_SUBEX_RH0ADJ] : t.rh0adj, t.cti[0], t.cti[1], t.cti[2], ct_conf};
  }
  // The extra argument blocks of a tendency launch (kernels.hpp): fn(blocks...) with those that
  // are switched on, Budget before Condtq.  fn is a generic lambda that issues the launch of the
  // instance its arguments name, so a further switch is one more rung here for every kernel.
  template <class F>
  void with_extras(const Tile& t, F&& fn) const {
    if (condtq && budget) fn(budget_args(t), condtq_args(t));
    else if (condtq) fn(condtq_args(t));
    else if (budget) fn(budget_args(t));
    else fn();
  }
  // the name an instance reports to the kernel-time profile: every instance the kernel's plain
  // name, the budget ones (with or without condtq) the name they always had
  template <class... B>
  static const char* tend_name(const char* plain, const char* bud) { return pack_has<Budget, B...> ? bud : plain; }
  void condtq_ready(const char* who) const {
    if (condtq && !rh0_put && !subex)
      throw std::runtime_error(std::string(who) + ": condtq is on and no rh0adj was put since that covers the tiles' interior "
                               "cross points and their rings on every level (rcmdyn_put_rh0adj)");
  }
  // mass check of tend (rcmdyn_set_massck; massck.hip): the switch, the ring's capacity, the
  // tiles' slots with k_massck_final's table of them, the device log (its counter, then the
  // records) and the counter's value at the host's last read
  bool massck = false;
  int mck_cap = 0;
  std::vector<MassckTile> mck_lay;
  double* mck_part = nullptr;
  MassckTile* mck_tab = nullptr;
  double* mck_log = nullptr;
  long long mck_seen = 0;
  KernelProf* prof = nullptr;  // set while rcmdyn_kernel_times runs
  double last_ms = 0.0;
  // parity of t, qv, qc: the step's ping-pong (hydrostatic), Tile::tq (NH)
  int thp(const Tile& t) const { return cfg.idynamic == 2 ? t.tq : t.cur; }
  // the parity the step graphs are captured for
  int gpar() const { return thp(tiles[0]); }
  int inject_fail = 0;        // launches of a lazy tend's graph left before the injected failure
  bool qfuse() const { return cfg.idynamic != 2 && !sw.no_qfuse; }
  // nqx = 5, hydrostatic qfuse: the species' serial fix joins the qv / qc one after the split
  // corrections (k_negfix_serial_qx)
  bool serial_with_corr() const { return qfuse() && hc.nsp > 0; }
  // halo/compute overlap of the hydrostatic prologue exchange (Switches::no_overlap; idiffu = 3:
  // the column terms are formed after the whole exchange, so no overlap)
  bool overlap() const { return halo && cfg.idynamic != 2 && cfg.idiffu != 3 && !sw.no_overlap; }
  std::string err;
  std::unique_ptr<Comm> comm;
  int device = 0;
  // halo/compute overlap: the second stream carries the atm2 part of the prologue exchange
  // while the first computes what needs only atm1 and p* (xch_begin / xch_join)
  hipStream_t stream2 = nullptr;
  // two exchanges may be in flight on the second stream at once (joined separately, slot 0/1)
  hipEvent_t evfork = nullptr, evjoin[2] = {nullptr, nullptr};
  bool join_pending[2] = {false, false};
  bool on2 = false;           // an exchange is being issued on stream2 (its staging buffers)
  // plan-only engine (rcmdyn_exchange_plan): host logic only, no device call; the exchanges and
  // collectives a rank would issue are logged by a PlanComm
  bool dry = false;

  std::vector<NHFields> nhf;   // non-hydrostatic buffers of each owned tile (idynamic = 2)
  double* nh_gbuf = nullptr;   // global-indexed day-alarm terms of the radiative condition

  int nsplit() const { return cfg.nsplit; }

  // ------------------------------------------------------------------ setup
  void compute_constants() {
    Consts& c = hc;
    std::memset(&c, 0, sizeof(c));
    c.kz = cfg.kz; c.nsplit = cfg.nsplit; c.iboudy = cfg.iboudy; c.nspgx = cfg.nspgx;
    c.stability_enhance = cfg.stability_enhance; c.present_qc = cfg.present_qc;
    const double rgasmol = NAVGDR * BOLTZK;
    c.c287 = rgasmol / AMD; c.rgas = c.c287 * 1000.0; c.cpd = 3.5 * c.rgas;
    c.ep1 = AMD / AMW - 1.0; c.regrav = 1.0 / EGRAV;
    c.rovcp = c.rgas * (1.0 / c.cpd);                        // Share/mod_constants.F90:183-184
    c.ipgf = cfg.ipgf;
    c.isladvec = cfg.isladvec; c.iqmsl = cfg.iqmsl;
    c.idiffu = cfg.idiffu;
    c.pgfaa1 = 6.5e-3 * c.rgas * c.regrav;                  // Share/mod_constants.F90:359-362
    c.dx = cfg.ds * 1000.0; c.dx2 = 2.0 * c.dx; c.dx4 = 4.0 * c.dx; c.dx8 = 8.0 * c.dx;
    c.dx16 = 16.0 * c.dx; c.dxsq = c.dx * c.dx; c.rdxsq = 1.0 / c.dxsq;
    c.ptop = cfg.ptop; c.dtsec = cfg.dtsec; c.gnu1 = cfg.gnu1; c.gnu2 = cfg.gnu2;
    c.t_extrema = cfg.t_extrema; c.q_rel_extrema = cfg.q_rel_extrema;
    const int kz = cfg.kz;
    for (int k = 1; k <= kz + 1; k++) c.sigma[k] = cfg.sigma[k - 1];
    for (int k = 1; k <= kz; k++) {
      c.hsigma[k] = (c.sigma[k + 1] + c.sigma[k]) * 0.5;
      c.dsigma[k] = (c.sigma[k + 1] - c.sigma[k]);
    }
    for (int k = 2; k <= kz; k++) {                         // Main/mod_params.F90:2208-2215
      c.twt1[k] = (c.sigma[k] - c.hsigma[k - 1]) / (c.hsigma[k] - c.hsigma[k - 1]);
      c.twt2[k] = 1.0 - c.twt1[k];
      c.qcon[k] = (c.sigma[k] - c.hsigma[k]) / (c.hsigma[k - 1] - c.hsigma[k]);
    }
    for (int k = 1; k <= kz; k++) c.xds[k] = 1.0 / c.dsigma[k];  // Main/mod_advection.F90:100
    // :106 (init dt).  upstream_mode = .false. selects the centred branches of hadvuv, hadvt,
    // hadv3d, hadvqv, hadvqx (Main/mod_advection.F90:141-201, 322-335, 409-460, 532-545,
    // 624-637): each is the upstream expression with ul = 0, term for term -- (1 + 0) a +
    // (1 - 0) b evaluates to exactly a + b, f1 = f2 = ff1..ff4 = +-0 -- so ul = 0 is the
    // centred scheme bit for bit
    c.ul = cfg.upstream_mode ? cfg.uoffc * 0.5 * cfg.dtsec / c.dx : 0.0;
    c.xkhmax = c.dxsq / (64.0 * cfg.dtsec);                          // Main/mod_diffusion.F90:104
    c.dydc = cfg.adyndif * VONKAR * VONKAR * c.dx * 0.25;
    c.diff6 = 0.12 * 0.015625 / (2.0 * cfg.dtsec);                    // Main/mod_diffusion.F90:78, 154
    c.xkhz = cfg.ckh * 1.5e-3 * c.dxsq / cfg.dtsec;
    const double fnudge = (cfg.bdy_nm > 0) ? cfg.bdy_nm : 0.1 / cfg.dtsec;   // Main/mod_bdycod.F90:204-215
    const double gnudge = (cfg.bdy_dm > 0) ? cfg.bdy_dm : 1.0 / (cfg.dtsec * 50.0);
    for (int n = 2; n <= cfg.nspgx - 1 && n < MAXNSP; n++) {
      double xfun = (double)(cfg.nspgx - n) / (double)(cfg.nspgx - 2);
      c.fcx[n] = fnudge * xfun; c.gcx[n] = gnudge * xfun;
    }
    if (cfg.iboudy == 4) {                                  // Main/mod_bdycod.F90:237-250
      c.wgtd[2] = 0.20; c.wgtd[3] = 0.55; c.wgtd[4] = 0.80; c.wgtd[5] = 0.95;
      for (int n = 6; n <= cfg.nspgd - 1 && n < MAXNSP; n++) c.wgtd[n] = 1.0;
      c.wgtx[2] = 0.4; c.wgtx[3] = 0.7; c.wgtx[4] = 0.9;
      for (int n = 5; n <= cfg.nspgx - 1 && n < MAXNSP; n++) c.wgtx[n] = 1.0;
    }
    for (int k = 1; k <= kz; k++) {
      double an = (c.hsigma[k] < 0.4) ? cfg.high_nudge : (c.hsigma[k] < 0.8) ? cfg.medium_nudge : cfg.low_nudge;
      for (int n = 2; n <= cfg.nspgx - 1 && n < MAXNSP; n++) {
        double xfun = std::exp(-((double)(n - 2) / an));
        c.hefc[n][k] = fnudge * xfun; c.hegc[n][k] = gnudge * xfun;
      }
    }
    for (int l = 0; l < cfg.nsplit; l++) {
      for (int k = 0; k < kz; k++) {
        c.zmatx[l][k] = cfg.zmatx[l][k]; c.zmatxr[l][k] = cfg.zmatxr[l][k];
        c.am[l][k] = cfg.am[l][k]; c.tau[l][k] = cfg.tau[l][k];
      }
      c.an[l] = cfg.an[l]; c.hbar[l] = cfg.hbar[l]; c.aam[l] = cfg.aam[l]; c.dtau[l] = cfg.dtau[l];
      for (int k = 1; k <= kz + 1; k++) {                  // Main/mod_split.F90:343-353
        double sh = cfg.sigmah[k - 1], va = cfg.varpa1[l][k - 1];
        c.pdlog[l][k] = va * std::log(sh * cfg.pd + cfg.ptop);
        c.eps1[l][k] = va * sh / (sh * cfg.pd + cfg.ptop);
      }
    }
    c.pd = cfg.pd;
    c.negfix_mode = sw.negfix_mode;
    // non-hydrostatic core: diffusion constants (Main/mod_diffusion.F90:108-113), sound
    c.idynamic = cfg.idynamic;
    if (cfg.idynamic == 2) {
      c.xkhz = cfg.ckh * c.dx;
      c.xkhmax = 2.0 * c.xkhmax;
      c.ifupr = cfg.ifupr; c.ifrayd = cfg.ifrayd; c.rayndamp = cfg.rayndamp; c.crm = cfg.i_crm;
      c.rayalpha0 = cfg.rayalpha0; c.rayhd = cfg.rayhd; c.nhbet = cfg.nhbet; c.nhxkd = cfg.nhxkd;
      c.nh_dtsmax = cfg.nh_dtsmax; c.nh_xmsf = cfg.nh_xmsf;
      c.xgamma = 1.0 / (1.0 - c.rgas * (1.0 / c.cpd));           // Main/mod_sound.F90:77
    }
    c.dds[1] = 0.0; c.dds[kz + 1] = 0.0;                            // Main/mod_advection.F90:101-105
    for (int k = 2; k <= kz; k++) c.dds[k] = 1.0 / (c.dsigma[k] + c.dsigma[k - 1]);
    c.ibltyp = cfg.ibltyp; c.nuk = cfg.nuk; c.tkemin = cfg.tkemin;
    c.iqxvadv = (cfg.ibltyp == 2 && cfg.iuwvadv == 1) ? 3 : 1;
    c.ipptls = cfg.ipptls; c.nqx = cfg.nqx; c.nsp = cfg.nqx - 2;
  }

  // n zeroed T of device memory on an owner list: Tile::allocs lives as long as the tile,
  // Tile::tr_allocs until rcmdyn_set_tracers(0).  Null on a dry engine.
  template <class T>
  T* zalloc(std::vector<void*>& owner, size_t n) {
    if (dry) return nullptr;
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, n * sizeof(T)));
    owner.push_back(p);
    HIPCHK(hipMemset(p, 0, n * sizeof(T)));
    return (T*)p;
  }
  double* dalloc(Tile& t, size_t n) { return zalloc<double>(t.allocs, n); }
  template <class T> T* talloc(Tile& t, size_t n) { return zalloc<T>(t.allocs, n); }
  template <class T> T* tr_alloc(Tile& t, size_t n) { return zalloc<T>(t.tr_allocs, n); }

  void setup_tile(Tile& t, int index) {
    t.index = index;
    t.lj = index / cfg.nproc_i; t.li = index % cfg.nproc_i;
    t.g = all[index];
    const Geom& g = t.g;
    const int kz = cfg.kz, ns = cfg.nsplit;
    const size_t P = g.plane, P3 = P * kz;
    // neighbours L, R, B, T, BL, BR, TL, TR
    const int dj[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, di[8] = {0, 0, -1, 1, -1, -1, 1, 1};
    for (int d = 0; d < 8; d++) {
      int lj = t.lj + dj[d], li = t.li + di[d];
      if (cfg.i_band) lj = (lj + cfg.nproc_j) % cfg.nproc_j;      // periodic in j (a tile may be its own)
      if (cfg.i_crm) li = (li + cfg.nproc_i) % cfg.nproc_i;       // CRM: periodic in i too
      t.nbr[d] = (lj >= 0 && lj < cfg.nproc_j && li >= 0 && li < cfg.nproc_i) ? lj * cfg.nproc_i + li : -1;
    }
    for (int b = 0; b < 2; b++) {
      t.a1u[b] = dalloc(t, P3); t.a1v[b] = dalloc(t, P3); t.a1t[b] = dalloc(t, P3);
      t.a1qv[b] = dalloc(t, P3); t.a1qc[b] = dalloc(t, P3);
      t.a2u[b] = dalloc(t, P3); t.a2v[b] = dalloc(t, P3); t.a2t[b] = dalloc(t, P3);
      t.a2qv[b] = dalloc(t, P3); t.a2qc[b] = dalloc(t, P3);
    }
    for (int b = 0; b < 2; b++) { t.psa_[b] = dalloc(t, P); t.psb_[b] = dalloc(t, P); }
    t.dstor = dalloc(t, P * ns); t.hstor = dalloc(t, P * ns);
    t.msfx = dalloc(t, P); t.msfd = dalloc(t, P); t.coriol = dalloc(t, P); t.ht = dalloc(t, P);
    t.xmsf = dalloc(t, P); t.dmsf = dalloc(t, P); t.hgfact = dalloc(t, P); t.mapf = dalloc(t, P);
    t.rgcr = talloc<int8_t>(t, P); t.rgdt = talloc<int8_t>(t, P);
    t.ibcr = talloc<int16_t>(t, P); t.ibdt = talloc<int16_t>(t, P);
    t.ub0 = dalloc(t, P3); t.ubt = dalloc(t, P3); t.vb0 = dalloc(t, P3); t.vbt = dalloc(t, P3);
    t.tb0 = dalloc(t, P3); t.tbt = dalloc(t, P3); t.qb0 = dalloc(t, P3); t.qbt = dalloc(t, P3);
    t.pb0 = dalloc(t, P); t.pbt = dalloc(t, P);
    t.rpsa = dalloc(t, P); t.rpsb = dalloc(t, P); t.rpsda = dalloc(t, P); t.rpsdb = dalloc(t, P);
    t.psc = dalloc(t, P); t.psdota = dalloc(t, P); t.psdotb = dalloc(t, P); t.pten = dalloc(t, 2 * P);
    t.qdot = dalloc(t, P * (kz + 1));
    t.phi = dalloc(t, P3);
    if (cfg.isladvec == 1) { t.slqv = dalloc(t, P3); t.slqc = dalloc(t, P3); }
    if (cfg.idiffu == 3)
      for (int q = 0; q < (cfg.idynamic == 2 ? 7 : 5); q++) t.d6[q] = dalloc(t, P * (kz + 1));
    if (cfg.ibltyp == 2) {
      t.a1tke = dalloc(t, P * (kz + 1)); t.a2tke = dalloc(t, P * (kz + 1)); t.ctke = dalloc(t, P * (kz + 1));
      t.kpbl = dalloc(t, P);
    }
    t.cqv = dalloc(t, P3); t.cqc = dalloc(t, P3); t.fqv = dalloc(t, P3); t.fqc = dalloc(t, P3);
    for (int n = 0; n < hc.nsp; n++) {            // nqx = 5: qi, qr, qs (species.hip)
      for (int b = 0; b < (cfg.idynamic == 2 ? 1 : 2); b++) {     // the NH core: in place
        t.a1qx[n][b] = dalloc(t, P3);
        t.a2qx[n][b] = dalloc(t, P3);
      }
      t.cqx[n] = dalloc(t, P3); t.fqx[n] = dalloc(t, P3);
      if (cfg.isladvec == 1) t.slqx[n] = dalloc(t, P3);
      if (cfg.idiffu == 3) t.d6qx[n] = dalloc(t, P * (kz + 1));
    }
    if (hc.nsp) {
      t.depx = talloc<unsigned>(t, (size_t)hc.nsp * kz * negfix_rowwords(g));
      t.depxf = talloc<unsigned>(t, (size_t)hc.nsp * kz * (g.ici2 - g.ici1 + 1));
    }
    t.depplane = talloc<unsigned>(t, 2 * (size_t)kz * negfix_rowwords(g));
    t.depqf = talloc<unsigned>(t, 2 * (size_t)kz * (g.ici2 - g.ici1 + 1));
    if (cfg.idynamic != 2) {
      t.negcnt = talloc<int>(t, 1);
      t.neglist = talloc<uint32_t>(t, 2 * P3);     // every (point, level, qv|qc) at most once
    }
    t.deld = dalloc(t, P * 3 * ns); t.delh = dalloc(t, P * 3 * ns);
    t.ddsum = dalloc(t, P * ns); t.dhsum = dalloc(t, P * ns);
    t.uu = dalloc(t, P); t.vv = dalloc(t, P);
    t.tten = dalloc(t, P3); t.uten = dalloc(t, P3); t.vten = dalloc(t, P3);
    t.qvten = dalloc(t, P3); t.qcten = dalloc(t, P3); t.omega = dalloc(t, P3); t.xkcs = dalloc(t, P3);
    if (halo) {                       // wide frame of the fused split step
      t.gw = make_geom(cfg.jx, cfg.iy, cfg.nproc_j, cfg.nproc_i, index, SPH + G, cfg.i_band, cfg.i_crm);
      const size_t PW = t.gw.plane;
      t.wdeld = dalloc(t, PW * 3 * ns); t.wdelh = dalloc(t, PW * 3 * ns);
      t.wpsa = dalloc(t, PW); t.wpsdota = dalloc(t, PW);
      t.wmsfx = dalloc(t, PW); t.wmsfd = dalloc(t, PW); t.wmapf = dalloc(t, PW);
    }
    slen = std::max<long>(g.pitch, g.ni);
    for (int s = 0; s < 16; s++) t.sl[s] = dalloc(t, (size_t)slen * kz);
    // halo staging: 8 directions x widest exchange (the hydrostatic prologue: 5 fields 2 wide
    // + 5 fields 3 wide + p*; at most 32 field-widths of kz+1 levels; nqx = 5 adds 3 fields 2
    // wide + 3 fields 3 wide)
    staging_cap = std::max<long>(staging_cap, staging_need(g, 0));
    t.sbuf = dalloc(t, staging_cap);
    t.rbuf = dalloc(t, staging_cap);
    if (halo) {
      t.sbuf2 = dalloc(t, staging_cap);
      t.rbuf2 = dalloc(t, staging_cap);
    }
    // column blocks of k_columns (one noise partial each)
    // k_columns blocks: 64 columns x one row, over the tile and its ghost ring
    t.ncolx = (g.jdx2() - g.jdx1() + COLW) / COLW;
    t.nred = t.ncolx * (g.idx2() - g.idx1() + 1);
    if (overlap()) setup_overlap(t);
    t.red_off = red_total;
    red_total += t.nred;
    if (cfg.idynamic == 2) setup_nh(t);
    // boundary masks
    std::vector<int8_t> rg;
    std::vector<int16_t> ib;
    if (dry) return;
    // iboudy = 2 (time-dependent) and 3 (inflow/outflow) relax nothing (Main/mod_tendency.F90:
    // 1434-1510): an empty band turns every nudging and sponge branch of the kernels off
    const bool band = cfg.iboudy != 2 && cfg.iboudy != 3;
    setup_boundaries(g, cfg.jx, cfg.iy, cfg.nspgx, false, rg, ib);
    if (!band) std::fill(rg.begin(), rg.end(), (int8_t)0);
    HIPCHK(hipMemcpy(t.rgcr, rg.data(), P, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.ibcr, ib.data(), P * 2, hipMemcpyHostToDevice));
    setup_boundaries(g, cfg.jx, cfg.iy, cfg.nspgd, true, rg, ib);
    if (!band) std::fill(rg.begin(), rg.end(), (int8_t)0);
    HIPCHK(hipMemcpy(t.rgdt, rg.data(), P, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.ibdt, ib.data(), P * 2, hipMemcpyHostToDevice));
  }

  // non-hydrostatic buffers (kernels_nh.hpp NHFields); shared hydrostatic buffers are
  // filled per call by nhfields()
  void setup_nh(Tile& t) {
    const size_t P = t.g.plane, P3 = P * cfg.kz, P4 = P * (cfg.kz + 1);
    NHFields f{};
    for (double** p : {&f.a1pp, &f.a2pp, &f.pr1, &f.rho1, &f.cr, &f.xkcr, &f.ppten, &f.ct, &f.cu, &f.cv,
                       &f.cpp, &f.cdt, &f.se, &f.sf, &f.spi, &f.th})
      *p = dalloc(t, P3);
    f.neglist = talloc<unsigned>(t, 2 * P3);     // every interior point of both species at most once
    f.negcnt = talloc<int>(t, 1);
    for (double** p : {&f.a1w, &f.a2w, &f.wten, &f.cw})
      *p = dalloc(t, P4);
    f.ppb0 = dalloc(t, P3); f.ppbt = dalloc(t, P3); f.wwb0 = dalloc(t, P4); f.wwbt = dalloc(t, P4);
    f.pr0 = dalloc(t, P3); f.t0 = dalloc(t, P3); f.rho0 = dalloc(t, P3); f.z0 = dalloc(t, P3);
    f.dprddx = dalloc(t, P3); f.dprddy = dalloc(t, P3);
    f.pf0 = dalloc(t, P4); f.rhof0 = dalloc(t, P4); f.zf0 = dalloc(t, P4);
    f.ps0 = dalloc(t, P); f.dpsdxm = dalloc(t, P); f.dpsdym = dalloc(t, P);
    f.ef = dalloc(t, P); f.ddx = dalloc(t, P); f.ddy = dalloc(t, P); f.dmdx = dalloc(t, P); f.dmdy = dalloc(t, P);
    f.ex = dalloc(t, P); f.crx = dalloc(t, P); f.cry = dalloc(t, P);
    f.estore = dalloc(t, P); f.astore = dalloc(t, P);
    if (nhf.empty()) {                 // engine-wide: mask, CFL slots, day-alarm gather buffer
      f.tmask = dalloc(t, 169);
      f.cfl = talloc<unsigned long long>(t, NH_CFL_SLOTS);
      f.cfll = talloc<unsigned long long>(t, NH_CFL_SLOTS);
      nh_gbuf = dalloc(t, 2 * (size_t)cfg.jx * cfg.iy);
    } else {
      f.tmask = nhf[0].tmask;
      f.cfl = nhf[0].cfl;
      f.cfll = nhf[0].cfll;
    }
    if (halo) t.westore = dalloc(t, t.gw.plane);
    nhf.push_back(f);
  }

  TkeArgs tke_args(Tile& t) {
    const int c = t.cur;
    TkeArgs a{};
    a.a1u = t.a1u[c]; a.a1v = t.a1v[c]; a.msfd = t.msfd; a.xmsf = t.xmsf; a.psa = t.psa_[c]; a.rpsa = t.rpsa;
    a.qdot = t.qdot; a.tkephy = t.tkephy; a.a1tke = t.a1tke; a.a2tke = t.a2tke; a.ctke = t.ctke;
    a.psb = t.psb_[c];
    if (cfg.idynamic == 2) { a.xk = nhf[&t - tiles.data()].xkcr; a.xkpb = t.psb_[t.cur]; a.xk_half = 0; }
    else { a.xk = t.xkcs; a.xk_half = 1; }
    return a;
  }
  // the TKE forecast and filter of tend (Main/mod_tendency.F90:515-544), after the kernels
  // that produce qdot and the diffusion coefficients
  void tke_step() {
    if (cfg.ibltyp != 2) return;
    each([&](Tile& t) {
      const Geom& g = t.g;
      const dim3 grid = grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, cfg.kz + 1);
      KLAUNCH(k_tke_tend, grid, BLK, 0, stream, g, dc, ds, tke_args(t));
      KLAUNCH(k_tke_filter, grid, BLK, 0, stream, g, dc, tke_args(t));
    });
  }
  // the TKE boundary lines of bdyval, once the boundary-wind slices are current
  void tke_bdyval() {
    if (cfg.ibltyp != 2) return;
    each([&](Tile& t) {
      Slices sl;
      for (int q = 0; q < 16; q++) sl.s[q] = t.sl[q];
      KLAUNCH(k_bdyval_tke, dim3(cfg.kz + 1), dim3(256), 0, stream, t.g, dc, ds, tke_args(t), sl, slen);
    });
  }

  NHFields nhfields(Tile& t) {
    NHFields f = nhf[&t - tiles.data()];
    const int c = t.cur, q = thp(t), o = 1 - q;
    f.a1u = t.a1u[c]; f.a1v = t.a1v[c]; f.a1t = t.a1t[q]; f.a1qv = t.a1qv[q]; f.a1qc = t.a1qc[q];
    f.a2u = t.a2u[c]; f.a2v = t.a2v[c]; f.a2t = t.a2t[q]; f.a2qv = t.a2qv[q]; f.a2qc = t.a2qc[q];
    f.b1t = t.a1t[o]; f.b1qv = t.a1qv[o]; f.b1qc = t.a1qc[o];
    f.b2t = t.a2t[o]; f.b2qv = t.a2qv[o]; f.b2qc = t.a2qc[o];
    f.tfuse = sw.nh_tfuse ? 1 : 0;
    f.psa = t.psa_[c]; f.psb = t.psb_[c];
    f.msfx = t.msfx; f.msfd = t.msfd; f.coriol = t.coriol; f.ht = t.ht; f.xmsf = t.xmsf; f.dmsf = t.dmsf;
    f.hgfact = t.hgfact; f.rgcr = t.rgcr; f.rgdt = t.rgdt; f.ibcr = t.ibcr; f.ibdt = t.ibdt;
    f.ub0 = t.ub0; f.ubt = t.ubt; f.vb0 = t.vb0; f.vbt = t.vbt; f.tb0 = t.tb0; f.tbt = t.tbt;
    f.qb0 = t.qb0; f.qbt = t.qbt;
    f.rpsa = t.rpsa; f.rpsb = t.rpsb; f.rpsda = t.rpsda; f.rpsdb = t.rpsdb; f.psdota = t.psdota;
    f.psdotb = t.psdotb; f.qdot = t.qdot;
    f.tten = t.tten; f.qvten = t.qvten; f.qcten = t.qcten; f.uten = t.uten; f.vten = t.vten;
    f.cqv = t.cqv; f.cqc = t.cqc; f.fqv = t.fqv; f.fqc = t.fqc; f.depplane = t.depplane;
    f.tphy = phy_tqc(t, 0); f.qvphy = phy_tqc(t, 1); f.qcphy = phy_tqc(t, 2); f.uphy = t.phy[3]; f.vphy = t.phy[4];
    f.ppphy = t.phy[5]; f.wphy = t.phy[6];
    f.slqv = t.slqv; f.slqc = t.slqc;
    f.d6u = t.d6[0]; f.d6v = t.d6[1]; f.d6t = t.d6[2]; f.d6qv = t.d6[3]; f.d6qc = t.d6[4];
    f.d6pp = t.d6[5]; f.d6w = t.d6[6];
    f.kpbl = hc.iqxvadv == 3 ? t.kpbl : nullptr;
    for (int n = 0; n < hc.nsp; n++) f.qxa1[n] = t.a1qx[n][c];
    return f;
  }

  // The LDS-tiled kernels stage a tile sized at compile time (their __launch_bounds__ = the
  // tile's thread count) and index it by threadIdx; their launches take grid and block from the
  // same kernels.hpp constants.  Check once that the code objects were built for those tiles, so
  // a block-size mismatch between a kernel and its launch fails here, not as unwritten points.
  void check_block_sizes() {
    struct K { const void* f; int threads; const char* name; };
    const K ks[] = {{(const void*)k_update<OptDefault>, SBT, "k_update<OptDefault>"},
                    {(const void*)k_momentum<OptDefault>, MBT, "k_momentum<OptDefault>"},
                    {(const void*)k_scalars<OptDefault>, SBT, "k_scalars<OptDefault>"},
                    {(const void*)k_update<OptGeneric>, SBT, "k_update<OptGeneric>"},
                    {(const void*)k_momentum<OptGeneric>, MBT, "k_momentum<OptGeneric>"},
                    {(const void*)k_scalars<OptGeneric>, SBT, "k_scalars<OptGeneric>"},
                    {(const void*)k_update<OptGeneric, Budget>, SBT, "k_update<OptGeneric, Budget>"},
                    {(const void*)k_scalars<OptGeneric, Budget>, SBT, "k_scalars<OptGeneric, Budget>"},
                    {(const void*)k_qx_tend<FamQx>, QBT, "k_qx_tend<FamQx>"},
                    {(const void*)k_qx_tend<FamTr>, QBT, "k_qx_tend<FamTr>"},
                    {(const void*)k_qx_tend<FamTr, TrBudget>, QBT, "k_qx_tend<FamTr, TrBudget>"}};
    for (const K& k : ks) {
      hipFuncAttributes a{};
      HIPCHK(hipFuncGetAttributes(&a, k.f));
      if (a.maxThreadsPerBlock != k.threads)
        throw std::runtime_error(std::string("rcmdyn: ") + k.name + " was compiled for " +
                                 std::to_string(a.maxThreadsPerBlock) + " threads per block, launched with " +
                                 std::to_string(k.threads));
    }
  }

  // The dynamic LDS the launches request grows with the tile: the serial moisture fix's
  // (negfix_lds / negfix_sweep_lds, a row of the plane) and k_split_project's (4 x kz x SPC).
  // Check the owned tiles' requests against the device's limit at create, so a tile too large
  // for them is refused here rather than failing a launch inside a step.  The hydrostatic
  // k_columns asks for col_lds() (4 x kz x COLW, twice k_split_project's) whatever the tile.
  void check_lds() {
    int maxs = 0;
    HIPCHK(hipDeviceGetAttribute(&maxs, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (cfg.idynamic != 2 && col_lds() > (size_t)maxs)
      throw std::runtime_error("rcmdyn: k_columns at kz = " + std::to_string(cfg.kz) + " needs " + std::to_string(col_lds()) +
                               " bytes of LDS per block, the device allows " + std::to_string(maxs));
    for (int t = 0; t < cfg.tile_count; t++) {
      const Geom& g = all[cfg.tile_first + t];
      const size_t need = sizeof(double) * (size_t)std::max(negfix_lds(g), 4 * cfg.kz * SPC);
      if (need > (size_t)maxs)
        throw std::runtime_error("rcmdyn: tile " + std::to_string(cfg.tile_first + t) + " needs " + std::to_string(need) +
                                 " bytes of LDS per block, the device allows " + std::to_string(maxs));
    }
  }

  void create(const rcmdyn_config* c, std::vector<PlanOp>* plan = nullptr) {
    sw = Switches::read();
    inject_fail = sw.inject_launch_failure;
    cfg = *c;
    dry = plan != nullptr;
    if (cfg.abi_version != RCMDYN_ABI_VERSION) throw std::runtime_error("rcmdyn: ABI version mismatch");
    if (cfg.idynamic != 1 && cfg.idynamic != 2) throw std::runtime_error("rcmdyn: idynamic must be 1 or 2");
    if (cfg.idynamic == 2) {
      if (!(cfg.nh_dtsmax > 0.0) || !(cfg.nh_xmsf > 0.0))
        throw std::runtime_error("rcmdyn: nh_dtsmax / nh_xmsf (init_sound) must be set for idynamic=2");
    }
    if (cfg.idiffu < 1 || cfg.idiffu > 3) throw std::runtime_error("rcmdyn: idiffu must be 1, 2 or 3");
    if (cfg.ipgf != 0 && cfg.ipgf != 1) throw std::runtime_error("rcmdyn: ipgf must be 0 or 1");
    if (cfg.isladvec != 0 && cfg.isladvec != 1) throw std::runtime_error("rcmdyn: isladvec must be 0 or 1");
    if (cfg.ibltyp == 2 && !(cfg.tkemin >= 0.0))
      throw std::runtime_error("rcmdyn: ibltyp=2 needs tkemin (uwtkemin) >= 0");
    if (cfg.iuwvadv != 0 && cfg.iuwvadv != 1) throw std::runtime_error("rcmdyn: iuwvadv must be 0 or 1");
    if (cfg.iboudy < 0 || cfg.iboudy > 5) throw std::runtime_error("rcmdyn: iboudy must be 0 to 5");
    // iboudy = 0 (fixed lateral values): the b0-only branches of bdyval (Main/mod_bdycod.F90:944,
    // 1317, 1535) act on the boundary lines only, so with CRM, which has none, it is the empty
    // boundary of crm_test.in; on a limited area those branches are not built
    if (cfg.iboudy == 0 && cfg.i_crm != 1)
      throw std::runtime_error("rcmdyn: iboudy = 0 (fixed lateral values) is built for i_crm = 1 only");
    // physicsparam ipptls and the nqx param derives from it (Main/mod_params.F90:1358-1366)
    if (cfg.ipptls < 1 || cfg.ipptls > 2)
      throw std::runtime_error("rcmdyn: ipptls must be 1 or 2 (ipptls = 0 leaves the hydrometeor tendencies unsummed, "
                               "Main/mod_tendency.F90:331: not supported)");
    if (cfg.nqx != (cfg.ipptls > 1 ? 5 : 2))
      throw std::runtime_error("rcmdyn: nqx must be 2 for ipptls = 1 and 5 for ipptls = 2 (Main/mod_params.F90:1358-1366)");
    // periodic decompositions and chemical tracers are not built: refused, not ignored
    if (cfg.i_band != 0 && cfg.i_band != 1) throw std::runtime_error("rcmdyn: i_band must be 0 or 1");
    // CRM (i_crm = 1, PreProc/CRM/crm_test.in): periodic in j and i, for the non-hydrostatic
    // core over the band; CRM without the band decomposes differently on one rank and on
    // several in the reference (Main/mpplib/mod_mppparam.F90:1104-1108 against 1132)
    if (cfg.i_crm != 0 && cfg.i_crm != 1) throw std::runtime_error("rcmdyn: i_crm must be 0 or 1");
    if (cfg.i_crm == 1 && (cfg.i_band != 1 || cfg.idynamic != 2))
      throw std::runtime_error("rcmdyn: i_crm = 1 is built for the non-hydrostatic core over the band (i_band = 1)");
    if (cfg.i_band != 0 && cfg.idynamic == 2 && cfg.idiffu == 3)
      throw std::runtime_error("rcmdyn: idiffu = 3 on the non-hydrostatic band / CRM is not supported");
    if (cfg.ichem != 0)
      throw std::runtime_error("rcmdyn: ichem = 1 is not supported in rcmdyn_config, which carries no tracer count: create "
                               "with ichem = 0 and declare the chemical tracers with rcmdyn_set_tracers");
    if (const char* m = std::getenv("RCMDYN_RCCL_CHAN2"))   // the removed second-communicator modes
      if (std::string(m) != "one") throw std::runtime_error("rcmdyn: RCMDYN_RCCL_CHAN2 must be one (or unset)");
    // dynparam's upstream_mode (default .true., Main/mod_params.F90:646); .false. runs the
    // centred branches (Main/mod_advection.F90:141,322,409,532,624; see c.ul)
    if (cfg.upstream_mode != 0 && cfg.upstream_mode != 1)
      throw std::runtime_error("rcmdyn: upstream_mode must be 0 or 1");
    if (cfg.stability_enhance != 0 && cfg.stability_enhance != 1)
      throw std::runtime_error("rcmdyn: stability_enhance must be 0 or 1");
    if (cfg.kz < 2 || cfg.kz > MAXKZ) throw std::runtime_error("rcmdyn: kz out of range");
    if (cfg.nsplit < 1 || cfg.nsplit > MAXSPLIT) throw std::runtime_error("rcmdyn: nsplit out of range");
    if (cfg.nspgx >= MAXNSP || cfg.nspgd != cfg.nspgx) throw std::runtime_error("rcmdyn: nspgx/nspgd unsupported");
    ntiles = cfg.nproc_j * cfg.nproc_i;
    halo = ntiles > 1 || cfg.i_band != 0;
    if (ntiles < 1 || cfg.tile_first < 0 || cfg.tile_count < 1 || cfg.tile_first + cfg.tile_count > ntiles)
      throw std::runtime_error("rcmdyn: bad tile range");
    if (!dry) {
      if (cfg.device >= 0) HIPCHK(hipSetDevice(cfg.device));
      HIPCHK(hipGetDevice(&device));
    }
    for (int t = 0; t < ntiles; t++) {
      all.push_back(make_geom(cfg.jx, cfg.iy, cfg.nproc_j, cfg.nproc_i, t, G, cfg.i_band, cfg.i_crm));
      const Geom& g = all.back();
      if (g.jde2 - g.jde1 + 1 < 3 || g.ide2 - g.ide1 + 1 < 3)
        throw std::runtime_error("rcmdyn: Too much processors (tile < 3x3), mod_mppparam.F90:1365");
      // the NH radiative condition reaches 6 points: its halo must come from direct neighbours
      if (cfg.idynamic == 2 && cfg.nproc_j * cfg.nproc_i > 1 && (g.jde2 - g.jde1 + 1 < 6 || g.ide2 - g.ide1 + 1 < 6))
        throw std::runtime_error("rcmdyn: non-hydrostatic tiles must be at least 6x6 points");
    }
    compute_constants();
    if (dry) {
      if (cfg.tile_count != 1 || cfg.comm_size != ntiles || cfg.tile_first != cfg.comm_rank)
        throw std::runtime_error("rcmdyn_exchange_plan: one tile per rank (tile_first == comm_rank, comm_size = tiles)");
      hs = StepState{};
      hs.dt = cfg.dtsec;
      tiles.resize(1);
      setup_tile(tiles[0], cfg.tile_first);
      comm.reset(make_plan_comm(cfg.comm_rank, plan));
      return;
    }
    check_block_sizes();
    check_lds();
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&dc, sizeof(Consts)));
    HIPCHK(hipMemcpy(dc, &hc, sizeof(Consts), hipMemcpyHostToDevice));
    hs = StepState{};
    hs.dt = cfg.dtsec; hs.xbctime = 0.0; hs.lcount = 0;
    HIPCHK(hipMalloc(&ds, sizeof(StepState)));
    HIPCHK(hipMemcpy(ds, &hs, sizeof(StepState), hipMemcpyHostToDevice));
    tiles.resize(cfg.tile_count);
    for (int t = 0; t < cfg.tile_count; t++) {
      const Geom& g = all[cfg.tile_first + t];
      if ((double)g.plane * 8.0 * (cfg.kz + 1) >= 4294967296.0)
        throw std::runtime_error("rcmdyn: tile too large for 32-bit field offsets");
      setup_tile(tiles[t], cfg.tile_first + t);
    }
    HIPCHK(hipMalloc(&red, sizeof(double) * 2 * (size_t)(red_total + 1)));
    HIPCHK(hipHostMalloc((void**)&hflags, sizeof(FlagSnap) * NFLAGSLOT, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(hflags, 0, sizeof(FlagSnap) * NFLAGSLOT);
    HIPCHK(hipHostGetDevicePointer((void**)&dflags, hflags, 0));
    for (auto& e : fev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (cfg.tile_count < ntiles) {
      // RCMDYN_LOCAL_COMM=<group>: the in-process loopback transport of the multi-rank tests
      const char* lg = std::getenv("RCMDYN_LOCAL_COMM");
      if (lg && *lg) {
        if (cfg.comm_size != ntiles || cfg.tile_count != 1 || cfg.tile_first != cfg.comm_rank)
          throw std::runtime_error("rcmdyn: local communicator mode needs one tile per rank (tile_first == comm_rank)");
        comm.reset(make_local_comm(lg, cfg.comm_rank, cfg.comm_size));
      } else {
        comm.reset(make_rccl_comm(cfg));
      }
    }
    else if (sw.force_rccl && halo) comm.reset(make_rccl_self_comm());
    if (comm) {
      HIPCHK(hipMalloc(&derr, sizeof(int32_t)));
      HIPCHK(hipHostMalloc((void**)&hgerr, sizeof(int32_t) * NFLAGSLOT, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(hgerr, 0, sizeof(int32_t) * NFLAGSLOT);
      HIPCHK(hipHostGetDevicePointer((void**)&dgerr, hgerr, 0));
      for (auto& e : gev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (halo) {
      HIPCHK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&evfork, hipEventDisableTiming));
      for (hipEvent_t& e : evjoin) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
  }

  void destroy() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (ostream) {
      (void)hipStreamSynchronize(ostream);
      (void)hipEventDestroy(ev_out);
      (void)hipEventDestroy(ev_copied);
      (void)hipStreamDestroy(ostream);
      if (oflags) (void)hipHostFree(oflags);
      for (auto& t : tiles)
        if (t.ohost) (void)hipHostFree(t.ohost);
    }
    invalidate_graphs();
    for (auto& e : fev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : gev)
      if (e) (void)hipEventDestroy(e);
    if (hflags) (void)hipHostFree(hflags);
    if (hgerr) (void)hipHostFree(hgerr);
    if (derr) (void)hipFree(derr);
    free_tracers();
    free_subex();
    if (sbx_chis) (void)hipFree(sbx_chis);
    che_destroy();
    for (auto& t : tiles)
      for (void* p : t.allocs) (void)hipFree(p);
    tiles.clear();
    comm.reset();
    if (dc) (void)hipFree(dc);
    if (ds) (void)hipFree(ds);
    if (red) (void)hipFree(red);
    if (mck_part) (void)hipFree(mck_part);
    if (mck_tab) (void)hipFree(mck_tab);
    if (mck_log) (void)hipFree(mck_log);

    if (evfork) (void)hipEventDestroy(evfork);
    for (hipEvent_t e : evjoin)
      if (e) (void)hipEventDestroy(e);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (stream) (void)hipStreamDestroy(stream);
  }

  void invalidate_graphs() {
    for (auto& g : graphs)
      for (hipGraphExec_t& x : g)
        if (x) { (void)hipGraphExecDestroy(x); x = nullptr; }
  }

  // ------------------------------------------------------------------ step error flags
  // a tend was issued whose clock is lc once it ran: remember its snapshot slot; with a
  // communicator, every GLOBAL_EVERY steps (or when `global`) issue the job-wide reduction
  void note_step(long long lc, bool global = false) {
    if (dry) {
      if (global || lc % GLOBAL_EVERY == 0) comm->allreduce_max(nullptr, 1, stream);
      return;
    }
    if (comm) {
      if (global || lc % GLOBAL_EVERY == 0) {
        if ((int)gpending.size() >= NFLAGSLOT - 1) check(0);
        const int slot = gslot++ % NFLAGSLOT;
        hipLaunchKernelGGL(k_err_gather, dim3(1), dim3(64), 0, stream, ds, derr);
        comm->allreduce_max(derr, 1, stream);
        hipLaunchKernelGGL(k_err_publish, dim3(1), dim3(64), 0, stream, derr, dgerr + slot);
        HIPCHK(hipEventRecord(gev[slot], stream));
        gpending.push_back({lc, slot});
      }
      return;
    }
    if ((int)pending.size() >= NFLAGSLOT - 1) check(0);
    HIPCHK(hipEventRecord(fev[(lc - 1 + NFLAGSLOT) % NFLAGSLOT], stream));
    pending.push_back(lc);
  }
  // a failure: the stream drains, the sticky device flags are cleared (reported once) and
  // the error is raised -- the reference's fatal (Main/mod_tendency.F90:702,
  // Main/mod_sound.F90:679-681, Main/mod_sladvection.F90:149-154).  keep: a rank-local report
  // (check_now with a communicator) leaves the flags set, so the next job-wide reduction still
  // carries the failure to the other ranks even if this rank's host catches the error.
  [[noreturn]] void fail(int sl, long long lc, const std::string& scope, bool keep = false) {
    HIPCHK(hipStreamSynchronize(stream));
    pending.clear();
    gpending.clear();
    if (!keep) {
      StepState st;
      HIPCHK(hipMemcpy(&st, ds, sizeof(st), hipMemcpyDeviceToHost));
      st.nanflag = 0; st.slflag = 0;
      HIPCHK(hipMemcpy(ds, &st, sizeof(st), hipMemcpyHostToDevice));
    }
    const std::string at = " (" + scope + std::to_string(lc) + ")";
    if (sl) throw std::runtime_error("SLADVECTION: departure point beyond one grid cell" + at);
    throw std::runtime_error("CFL VIOLATION" + at);
  }
  // check the flags of the oldest steps until at most `keep` stay unchecked (with a
  // communicator: the reduced words, one reduction interval behind unless keep = 0)
  void check(size_t keep) {
    if (comm) {
      const size_t gkeep = keep == 0 ? 0 : 1;
      while (gpending.size() > gkeep) {
        const auto [lc, slot] = gpending.front();
        HIPCHK(hipEventSynchronize(gev[slot]));
        gpending.pop_front();
        const int w = ((volatile int32_t*)hgerr)[slot];
        if (w) fail(w & 2, lc, "job, by step ");
      }
      return;
    }
    while (pending.size() > keep) {
      const long long lc = pending.front();
      const int slot = (int)((lc - 1 + NFLAGSLOT) % NFLAGSLOT);
      HIPCHK(hipEventSynchronize(fev[slot]));
      pending.pop_front();
      const volatile FlagSnap* f = hflags + slot;
      const int sl = f->slflag, nan = f->nanflag;
      if (sl || nan) fail(sl, lc, "step ");
    }
  }
  // at a host read point (get, diagnostics) with the stream idle: every step issued so far is
  // checked, so no field of a failed run leaves the engine (the reference's fatal stops before
  // any output).  With a communicator the reductions already issued are drained (no new
  // collective: a get need not be called by every rank) and this rank's own sticky flags are
  // read as well; a rank-local failure is reported to its host, which aborts the job as the
  // reference's fatal does (Main/abort.F90:20-36).
  void check_now() {
    check(0);
    if (!comm) return;
    StepState st;
    HIPCHK(hipMemcpy(&st, ds, sizeof(st), hipMemcpyDeviceToHost));
    if (st.nanflag || st.slflag) fail(st.slflag, hs.lcount, "this rank, by step ", true);
  }


  // ------------------------------------------------------------------ field access
  double* fptr(Tile& t, FK f, int n = 0) {
    const int c = t.cur, q = thp(t);
    const int tc = cfg.idynamic == 2 ? 0 : c;        // the tracers' parity (the NH core: in place)
    switch (f) {
      case FK::TRA1: return t.tra1[tc][n]; case FK::TRA2: return t.tra2[tc][n]; case FK::TRCQ: return t.trcq[n];
      case FK::TRB0: return t.trb0[n]; case FK::TRBT: return t.trbt[n];
      default: break;
    }
    switch (f) {
      case FK::A1U: return t.a1u[c]; case FK::A1V: return t.a1v[c]; case FK::A1T: return t.a1t[q];
      case FK::A1QV: return t.a1qv[q]; case FK::A1QC: return t.a1qc[q];
      case FK::A2U: return t.a2u[c]; case FK::A2V: return t.a2v[c]; case FK::A2T: return t.a2t[q];
      case FK::A2QV: return t.a2qv[q]; case FK::A2QC: return t.a2qc[q];
      case FK::PSA: return t.psa_[c]; case FK::PSB: return t.psb_[c];
      case FK::PSDOTA: return t.psdota; case FK::PSDOTB: return t.psdotb;
      case FK::RPSDA: return t.rpsda; case FK::RPSDB: return t.rpsdb; case FK::QDOT: return t.qdot;
      case FK::CQV: return t.cqv; case FK::CQC: return t.cqc;
      case FK::PHI: return t.phi; case FK::UU: return t.uu; case FK::VV: return t.vv;
      case FK::DHSUM: return t.dhsum; case FK::DELH: return t.delh;
      case FK::MSFX: return t.msfx; case FK::MSFD: return t.msfd; case FK::HT: return t.ht;
      case FK::CORIOL: return t.coriol;
      case FK::UB0: return t.ub0; case FK::UBT: return t.ubt; case FK::VB0: return t.vb0;
      case FK::VBT: return t.vbt; case FK::TB0: return t.tb0; case FK::TBT: return t.tbt;
      case FK::QB0: return t.qb0; case FK::QBT: return t.qbt; case FK::PB0: return t.pb0;
      case FK::PBT: return t.pbt; case FK::DSTOR: return t.dstor; case FK::HSTOR: return t.hstor;
      default: break;
    }
    switch (f) {
      case FK::UB1: return t.bb1[0]; case FK::VB1: return t.bb1[1]; case FK::TB1: return t.bb1[2];
      case FK::QB1: return t.bb1[3]; case FK::PB1: return t.bb1[4]; case FK::PPB1: return t.bb1[5];
      case FK::WWB1: return t.bb1[6];
      case FK::SLQV: return t.slqv; case FK::SLQC: return t.slqc;
      case FK::A1TKE: return t.a1tke; case FK::A2TKE: return t.a2tke;
      case FK::D6U: return t.d6[0]; case FK::D6V: return t.d6[1]; case FK::D6T: return t.d6[2];
      case FK::D6QV: return t.d6[3]; case FK::D6QC: return t.d6[4];
      case FK::KPBL: return t.kpbl;
      case FK::SBX_RH0ADJ: return t.sbx[RCMDYN_SUBEX_RH0ADJ]; case FK::SBX_LSCT: return t.sbx[RCMDYN_SUBEX_LSC_T];
      case FK::SBX_LSCQV: return t.sbx[RCMDYN_SUBEX_LSC_QV]; case FK::SBX_LSCQC: return t.sbx[RCMDYN_SUBEX_LSC_QC];
      default: break;
    }
    if (f >= FK::A1QX0 && f <= FK::D6QX2) {
      const int r = (int)f - (int)FK::A1QX0, n = r % NQXH;
      switch (r / NQXH) {
        case 0: return t.a1qx[n][c];
        case 1: return t.a2qx[n][c];
        case 2: return t.cqx[n];
        case 3: return t.slqx[n];
        default: return t.d6qx[n];
      }
    }
    const NHFields& h = nhf[&t - tiles.data()];
    switch (f) {
      case FK::A1PP: return h.a1pp; case FK::A2PP: return h.a2pp; case FK::A1W: return h.a1w;
      case FK::A2W: return h.a2w; case FK::NCR: return h.cr; case FK::NXKCR: return h.xkcr;
      case FK::NCDT: return h.cdt; case FK::NCPP: return h.cpp; case FK::NCU: return h.cu; case FK::NCV: return h.cv;
      default: break;
    }
    return nullptr;
  }

  // public field id -> buffer on tile t, null where this engine holds none (an NH or nqx = 5
  // field on an engine without that option, a lazily allocated one before its event); the
  // attributes of the field are its row of fieldtab::TAB.  Every enumerator is named and there
  // is no default, so -Wswitch reports an id without a buffer.
  double* field_ptr(Tile& t, int id) {
    const fieldtab::Row* r = fieldtab::row(id);
    if (!r || !holds(r->need)) return nullptr;
    const rcmdyn_field f = r->id;
    auto nh = [&]() -> NHFields& { return nhf[&t - tiles.data()]; };
    auto cst = [](const double* p) { return const_cast<double*>(p); };
    switch (f) {
      case RCMDYN_ATM1_U: return fptr(t, FK::A1U); case RCMDYN_ATM1_V: return fptr(t, FK::A1V);
      case RCMDYN_ATM1_T: return fptr(t, FK::A1T); case RCMDYN_ATM1_QV: return fptr(t, FK::A1QV);
      case RCMDYN_ATM1_QC: return fptr(t, FK::A1QC);
      case RCMDYN_ATM2_U: return fptr(t, FK::A2U); case RCMDYN_ATM2_V: return fptr(t, FK::A2V);
      case RCMDYN_ATM2_T: return fptr(t, FK::A2T); case RCMDYN_ATM2_QV: return fptr(t, FK::A2QV);
      case RCMDYN_ATM2_QC: return fptr(t, FK::A2QC);
      case RCMDYN_PSA: return fptr(t, FK::PSA); case RCMDYN_PSB: return fptr(t, FK::PSB);
      case RCMDYN_DSTOR: return fptr(t, FK::DSTOR); case RCMDYN_HSTOR: return fptr(t, FK::HSTOR);
      case RCMDYN_MSFX: return fptr(t, FK::MSFX); case RCMDYN_MSFD: return fptr(t, FK::MSFD);
      case RCMDYN_CORIOL: return fptr(t, FK::CORIOL); case RCMDYN_HT: return fptr(t, FK::HT);
      case RCMDYN_XUB_B0: return fptr(t, FK::UB0); case RCMDYN_XUB_BT: return fptr(t, FK::UBT);
      case RCMDYN_XVB_B0: return fptr(t, FK::VB0); case RCMDYN_XVB_BT: return fptr(t, FK::VBT);
      case RCMDYN_XTB_B0: return fptr(t, FK::TB0); case RCMDYN_XTB_BT: return fptr(t, FK::TBT);
      case RCMDYN_XQB_B0: return fptr(t, FK::QB0); case RCMDYN_XQB_BT: return fptr(t, FK::QBT);
      case RCMDYN_XPSB_B0: return fptr(t, FK::PB0); case RCMDYN_XPSB_BT: return fptr(t, FK::PBT);
      case RCMDYN_PSC: return t.psc; case RCMDYN_PTEN: return t.pten + t.g.plane;
      case RCMDYN_PSDOTA: return fptr(t, FK::PSDOTA);
      case RCMDYN_TTEN: return t.tten; case RCMDYN_UTEN: return t.uten; case RCMDYN_VTEN: return t.vten;
      case RCMDYN_QVTEN: return t.qvten; case RCMDYN_QCTEN: return t.qcten; case RCMDYN_OMEGA: return t.omega;
      case RCMDYN_QDOT: return fptr(t, FK::QDOT); case RCMDYN_XKC: return t.xkcs; case RCMDYN_PHI: return fptr(t, FK::PHI);
      case RCMDYN_ATM1_PP: return fptr(t, FK::A1PP); case RCMDYN_ATM2_PP: return fptr(t, FK::A2PP);
      case RCMDYN_ATM1_W: return fptr(t, FK::A1W); case RCMDYN_ATM2_W: return fptr(t, FK::A2W);
      case RCMDYN_XPPB_B0: return cst(nh().ppb0); case RCMDYN_XPPB_BT: return cst(nh().ppbt);
      case RCMDYN_XWWB_B0: return cst(nh().wwb0); case RCMDYN_XWWB_BT: return cst(nh().wwbt);
      case RCMDYN_ATM0_PS: return cst(nh().ps0); case RCMDYN_ATM0_PR: return cst(nh().pr0);
      case RCMDYN_ATM0_T: return cst(nh().t0); case RCMDYN_ATM0_RHO: return cst(nh().rho0);
      case RCMDYN_ATM0_Z: return cst(nh().z0); case RCMDYN_ATM0_PF: return cst(nh().pf0);
      case RCMDYN_ATM0_RHOF: return cst(nh().rhof0); case RCMDYN_ATM0_ZF: return cst(nh().zf0);
      case RCMDYN_DPSDXM: return cst(nh().dpsdxm); case RCMDYN_DPSDYM: return cst(nh().dpsdym);
      case RCMDYN_DPRDDX: return cst(nh().dprddx); case RCMDYN_DPRDDY: return cst(nh().dprddy);
      case RCMDYN_EF: return cst(nh().ef); case RCMDYN_DDX: return cst(nh().ddx); case RCMDYN_DDY: return cst(nh().ddy);
      case RCMDYN_DMDX: return cst(nh().dmdx); case RCMDYN_DMDY: return cst(nh().dmdy);
      case RCMDYN_EX: return cst(nh().ex); case RCMDYN_CRX: return cst(nh().crx); case RCMDYN_CRY: return cst(nh().cry);
      case RCMDYN_TPHY: case RCMDYN_QVPHY: case RCMDYN_QCPHY: case RCMDYN_UPHY: case RCMDYN_VPHY:
      case RCMDYN_PPPHY: case RCMDYN_WPHY:
        return t.phy[f - RCMDYN_TPHY];
      case RCMDYN_ATMS_UBX3D: case RCMDYN_ATMS_VBX3D: case RCMDYN_ATMS_UBD3D: case RCMDYN_ATMS_VBD3D:
      case RCMDYN_ATMS_TB3D: case RCMDYN_ATMS_QVB3D: case RCMDYN_ATMS_QCB3D: case RCMDYN_ATMS_TV3D:
      case RCMDYN_ATMS_PB3D: case RCMDYN_ATMS_PF3D: case RCMDYN_ATMS_PS2D: case RCMDYN_ATMS_RHOX2D:
      case RCMDYN_ATMS_TH3D: case RCMDYN_ATMS_RHOB3D: case RCMDYN_ATMS_TP3D: case RCMDYN_ATMS_WPX3D:
      case RCMDYN_ATMS_WB3D: case RCMDYN_ATMS_ZQ: case RCMDYN_ATMS_ZA: case RCMDYN_ATMS_DZQ:
      case RCMDYN_ATMS_QSB3D: case RCMDYN_ATMS_RHB3D:
        return t.atms[f - RCMDYN_ATMS_UBX3D];
      case RCMDYN_XUB_B1: case RCMDYN_XVB_B1: case RCMDYN_XTB_B1: case RCMDYN_XQB_B1: case RCMDYN_XPSB_B1:
      case RCMDYN_XPPB_B1: case RCMDYN_XWWB_B1:
        return t.bin[f - RCMDYN_XUB_B1];
      case RCMDYN_ATM0_PSDOT: return t.psdot0;
      case RCMDYN_ATM1_TKE: return fptr(t, FK::A1TKE); case RCMDYN_ATM2_TKE: return fptr(t, FK::A2TKE);
      case RCMDYN_TKEPHY: return t.tkephy; case RCMDYN_KPBL: return fptr(t, FK::KPBL);
      case RCMDYN_ATM1_QI: case RCMDYN_ATM1_QR: case RCMDYN_ATM1_QS: return fptr(t, fkq(FK::A1QX0, f - RCMDYN_ATM1_QI));
      case RCMDYN_ATM2_QI: case RCMDYN_ATM2_QR: case RCMDYN_ATM2_QS: return fptr(t, fkq(FK::A2QX0, f - RCMDYN_ATM2_QI));
      case RCMDYN_QIPHY: case RCMDYN_QRPHY: case RCMDYN_QSPHY: return t.phyx[f - RCMDYN_QIPHY];
      case RCMDYN_ATMS_QXB3D_QI: case RCMDYN_ATMS_QXB3D_QR: case RCMDYN_ATMS_QXB3D_QS:
        return t.atmsx[f - RCMDYN_ATMS_QXB3D_QI];
      case RCMDYN_NFIELDS: break;
    }
    return nullptr;
  }
  // whether an engine of this configuration keeps a buffer for a field with this need
  bool holds(fieldtab::Need n) const {
    return !(n == fieldtab::NH && cfg.idynamic != 2) && !(n == fieldtab::NQX5 && hc.nsp == 0);
  }
  int field_levels(int f) const { return fieldtab::levels(fieldtab::TAB[f].lev, cfg.kz, cfg.nsplit); }
  size_t field_size(const Tile& t, int f) const { return t.g.plane * (size_t)field_levels(f); }
  // why an engine of this configuration refuses a field with this need, null when it does not
  const char* lacks(fieldtab::Need n) const {
    const bool nh = cfg.idynamic == 2;
    switch (n) {
      case fieldtab::ANY: break;
      case fieldtab::NH: return nh ? nullptr : "non-hydrostatic field on a hydrostatic engine";
      case fieldtab::HYD_PS: return nh ? "the non-hydrostatic core reads no ps record (p* is atm0%ps)" : nullptr;
      case fieldtab::HYD_Z: return nh ? "zq/za/dzq are not computed by mkslice for idynamic=2" : nullptr;
      case fieldtab::NQX5: return hc.nsp ? nullptr : "qi/qr/qs fields need nqx = 5 (ipptls = 2)";
      case fieldtab::UW: return cfg.ibltyp == 2 ? nullptr : "TKE/kpbl fields need ibltyp=2 (UW PBL)";
    }
    return nullptr;
  }
  // whether the buffers of a lazily allocated group exist (DIAG: are being written)
  bool have(fieldtab::Lazy g) const {
    if (tiles.empty()) return true;
    const Tile& t = tiles[0];
    switch (g) {
      case fieldtab::NONE: break;
      case fieldtab::PHYSICS: return t.phy[0];
      case fieldtab::BDYIN: return t.bin[0];
      case fieldtab::TKEPHY: return t.tkephy;
      case fieldtab::SLICE: return t.atms[0];
      case fieldtab::DIAG: return diag;
    }
    return true;
  }
  // what a get says of a group that does not exist yet (the bdyin record: 'unknown field')
  static constexpr const char* WAITS_FOR[] = {
      nullptr, "no physics tendencies were put", nullptr, "no TKE tendency was put",
      "no slice fields yet (rcmdyn_tend_pre_physics)", "tendency diagnostics are off (rcmdyn_set_diagnostics)"};
  static_assert(fieldtab::DIAG == 5 && sizeof(WAITS_FOR) / sizeof(WAITS_FOR[0]) == 6, "one text per fieldtab::Lazy");

  // ------------------------------------------------------------------ host windows
  // Every put and get hands a host box to or from the tiles' frames (window.hpp has the index
  // arithmetic): a band's columns (i_band) and the CRM's rows (i_crm) wrap.
  Period period() const { return Period{cfg.jx, cfg.iy, cfg.i_band != 0, cfg.i_crm != 0}; }
  static Staging frame(const Geom& g, int nk) { return Staging{g.j0, g.i0, g.nj, g.ni, g.pitch, g.plane, nk, 0}; }
  // a pending lazy tend or its corrections are launched, and the stream is idle
  void quiesce() {
    settle();
    HIPCHK(hipStreamSynchronize(stream));
  }
  // The host box src into the buffer ptr(tile) of nk levels of every tile: every frame point whose
  // global index lies in the box, the ghost ring included, and the frame points past either end of
  // a period from the wrapped index.
  template <class P>
  void put_window(const double* src, const Box& b, int nk, P ptr) {
    quiesce();
    for (auto& t : tiles) {
      double* d = ptr(t);
      std::vector<double> h((size_t)nk * t.g.plane);
      HIPCHK(hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
      scatter(h.data(), frame(t.g, nk), period(), src, b);
      HIPCHK(hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    }
  }
  // The other way, at a host read point (check_now): of every tile the owned dot points, or the
  // interior cross points alone, that lie in the box.
  enum class Range { Owned, Interior };
  template <class P>
  void get_window(double* dst, const Box& b, int nk, P ptr, Range range = Range::Owned) {
    quiesce();
    check_now();
    for (auto& t : tiles) {
      const double* d = ptr(t);
      const Geom& g = t.g;
      std::vector<double> h((size_t)nk * g.plane);
      HIPCHK(hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
      if (range == Range::Owned) gather(dst, b, h.data(), frame(g, nk), g.jde1, g.jde2, g.ide1, g.ide2);
      else gather(dst, b, h.data(), frame(g, nk), g.jci1, g.jci2, g.ici1, g.ici2);
    }
  }

  void put(int f, const double* src, const Box& b) {
    settle();
    const fieldtab::Row* r = fieldtab::row(f);
    if (!r || r->acc == fieldtab::RO) throw std::runtime_error("rcmdyn_put: field is read-only or unknown");
    if (const char* m = lacks(r->need)) throw std::runtime_error(std::string("rcmdyn_put: ") + m);
    if (f == RCMDYN_KPBL) {
      // vadv4d ind = 3 stops on a PBL top above the model (Main/mod_advection.F90:923-925); a 2-D
      // field: never fewer than one plane
      const size_t n = Box{b.j1, b.j2, b.i1, b.i2, b.k1, std::max(b.k1, b.k2)}.cells();
      for (size_t q = 0; q < n; q++) {
        if (src[q] > cfg.kz) throw std::runtime_error("rcmdyn_put: kpbl is greater than kz");
        if (src[q] != std::floor(src[q])) throw std::runtime_error("rcmdyn_put: kpbl must hold integers");
      }
    }
    if (!have(r->lazy)) enable(r->lazy);
    put_window(src, b, field_levels(f), [&](Tile& t) {
      double* d = field_ptr(t, f);
      if (!d) throw std::runtime_error("rcmdyn_put: unknown field");
      return d;
    });
    ghosts_stale = true;
    switch (r->after) {
      case fieldtab::NOTHING: break;
      case fieldtab::STATICS: statics_dirty = true; break;
      case fieldtab::BDY: bdy_dirty = true; break;
      // only the hydrostatic vadv4d ind = 3 (k_scalars, k_qx_tend) reads kpbl on the ghost ring;
      // the NH kernels read it at their own point
      case fieldtab::KPBL_RING: if (hc.iqxvadv == 3 && cfg.idynamic != 2) kpbl_dirty = true; break;
      case fieldtab::DPRD: dprd_any = dprd_put = true; invalidate_graphs(); break;
      case fieldtab::PR0: if (dprd_any) dprd_put = true; invalidate_graphs(); break;
      case fieldtab::GRAPHS: invalidate_graphs(); break;
    }
  }

  // The zero-filled buffers of a group that exists from the first put of one of its fields on,
  // for the fields this configuration offers.  PHYSICS: the pc_physic seam, which every later
  // tend adds; TKEPHY: the UW scheme's tendency; the captured graphs held null pointers for
  // both.  BDYIN: the raw ICBC record and NH atm0%psdot, with the coupled b1 (bb1) beside it.
  void enable(fieldtab::Lazy g) {
    HIPCHK(hipStreamSynchronize(stream));
    for (auto& t : tiles)
      for (const fieldtab::Row& r : fieldtab::TAB) {
        if (r.lazy != g || !holds(r.need)) continue;
        const rcmdyn_field f = r.id;
        double* d = dalloc(t, field_size(t, f));
        if (g == fieldtab::PHYSICS) (f < RCMDYN_QIPHY ? t.phy[f - RCMDYN_TPHY] : t.phyx[f - RCMDYN_QIPHY]) = d;
        else if (g == fieldtab::TKEPHY) t.tkephy = d;
        else if (f == RCMDYN_ATM0_PSDOT) t.psdot0 = d;
        else { t.bin[f - RCMDYN_XUB_B1] = d; t.bb1[f - RCMDYN_XUB_B1] = dalloc(t, field_size(t, f)); }
      }
    if (g != fieldtab::BDYIN) invalidate_graphs();
  }

  // mod_bdycod::bdyin from read_icbc on (bdyin.hip)
  void bdyin() {
    settle();
    if (tiles.empty() || !tiles[0].bin[0]) throw std::runtime_error("rcmdyn_bdyin: no ICBC record was put (XUB_B1 ..)");
    const int kz = cfg.kz;
    const bool nh = cfg.idynamic == 2;
    auto args = [&](Tile& t) {
      BdyinArgs a{};
      a.rub = t.bin[0]; a.rvb = t.bin[1]; a.rtb = t.bin[2]; a.rqb = t.bin[3]; a.rpb = t.bin[4];
      a.rppb = t.bin[5]; a.rwwb = t.bin[6]; a.psdot0 = t.psdot0;
      a.ub0 = t.ub0; a.ubt = t.ubt; a.ub1 = t.bb1[0]; a.vb0 = t.vb0; a.vbt = t.vbt; a.vb1 = t.bb1[1];
      a.tb0 = t.tb0; a.tbt = t.tbt; a.tb1 = t.bb1[2]; a.qb0 = t.qb0; a.qbt = t.qbt; a.qb1 = t.bb1[3];
      a.pb0 = t.pb0; a.pbt = t.pbt; a.pb1 = t.bb1[4];
      if (nh) {
        NHFields& h = nhf[&t - tiles.data()];
        a.ps0 = h.ps0;
        a.ppb0 = const_cast<double*>(h.ppb0); a.ppbt = const_cast<double*>(h.ppbt); a.ppb1 = t.bb1[5];
        a.wwb0 = const_cast<double*>(h.wwb0); a.wwbt = const_cast<double*>(h.wwbt); a.wwb1 = t.bb1[6];
      }
      a.rdtbdy = 1.0 / cfg.dtbdys;                        // Main/mod_bdycod.F90:203
      a.ptop = cfg.ptop; a.kz = kz; a.nh = nh ? 1 : 0;
      return a;
    };
    each([&](Tile& t) {
      KLAUNCH(k_bdyin_shift, grid3(t.g.nj, t.g.ni, kz + 1), BLK, 0, stream, t.g, args(t));
      KLAUNCH(k_bdyin_ps, grid3(t.g.jce2 - t.g.jce1 + 1, t.g.ice2 - t.g.ice1 + 1, 1), BLK, 0, stream, t.g, args(t));
    });
    xch({{FK::PB1, 1}}, 1, 0);                              // :759
    each([&](Tile& t) {
      KLAUNCH(k_bdyin_couple, grid3(t.g.jde2 - t.g.jde1 + 1, t.g.ide2 - t.g.ide1 + 1, kz + 1), BLK, 0, stream,
              t.g, args(t));
    });
    if (nh) xch({{FK::UB1, kz}, {FK::VB1, kz}, {FK::TB1, kz}, {FK::QB1, kz}, {FK::PPB1, kz}, {FK::WWB1, kz + 1}}, 1, 0);
    else xch({{FK::UB1, kz}, {FK::VB1, kz}, {FK::TB1, kz}, {FK::QB1, kz}}, 1, 0);   // :800-815
    each([&](Tile& t) {
      KLAUNCH(k_bdyin_timeint, grid3(t.g.nj, t.g.ni, kz + 1), BLK, 0, stream, t.g, args(t));
    });
    set_time(hs.lcount, hs.dt, 0.0);                        // xbctime = d_zero, :666
    bdy_dirty = true;                                       // b0/bt ghost rings (prepare)
  }

  // mkslice export (slice.hip) for the host physics, run by rcmdyn_tend_pre_physics
  // the export's buffers, allocated by the first slice (a capture that holds one allocates them
  // before it begins)
  void slice_allocs() {
    for (auto& t : tiles) {
      if (t.atms[0]) continue;
      for (int q = 0; q < fieldtab::NATMS; q++) t.atms[q] = dalloc(t, field_size(t, RCMDYN_ATMS_UBX3D + q));
      for (int n = 0; n < hc.nsp; n++) t.atmsx[n] = dalloc(t, field_size(t, RCMDYN_ATMS_QXB3D_QI + n));
    }
    tracer_slice_allocs();
  }
  void run_slice() {
    slice_allocs();
    each([&](Tile& t) {
      const Geom& g = t.g;
      const int c = t.cur;
      SliceArgs a{};
      a.a1u = t.a1u[c]; a.a1v = t.a1v[c]; a.a2u = t.a2u[c]; a.a2v = t.a2v[c]; a.a2t = t.a2t[thp(t)];
      a.a2qv = t.a2qv[thp(t)]; a.a2qc = t.a2qc[thp(t)]; a.psa = t.psa_[c]; a.psb = t.psb_[c];
      a.rpsb = t.rpsb; a.rpsdb = t.rpsdb; a.rpsda = t.rpsda; a.msfx = t.msfx; a.qdot = t.qdot; a.pten = t.pten;
      if (cfg.idynamic == 2) {
        const NHFields& h = nhf[&t - tiles.data()];
        a.a2pp = h.a2pp; a.a2w = h.a2w; a.ps0 = h.ps0; a.pr0 = h.pr0; a.pf0 = h.pf0; a.rho0 = h.rho0;
      }
      double** o = t.atms;
      a.ubx3d = o[0]; a.vbx3d = o[1]; a.ubd3d = o[2]; a.vbd3d = o[3]; a.tb3d = o[4]; a.qvb3d = o[5];
      a.qcb3d = o[6]; a.tv3d = o[7]; a.pb3d = o[8]; a.pf3d = o[9]; a.ps2d = o[10]; a.rhox2d = o[11];
      a.th3d = o[12]; a.rhob3d = o[13]; a.tp3d = o[14]; a.wpx3d = o[15]; a.wb3d = o[16]; a.zq = o[17];
      a.za = o[18]; a.dzq = o[19]; a.qsb3d = o[20]; a.rhb3d = o[21];
      a.ep2 = AMW / AMD;                                  // Share/mod_constants.F90:306
      a.rhmin = cfg.rhmin; a.rhmax = cfg.rhmax;
      for (int n = 0; n < hc.nsp; n++) { a.a2qx[n] = t.a2qx[n][c]; a.qxb3d[n] = t.atmsx[n]; }
      if (outon) {                                        // atm1%pr of this moment for OUT_RH
        a.opr = t.opr;
        if (cfg.idynamic == 2) a.a1pp = nhf[&t - tiles.data()].a1pp;
      }
      KLAUNCH(k_slice, grid3(g.jde2 - g.jde1 + 1, g.ide2 - g.ide1 + 1, 1), BLK, 0, stream, g, dc, a);
    });
    tracer_slice();
    if (outon) opr_filled = true;
  }

  void get(int f, double* dst, const Box& b) {
    settle();
    // A get names the option (nqx = 5, ibltyp = 2) or the event (the group's first put, the
    // slice, the diagnostics switch) a field waits for, then what the NH slice leaves out.  It
    // does not test NH and HYD_PS: a buffer this engine does not hold, the bdyin record before
    // its first put among them, is an 'unknown field' below, and XPSB_B1 reads as it was stored.
    const fieldtab::Row* r = fieldtab::row(f);
    if (r) {
      const char* m = r->need == fieldtab::NQX5 || r->need == fieldtab::UW ? lacks(r->need) : nullptr;
      if (!m && !have(r->lazy)) m = WAITS_FOR[r->lazy];
      if (!m && r->need == fieldtab::HYD_Z) m = lacks(r->need);
      if (m) throw std::runtime_error(std::string("rcmdyn_get: ") + m);
    }
    get_window(dst, b, r ? field_levels(f) : 0, [&](Tile& t) {   // no row: field_ptr is null
      double* d = field_ptr(t, f);
      if (!d) throw std::runtime_error("rcmdyn_get: unknown field");
      return d;
    });
  }

  // ------------------------------------------------------------------ output stream
  // The fields of mod_output's ATM / SRF / SHF streams that the dyn core owns (output.hip), off by
  // default and outside the captured step.  rcmdyn_output_atm forms the requested fields on the
  // compute stream into each tile's compact buffer (jci1:jci2 x ici1:ici2, floats or doubles) and
  // copies it to its pinned twin on a stream of its own behind an event, with the step's sticky
  // error flags of that moment; rcmdyn_get_output waits for that copy alone.  The copy has its
  // own stream because a decomposed step issues work on the engine's second stream, which would
  // otherwise queue behind the copy.
  bool outon = false;
  int out_prec = 8;
  uint32_t out_mask = 0;          // the fields of the last rcmdyn_output_atm (0: no snapshot)
  long long out_lcount = 0;       // the clock of that snapshot
  bool opr_filled = false;        // a slice ran with the stage on: Tile::opr holds atm1%pr
  hipStream_t ostream = nullptr;
  hipEvent_t ev_out = nullptr, ev_copied = nullptr;
  StepState* oflags = nullptr;    // pinned: the device clock and flags at the snapshot
  static constexpr const char* OUT_NAME[RCMDYN_NOUT] = {
      "OUT_PS", "OUT_PS_PA", "OUT_T", "OUT_U", "OUT_V", "OUT_W", "OUT_PP", "OUT_QV", "OUT_QC", "OUT_QI", "OUT_QR",
      "OUT_QS", "OUT_TKE", "OUT_PH", "OUT_ZH", "OUT_UA100", "OUT_VA100", "OUT_RH", "OUT_PF", "OUT_ZF", "OUT_OMEGA"};
  int out_levels(int f) const { return out_is_2d(f) ? 1 : cfg.kz; }
  static size_t out_cells(const Geom& g) { return (size_t)(g.jci2 - g.jci1 + 1) * (g.ici2 - g.ici1 + 1); }
  // why this engine refuses an output field now, null when it serves it
  const char* out_refusal(int f) const {
    const bool nh = cfg.idynamic == 2;
    switch (f) {
      case RCMDYN_OUT_W: case RCMDYN_OUT_PP: return lacks(fieldtab::NH);
      case RCMDYN_OUT_QI: case RCMDYN_OUT_QR: case RCMDYN_OUT_QS: return lacks(fieldtab::NQX5);
      case RCMDYN_OUT_TKE: return lacks(fieldtab::UW);
      case RCMDYN_OUT_ZH:
        if (nh) return "the non-hydrostatic height of the half levels is the constant atm0%z (ATM0_Z)";
        break;
      case RCMDYN_OUT_ZF:
        if (nh) return lacks(fieldtab::HYD_Z);
        break;
      case RCMDYN_OUT_OMEGA:
        // the NH step never fills the RCMDYN_OMEGA export (its omega is ATMS_WPX3D of the slice)
        if (nh) return "the diagnostics export holds no omega on the non-hydrostatic core (ATMS_WPX3D has it)";
        return diag ? nullptr : WAITS_FOR[fieldtab::DIAG];
      default: break;
    }
    // the leftovers of the last mkslice: zq and pf3d of its export, atm1%pr of one run with the stage on
    if (f == RCMDYN_OUT_ZH || f == RCMDYN_OUT_ZF || f == RCMDYN_OUT_PF) return have(fieldtab::SLICE) ? nullptr : WAITS_FOR[fieldtab::SLICE];
    if (f == RCMDYN_OUT_RH) return have(fieldtab::SLICE) && opr_filled ? nullptr : WAITS_FOR[fieldtab::SLICE];
    return nullptr;
  }
  void wait_output_copy() {
    if (ev_copied) HIPCHK(hipEventSynchronize(ev_copied));
  }
  void set_output(int on, int prec) {
    if (on && prec != 4 && prec != 8)
      throw std::runtime_error("rcmdyn_set_output: prec = " + std::to_string(prec) + " is neither 4 (float) nor 8 (double)");
    wait_output_copy();
    if (on && !ostream) {
      HIPCHK(hipStreamCreateWithFlags(&ostream, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_copied, hipEventDisableTiming));
      HIPCHK(hipHostMalloc((void**)&oflags, sizeof(StepState), hipHostMallocDefault));
      std::memset(oflags, 0, sizeof(StepState));
      // room for every field in doubles: 4 planes and RCMDYN_NOUT - 4 fields of kz levels
      for (auto& t : tiles) {
        const size_t n = out_cells(t.g) * (4 + (size_t)(RCMDYN_NOUT - 4) * cfg.kz);
        t.odev = dalloc(t, n);
        HIPCHK(hipHostMalloc(&t.ohost, n * sizeof(double), hipHostMallocDefault));
        std::memset(t.ohost, 0, n * sizeof(double));
        t.opr = dalloc(t, t.g.plane * (size_t)cfg.kz);
      }
    }
    const bool b = on != 0;
    if (b != outon || (b && prec != out_prec)) out_mask = 0;
    if (!b) opr_filled = false;          // k_slice stops writing atm1%pr: what is held goes stale
    outon = b;
    if (b) out_prec = prec;
  }
  void output_atm(uint32_t mask) {
    if (!outon) throw std::runtime_error("rcmdyn_output_atm: the output stage is off (rcmdyn_set_output)");
    if (mask == 0) throw std::runtime_error("rcmdyn_output_atm: mask = 0 names no field");
    if (mask >> RCMDYN_NOUT)
      throw std::runtime_error("rcmdyn_output_atm: mask = " + std::to_string(mask) + " has a bit beyond the last field (" +
                               std::to_string(RCMDYN_NOUT - 1) + ")");
    for (int f = 0; f < RCMDYN_NOUT; f++)
      if (((mask >> f) & 1u))
        if (const char* why = out_refusal(f)) throw std::runtime_error(std::string("rcmdyn_output_atm: ") + OUT_NAME[f] + ": " + why);
    settle();                       // a lazy tend replays its graph first
    wait_output_copy();             // the previous snapshot leaves the buffers first
    constexpr uint32_t WINDS = 1u << RCMDYN_OUT_U | 1u << RCMDYN_OUT_V | 1u << RCMDYN_OUT_UA100 | 1u << RCMDYN_OUT_VA100;
    // the ghost line of Main/mod_output.F90:250-251: the mean reads atm1%u, atm1%v at j + 1, i + 1
    if (mask & WINDS) xch({{FK::A1U, cfg.kz}, {FK::A1V, cfg.kz}}, 1, 0);
    out_mask = 0;
    const size_t esz = (size_t)out_prec;
    each([&](Tile& t) {
      const Geom& g = t.g;
      if (g.jci2 < g.jci1 || g.ici2 < g.ici1) return;
      OutArgs a{};
      long off = 0;
      for (int f = 0; f < RCMDYN_NOUT; f++) {
        t.ooff[f] = a.off[f] = off;
        if ((mask >> f) & 1u) off += (long)(out_cells(g) * out_levels(f));
      }
      const int c = t.cur, q = thp(t);
      a.psa = t.psa_[c]; a.a1t = t.a1t[q]; a.a1u = t.a1u[c]; a.a1v = t.a1v[c]; a.a1qv = t.a1qv[q]; a.a1qc = t.a1qc[q];
      a.a1tke = t.a1tke;
      for (int n = 0; n < hc.nsp; n++) a.a1qx[n] = t.a1qx[n][c];
      if (cfg.idynamic == 2) {
        const NHFields& h = nhf[&t - tiles.data()];
        a.a1pp = h.a1pp; a.a1w = h.a1w; a.ps0 = h.ps0; a.pf0 = h.pf0; a.z0 = h.z0;
      }
      a.pr = t.opr; a.pf3d = t.atms[RCMDYN_ATMS_PF3D - RCMDYN_ATMS_UBX3D]; a.zq = t.atms[RCMDYN_ATMS_ZQ - RCMDYN_ATMS_UBX3D];
      a.omega = t.omega;
      a.out = t.odev; a.mask = mask;
      a.ep2 = AMW / AMD; a.rhmin = cfg.rhmin; a.rhmax = cfg.rhmax;
      const dim3 grid = grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, cfg.kz);
      if (out_prec == 4) KLAUNCH(k_output<float>, grid, BLK, 0, stream, g, dc, a);
      else KLAUNCH(k_output<double>, grid, BLK, 0, stream, g, dc, a);
    });
    HIPCHK(hipEventRecord(ev_out, stream));
    HIPCHK(hipStreamWaitEvent(ostream, ev_out, 0));
    for (auto& t : tiles) {
      size_t n = 0;
      for (int f = 0; f < RCMDYN_NOUT; f++)
        if ((mask >> f) & 1u) n += out_cells(t.g) * out_levels(f);
      if (n) HIPCHK(hipMemcpyAsync(t.ohost, t.odev, n * esz, hipMemcpyDeviceToHost, ostream));
    }
    HIPCHK(hipMemcpyAsync(oflags, ds, sizeof(StepState), hipMemcpyDeviceToHost, ostream));
    HIPCHK(hipEventRecord(ev_copied, ostream));
    out_mask = mask;
    out_lcount = hs.lcount;
  }
  void get_output(int f, void* dst, const Box& b) {
    if (!outon) throw std::runtime_error("rcmdyn_get_output: the output stage is off (rcmdyn_set_output)");
    if (f < 0 || f >= RCMDYN_NOUT) throw std::runtime_error("rcmdyn_get_output: unknown field " + std::to_string(f));
    if (!((out_mask >> f) & 1u))
      throw std::runtime_error(std::string("rcmdyn_get_output: ") + OUT_NAME[f] + " was not in the mask of the last rcmdyn_output_atm");
    wait_output_copy();
    // the steps issued before the snapshot: their sticky flags travelled with it
    if (oflags->nanflag || oflags->slflag) {
      out_mask = 0;
      fail(oflags->slflag, out_lcount, "by step ");
    }
    for (auto& t : tiles) {
      const Geom& g = t.g;
      const int ncj = g.jci2 - g.jci1 + 1, nci = g.ici2 - g.ici1 + 1;
      const Staging s{g.jci1, g.ici1, ncj, nci, ncj, (long)ncj * nci, out_levels(f), t.ooff[f]};
      if (out_prec == 4) gather((float*)dst, b, (const float*)t.ohost, s, g.jci1, g.jci2, g.ici1, g.ici2);
      else gather((double*)dst, b, (const double*)t.ohost, s, g.jci1, g.jci2, g.ici1, g.ici2);
    }
  }

  // Tendency budget of t and qv (idiag = 1): the switch, the host's read and its reset.  The
  // accumulators are allocated (zeroed) on the first use and persist; rw is a kernel argument,
  // so the captured graphs are dropped when it or the switch changes.
  void set_budget(int on, int idgq, double rw) {
    if (on) {
      if (idgq != 1)
        throw std::runtime_error("rcmdyn_set_budget: only the budget of qv (idgq = iqv = 1) is computed");
      if (!(rw > 0.0) || !std::isfinite(rw))
        throw std::runtime_error("rcmdyn_set_budget: rw must be finite and positive");
    }
    quiesce();                                       // a lazy tend replays its graph first
    if (on && !tiles.empty() && !tiles[0].bud[0])
      for (auto& t : tiles)
        for (double*& d : t.bud) d = dalloc(t, t.g.plane * (size_t)cfg.kz);
    const bool b = on != 0;
    if (b != budget || (b && rw != bud_rw)) invalidate_graphs();
    budget = b;
    if (b) bud_rw = rw;
  }
  void get_budget(int term, double* dst, const Box& b) {
    settle();
    if (!budget) throw std::runtime_error("rcmdyn_get_budget: the tendency budget is off (rcmdyn_set_budget)");
    if (term < 0 || term >= RCMDYN_NBUDGET) throw std::runtime_error("rcmdyn_get_budget: unknown budget term");
    get_window(dst, b, cfg.kz, [&](Tile& t) { return t.bud[term]; });
  }
  void reset_budget() {
    settle();
    if (!budget) throw std::runtime_error("rcmdyn_reset_budget: the tendency budget is off (rcmdyn_set_budget)");
    HIPCHK(hipStreamSynchronize(stream));
    for (auto& t : tiles)
      for (double* d : t.bud) HIPCHK(hipMemset(d, 0, t.g.plane * (size_t)cfg.kz * sizeof(double)));
  }

  // SUBEX condensation (condtq, Main/mod_micro_interface.F90:382-493) inside tend: the switch,
  // the host's rh0adj and the read of the last tend's increments.  rh0adj and the three
  // increment arrays are allocated at the first switch-on; the switch selects other kernel
  // instances and conf is a kernel argument, so the captured graphs are dropped when either
  // changes.  A put of rh0adj writes the buffer the graphs already point to.
  void set_condtq(int on, double conf) {
    if (on) {
      if (cfg.ipptls != 1)
        throw std::runtime_error("rcmdyn_set_condtq: condtq belongs to ipptls = 1 (SUBEX); the reference does not call it otherwise");
      if (!(conf > 0.0) || !(conf <= 1.0))
        throw std::runtime_error("rcmdyn_set_condtq: conf must be in (0, 1]");
    }
    quiesce();                                       // a lazy tend replays its graph first
    const bool b = on != 0;
    if (b == condtq && (!b || conf == ct_conf)) return;
    if (b && !tiles.empty() && !tiles[0].rh0adj)
      for (auto& t : tiles) {
        t.rh0adj = dalloc(t, t.g.plane * (size_t)cfg.kz);
        for (double*& d : t.cti) d = dalloc(t, t.g.plane * (size_t)cfg.kz);
      }
    invalidate_graphs();
    if (b && !condtq) rh0_put = false;
    condtq = b;
    if (b) ct_conf = conf;
  }
  void put_rh0adj(const double* src, const Box& b) {
    if (!condtq) throw std::runtime_error("rcmdyn_put_rh0adj: condtq is off (rcmdyn_set_condtq)");
    if (subex)
      throw std::runtime_error("rcmdyn_put_rh0adj: subex is on (rcmdyn_set_subex): condtq reads the rh0adj the device's cldfrac "
                               "forms in the same tend, a put would never be read");
    for (size_t q = 0, n = b.cells(); q < n; q++)
      if (!(src[q] >= 0.0) || !(src[q] <= 0.99999))
        throw std::runtime_error("rcmdyn_put_rh0adj: rh0adj must lie in [0, 0.99999]");
    // as rcmdyn_put scatters a *PHY field: the ghost ring and the wrapped columns of a band (rows
    // in CRM mode) included, since the hydrostatic step computes the forecasts of the ring as
    // their owners do (a pending lazy tend reads the previous values first)
    put_window(src, b, cfg.kz, [](Tile& t) { return t.rh0adj; });
    // tend waits for a put that covers every point condtq runs at, on every level: the interior
    // cross points (gci) of each tile and of its ring, the wrapped ones by their wrapped index.
    // None then reads the zeros of the allocation or the values of an earlier switch-on.  Smaller
    // boxes update the buffer before and after that put.
    const Period p = period();
    bool all = b.k1 <= 1 && b.k2 >= cfg.kz;
    for (const auto& t : tiles) {
      const Geom& g = t.g;
      for (int i = g.icx1(); all && i <= g.icx2(); i++)
        for (int j = g.jcx1(); all && j <= g.jcx2(); j++)
          if (g.gci(j, i) && !b.holds(p.j(j), p.i(i))) all = false;
    }
    if (all) rh0_put = true;
  }
  void get_condtq(int term, double* dst, const Box& b) {
    settle();
    if (!condtq) throw std::runtime_error("rcmdyn_get_condtq: condtq is off (rcmdyn_set_condtq)");
    if (term < 0 || term >= RCMDYN_NCONDTQ) throw std::runtime_error("rcmdyn_get_condtq: unknown term");
    // the increments live on the tile's interior cross points (the ring's are its neighbours')
    if (term == RCMDYN_CONDTQ_RH0ADJ)
      get_window(dst, b, cfg.kz, [&](Tile& t) { return subex ? t.sbx[RCMDYN_SUBEX_RH0ADJ] : t.rh0adj; });
    else get_window(dst, b, cfg.kz, [&](Tile& t) { return t.cti[term - RCMDYN_CONDTQ_T]; }, Range::Interior);
  }

  // ------------------------------------------------------------------ SUBEX on the device
  // cldfrac with subex_cldfrac and the rain columns of subex (rcmdyn_set_subex; subex.hpp,
  // subex.hip) in physical_parametrizations' place: after the mkslice export of a tend and before
  // its tendency kernels.  A whole tend runs the export and the kernels itself (captured with it); on
  // the split path rcmdyn_physics_subex runs them between the two phases, or the post phase does
  // first.  The kernels' increments reach the tendency kernels as the physics sums TPHY + LSC_T ..
  // (phy_tqc), formed by a pointwise pass at the start of the post phase; the tendency kernels are
  // the same instances either way.  The switch changes launches and kernel arguments, so the
  // captured graphs are dropped with it.
  bool subex = false, sbx_rem = false;
  SubexPar sbx_par{};
  double* sbx_chis = nullptr;                  // the chis table (device; lives with the engine)
  bool sbx_tab_put[5] = {};                    // RH0 .. CACCR: a put covered the interior since the switch-on
  bool sbx_pre = false, sbx_ran = false;       // the split path: the pre phase ran; the kernels ran after it
  static constexpr const char* SBX_NAME[RCMDYN_NSUBEX] = {
      "RH0", "QCK1", "CGUL", "CEVAP", "CACCR", "CU_CLDFRA", "CU_CLDLWC", "RAINNC", "LSMRNC", "FCC", "CLDFRA", "CLDLWC",
      "RH0ADJ", "LSC_T", "LSC_QV", "LSC_QC", "TRRATE", "REMRAT", "REMBC"};
  static bool sbx_2d(int f) {
    return f <= RCMDYN_SUBEX_CACCR || f == RCMDYN_SUBEX_RAINNC || f == RCMDYN_SUBEX_LSMRNC || f == RCMDYN_SUBEX_TRRATE;
  }
  static bool sbx_is_rem(int f) { return f == RCMDYN_SUBEX_REMRAT || f == RCMDYN_SUBEX_REMBC; }
  // the pc_physic tendency of t, qv or qc (q = 0, 1, 2) a tendency kernel reads: the host's, or with
  // subex on its sum with the rain columns' increment, or that increment alone where none was put
  double* phy_tqc(const Tile& t, int q) const {
    if (!subex) return t.phy[q];
    return t.phy[q] ? t.sbx_sum[q] : t.sbx[RCMDYN_SUBEX_LSC_T + q];
  }
  void free_subex() {
    for (auto& t : tiles) {
      for (void* p : t.sbx_allocs) (void)hipFree(p);
      t.sbx_allocs.clear();
      for (double*& d : t.sbx) d = nullptr;
      for (double*& d : t.sbx_sum) d = nullptr;
      t.sbx_dqc = nullptr;
    }
  }
  void set_subex(int on, double rhmax, double rhmin, double tc0, int larcticcorr, int iconvlwp, int rem, int icldfrac,
                 int icldmstrat, int lsecind) {
    if (on) {
      const std::string w = "rcmdyn_set_subex: ";
      if (cfg.ipptls != 1)
        throw std::runtime_error(w + "ipptls = " + std::to_string(cfg.ipptls) + ": subex is the scheme of ipptls = 1 alone");
      if (icldfrac != 0)
        throw std::runtime_error(w + "icldfrac = " + std::to_string(icldfrac) + " is not built (subex_cldfrac, icldfrac = 0, alone)");
      if (icldmstrat != 0)
        throw std::runtime_error(w + "icldmstrat = 1 is not built (the marine stratocumulus term needs th700 and iveg)");
      if (lsecind != 0)
        throw std::runtime_error(w + "lsecind is not built (the aerosol second indirect effect needs ccn)");
      if (!std::isfinite(rhmax) || !std::isfinite(rhmin) || !(rhmin >= 0.0) || !(rhmin < rhmax))
        throw std::runtime_error(w + "rhmin and rhmax must be finite with 0 <= rhmin < rhmax");
      if (!std::isfinite(tc0) || !(tc0 > 0.0)) throw std::runtime_error(w + "tc0 must be a finite temperature in K");
      if ((larcticcorr | 1) != 1) throw std::runtime_error(w + "larcticcorr must be 0 or 1");
      if ((iconvlwp | 1) != 1) throw std::runtime_error(w + "iconvlwp must be 0 or 1");
      if ((rem | 1) != 1) throw std::runtime_error(w + "rem must be 0 or 1");
    }
    quiesce();                                       // a lazy tend replays its graph first
    const bool b = on != 0;
    if (!b && !subex) return;
    invalidate_graphs();
    sbx_pre = sbx_ran = false;
    if (subex) free_subex();                         // a new switch-on starts from zeroed buffers
    subex = b;
    if (!b) return;
    sbx_par = SubexPar{rhmax, rhmin, tc0, larcticcorr, iconvlwp};
    sbx_rem = rem != 0;
    for (bool& p : sbx_tab_put) p = false;
    if (!sbx_chis && !dry) {
      std::vector<double> chis(sx::NCHI);
      for (int i = 0; i < sx::NCHI; i++) chis[i] = subex_chis(i);
      HIPCHK(hipMalloc((void**)&sbx_chis, sizeof(double) * sx::NCHI));
      HIPCHK(hipMemcpy(sbx_chis, chis.data(), sizeof(double) * sx::NCHI, hipMemcpyHostToDevice));
    }
    for (auto& t : tiles) {
      const size_t P = t.g.plane;
      for (int f = 0; f < RCMDYN_NSUBEX; f++)
        if (!sbx_is_rem(f) || sbx_rem) t.sbx[f] = zalloc<double>(t.sbx_allocs, P * (sbx_2d(f) ? 1 : (size_t)cfg.kz));
      t.sbx_dqc = zalloc<double>(t.sbx_allocs, P * cfg.kz);
      for (double*& d : t.sbx_sum) d = zalloc<double>(t.sbx_allocs, P * cfg.kz);
    }
  }
  void subex_on(const char* who) const {
    if (!subex) throw std::runtime_error(std::string(who) + ": subex is off (rcmdyn_set_subex)");
  }
  // a run waits for the five tables
  void subex_ready(const char* who) const {
    if (!subex) return;
    for (int f = 0; f < 5; f++)
      if (!sbx_tab_put[f])
        throw std::runtime_error(std::string(who) + ": subex is on and no " + SBX_NAME[f] + " was put since that covers the "
                                 "tiles' interior cross points (rcmdyn_put_subex)");
  }
  void put_subex(int f, const double* src, const Box& b) {
    subex_on("rcmdyn_put_subex");
    if (f < 0 || f >= RCMDYN_NSUBEX) throw std::runtime_error("rcmdyn_put_subex: unknown field");
    if (f > RCMDYN_SUBEX_LSMRNC)
      throw std::runtime_error(std::string("rcmdyn_put_subex: ") + SBX_NAME[f] + " is read-only (the device forms it)");
    const int nk = sbx_2d(f) ? 1 : cfg.kz;
    const size_t n = Box{b.j1, b.j2, b.i1, b.i2, b.k1, std::max(b.k1, b.k2)}.cells();
    for (size_t q = 0; q < n; q++) {
      if (!std::isfinite(src[q])) throw std::runtime_error(std::string("rcmdyn_put_subex: ") + SBX_NAME[f] + " must be finite");
      if (f == RCMDYN_SUBEX_CU_CLDFRA && (!(src[q] >= 0.0) || !(src[q] <= 1.0)))
        throw std::runtime_error("rcmdyn_put_subex: CU_CLDFRA must lie in [0, 1]");
    }
    put_window(src, b, nk, [&](Tile& t) { return t.sbx[f]; });
    if (f <= RCMDYN_SUBEX_CACCR) {
      const Period p = period();
      bool all = true;
      for (const auto& t : tiles) {
        const Geom& g = t.g;
        for (int i = g.ici1; all && i <= g.ici2; i++)
          for (int j = g.jci1; all && j <= g.jci2; j++)
            if (!b.holds(p.j(j), p.i(i))) all = false;
      }
      if (all) sbx_tab_put[f] = true;
    }
  }
  void get_subex(int f, double* dst, const Box& b) {
    settle();
    subex_on("rcmdyn_get_subex");
    if (f < 0 || f >= RCMDYN_NSUBEX) throw std::runtime_error("rcmdyn_get_subex: unknown field");
    if (f < RCMDYN_SUBEX_RAINNC)
      throw std::runtime_error(std::string("rcmdyn_get_subex: ") + SBX_NAME[f] + " is the host's own (put only)");
    if (sbx_is_rem(f) && !sbx_rem)
      throw std::runtime_error(std::string("rcmdyn_get_subex: ") + SBX_NAME[f] + " needs rem = 1 (rcmdyn_set_subex)");
    get_window(dst, b, sbx_2d(f) ? 1 : cfg.kz, [&](Tile& t) { return t.sbx[f]; }, Range::Interior);
  }
  // the two kernels on the mkslice export of this tend, then rh0adj and the increments one point
  // wide to the tiles' rings: condtq and the tendency kernels of a decomposed hydrostatic step
  // compute the ring as its owners do
  void run_subex() {
    each([&](Tile& t) {
      const Geom& g = t.g;
      SubexArgs a{};
      a.tb = t.atms[4]; a.qv = t.atms[5]; a.qc = t.atms[6]; a.pb = t.atms[8]; a.pf = t.atms[9]; a.rho = t.atms[13];
      a.rh = t.atms[21]; a.psb = t.psb_[t.cur];
      double** s = t.sbx;
      a.rh0 = s[RCMDYN_SUBEX_RH0]; a.qck1 = s[RCMDYN_SUBEX_QCK1]; a.cgul = s[RCMDYN_SUBEX_CGUL];
      a.cevap = s[RCMDYN_SUBEX_CEVAP]; a.caccr = s[RCMDYN_SUBEX_CACCR];
      a.cufra = s[RCMDYN_SUBEX_CU_CLDFRA]; a.culwc = s[RCMDYN_SUBEX_CU_CLDLWC]; a.chis = sbx_chis;
      a.fcc = s[RCMDYN_SUBEX_FCC]; a.cldfra = s[RCMDYN_SUBEX_CLDFRA]; a.cldlwc = s[RCMDYN_SUBEX_CLDLWC];
      a.rh0adj = s[RCMDYN_SUBEX_RH0ADJ]; a.dqc = t.sbx_dqc;
      a.lsc_t = s[RCMDYN_SUBEX_LSC_T]; a.lsc_qv = s[RCMDYN_SUBEX_LSC_QV]; a.lsc_qc = s[RCMDYN_SUBEX_LSC_QC];
      a.rainnc = s[RCMDYN_SUBEX_RAINNC]; a.lsmrnc = s[RCMDYN_SUBEX_LSMRNC]; a.trrate = s[RCMDYN_SUBEX_TRRATE];
      a.remrat = s[RCMDYN_SUBEX_REMRAT]; a.rembc = s[RCMDYN_SUBEX_REMBC];
      a.par = sbx_par; a.dtsec = cfg.dtsec;
      const int nj = g.jci2 - g.jci1 + 1, ni = g.ici2 - g.ici1 + 1;
      if (nj <= 0 || ni <= 0) return;
      KLAUNCH(k_subex_point, grid3(nj, ni, cfg.kz), BLK, 0, stream, g, cfg.kz, a);
      const size_t lds = sbx_rem ? sizeof(double) * SBX_COLW * (size_t)cfg.kz : 0;
      KLAUNCH(k_subex_column, dim3((nj + SBX_COLW - 1) / SBX_COLW, ni), dim3(SBX_COLW), lds, stream, g, cfg.kz, ds, a);
    });
    xch({{FK::SBX_RH0ADJ, cfg.kz}, {FK::SBX_LSCT, cfg.kz}, {FK::SBX_LSCQV, cfg.kz}, {FK::SBX_LSCQC, cfg.kz}}, 1, 0);
  }
  // TPHY + LSC_T, QVPHY + LSC_QV, QCPHY + LSC_QC over the whole frame (the host put the ring too)
  void subex_sums() {
    each([&](Tile& t) {
      if (!t.phy[0]) return;
      const long n = t.g.plane * (long)cfg.kz;
      double** s = t.sbx;
      KLAUNCH(k_subex_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, t.phy[0], t.phy[1], t.phy[2],
              s[RCMDYN_SUBEX_LSC_T], s[RCMDYN_SUBEX_LSC_QV], s[RCMDYN_SUBEX_LSC_QC], t.sbx_sum[0], t.sbx_sum[1], t.sbx_sum[2]);
    });
  }
  // between the two phases of a tend whose pre phase ran the mkslice export (tend, nh_tend)
  void subex_mid(int phase) {
    if (!subex) return;
    if (phase == TEND_PRE) { sbx_pre = true; sbx_ran = false; return; }
    if (phase == TEND_ALL || !sbx_ran) run_subex();
    sbx_pre = sbx_ran = false;
    subex_sums();
  }
  void physics_subex() {
    subex_on("rcmdyn_physics_subex");
    subex_ready("rcmdyn_physics_subex");
    if (!sbx_pre)
      throw std::runtime_error("rcmdyn_physics_subex: no rcmdyn_tend_pre_physics since the last tend (the mkslice export "
                               "subex reads is that call's)");
    if (sbx_ran) return;                             // once per tend
    run_subex();
    sbx_ran = true;
  }

  // ------------------------------------------------------------------ chemical tracers
  // The chi chain of tend and bdyval (rcmdyn_set_tracers; species.hip's FamTr instances).  The
  // family is declared after create, like the budget and condtq: the count is no field of
  // rcmdyn_config.  Its buffers are the tiles' (Tile::tra1 ..), the two relaxation tables the
  // engine's; the groups' argument tables are kernel inputs in device memory, so a put writes
  // buffers the captured graphs already point to and only a new count or a new table state (zero
  // or not) drops the graphs (the slice runs eagerly, from rcmdyn_tend_pre_physics, or with subex
  // on inside a whole tend, whose capture allocates the chib3d buffers before it begins).
  int ntr = 0;
  bool tr_bdy_dirty = false;          // chib0 / chibt put since the last tend: their ghost rings are stale
  bool tr_relax = false;              // a cefc / cegc entry is non-zero
  double *tr_cefc = nullptr, *tr_cegc = nullptr;
  int tr_groups() const { return (ntr + NQXH - 1) / NQXH; }
  TrArgs tr_args(Tile& t) {
    TrArgs a{};
    a.tab = static_cast<const QxArgs*>(t.trtab[cfg.idynamic == 2 ? 0 : t.cur]);
    a.cefc = tr_cefc; a.cegc = tr_cegc;
    a.ngroups = tr_groups();
    a.relax = (int)(tr_relax && (cfg.iboudy == 1 || cfg.iboudy == 5));     // Main/mod_tendency.F90:1506
    return a;
  }
  // the halo staging of a tile's widest grouped exchange, 8 directions: the hydrostatic prologue's
  // 31 (nqx = 5: 46) field-widths of at most kz + 1 levels (setup_tile), and 5 more per tracer
  // (atm1 2 wide, atm2 3 wide; rcmdyn_set_tracers)
  long staging_need(const Geom& g, int ntracers) const {
    return 8L * (std::max(g.nj, g.ni) + 2 * G) * (32 + 16 * (hc.nsp > 0) + 5 * ntracers) * (cfg.kz + 1);
  }
  void grow_staging(int ntracers) {
    if (!halo) return;
    long need = staging_cap;
    for (auto& t : tiles) need = std::max(need, staging_need(t.g, ntracers));
    if (need <= staging_cap) return;
    staging_cap = need;
    for (auto& t : tiles)
      for (double** b : {&t.sbuf, &t.rbuf, &t.sbuf2, &t.rbuf2}) {
        if (!*b) continue;
        t.allocs.erase(std::find(t.allocs.begin(), t.allocs.end(), (void*)*b));
        HIPCHK(hipFree(*b));
        *b = dalloc(t, staging_cap);
      }
  }
  void free_tracers() {
    che_free();                                      // the CHE output stage goes with its tracers
    for (auto& t : tiles) {
      for (void* p : t.tr_allocs) (void)hipFree(p);
      t.tr_allocs.clear();
      for (auto* v : {&t.tra1[0], &t.tra1[1], &t.tra2[0], &t.tra2[1], &t.trcq, &t.trfq, &t.trphy, &t.trb0, &t.trbt,
                      &t.trs3d})
        v->clear();
      t.trdep = t.trdepf = nullptr;
      t.trtab[0] = t.trtab[1] = nullptr;
      t.trsout = nullptr;
      t.cum[0] = t.cum[1] = t.cum[2] = nullptr;
      t.trbud.clear();
      t.trbudtab = nullptr;
    }
    cumtran = trbudget = false;
    if (tr_cefc) (void)hipFree(tr_cefc);
    if (tr_cegc) (void)hipFree(tr_cegc);
    tr_cefc = tr_cegc = nullptr;
    tr_relax = false;
    ntr = 0;
  }
  void set_tracers(int n, int ichebdy) {
    if (n < 0 || n > RCMDYN_MAXTR)
      throw std::runtime_error("rcmdyn_set_tracers: ntr must lie in 0 .. RCMDYN_MAXTR = " + std::to_string(RCMDYN_MAXTR));
    if (n > 0) {
      if (ichebdy != 1)
        throw std::runtime_error("rcmdyn_set_tracers: ichebdy must be 1 (the ichebdy = 0 relaxation indexes tile-local "
                                 "rows, Main/chemlib/mod_che_bdyco.F90:808-896: its result depends on the decomposition)");
      if (cfg.idiffu == 3)
        throw std::runtime_error("rcmdyn_set_tracers: idiffu = 3 is not built for tracers (no sixth-order column planes of chi)");
      if (cfg.isladvec == 1)
        throw std::runtime_error("rcmdyn_set_tracers: isladvec = 1 is not built for tracers (slhadv_x of chi)");
    }
    quiesce();                                       // a lazy tend replays its graph first
    if (n == ntr) return;
    invalidate_graphs();
    free_tracers();
    if (n == 0) return;
    try {
      grow_staging(n);
      const int kz = cfg.kz, ng = (n + NQXH - 1) / NQXH, npar = cfg.idynamic == 2 ? 1 : 2;
      HIPCHK(hipMalloc((void**)&tr_cefc, sizeof(double) * cfg.nspgx * kz));
      HIPCHK(hipMalloc((void**)&tr_cegc, sizeof(double) * cfg.nspgx * kz));
      HIPCHK(hipMemset(tr_cefc, 0, sizeof(double) * cfg.nspgx * kz));
      HIPCHK(hipMemset(tr_cegc, 0, sizeof(double) * cfg.nspgx * kz));
      for (auto& t : tiles) {
        const Geom& g = t.g;
        const size_t P3 = (size_t)g.plane * kz;
        const int R = g.ici2 - g.ici1 + 1;
        for (int q = 0; q < n; q++) {
          for (int b = 0; b < npar; b++) {
            t.tra1[b].push_back(tr_alloc<double>(t, P3));
            t.tra2[b].push_back(tr_alloc<double>(t, P3));
          }
          t.trcq.push_back(tr_alloc<double>(t, P3)); t.trfq.push_back(tr_alloc<double>(t, P3));
          t.trphy.push_back(tr_alloc<double>(t, P3));
          t.trb0.push_back(tr_alloc<double>(t, P3)); t.trbt.push_back(tr_alloc<double>(t, P3));
          t.trs3d.push_back(nullptr);
        }
        t.trdep = tr_alloc<unsigned>(t, (size_t)ng * NQXH * kz * negfix_rowwords(g));
        t.trdepf = tr_alloc<unsigned>(t, (size_t)ng * NQXH * kz * R);
        t.trsout = tr_alloc<double*>(t, n);
        for (int b = 0; b < npar; b++) {
          std::vector<QxArgs> tab(ng);
          for (int gq = 0; gq < ng; gq++) {
            QxArgs& q = tab[gq];
            q = QxArgs{};
            q.nsp = std::min(NQXH, n - gq * NQXH);
            for (int m = 0; m < q.nsp; m++) {
              const int x = gq * NQXH + m, o = npar == 1 ? b : 1 - b;
              q.a1[m] = t.tra1[b][x]; q.a2[m] = t.tra2[b][x];
              q.b1[m] = t.tra1[o][x]; q.b2[m] = t.tra2[o][x];
              q.cq[m] = t.trcq[x]; q.fq[m] = t.trfq[x]; q.phy[m] = t.trphy[x];
              q.b0[m] = t.trb0[x]; q.bt[m] = t.trbt[x];
            }
            q.dep = t.trdep + (size_t)gq * NQXH * kz * negfix_rowwords(g);
            q.depf = t.trdepf + (size_t)gq * NQXH * kz * R;
          }
          t.trtab[b] = tr_alloc<QxArgs>(t, ng);
          HIPCHK(hipMemcpy(t.trtab[b], tab.data(), sizeof(QxArgs) * ng, hipMemcpyHostToDevice));
        }
      }
      ntr = n;
    } catch (...) {
      free_tracers();
      throw;
    }
    ghosts_stale = true;
  }
  // the buffer of one tracer field on tile t (TR_CHIB3D: null before the first slice)
  double* tracer_ptr(Tile& t, int field, int x) {
    const int c = cfg.idynamic == 2 ? 0 : t.cur;
    switch (field) {
      case RCMDYN_TR_ATM1: return t.tra1[c][x]; case RCMDYN_TR_ATM2: return t.tra2[c][x];
      case RCMDYN_TR_PHY: return t.trphy[x]; case RCMDYN_TR_B0: return t.trb0[x]; case RCMDYN_TR_BT: return t.trbt[x];
      case RCMDYN_TR_CHIB3D: return t.trs3d[x];
      default: return nullptr;
    }
  }
  void tracer_check(const char* who, int field, int itr) const {
    if (ntr == 0) throw std::runtime_error(std::string(who) + ": no tracers are declared (rcmdyn_set_tracers)");
    if (field < 0 || field >= RCMDYN_NTRFIELDS) throw std::runtime_error(std::string(who) + ": unknown tracer field");
    if (itr < 1 || itr > ntr)
      throw std::runtime_error(std::string(who) + ": itr must lie in 1 .. ntr = " + std::to_string(ntr));
  }
  void put_tracer(int field, int itr, const double* src, const Box& b) {
    tracer_check("rcmdyn_put_tracer", field, itr);
    if (field == RCMDYN_TR_CHIB3D) throw std::runtime_error("rcmdyn_put_tracer: TR_CHIB3D is read-only (the mkslice export)");
    put_window(src, b, cfg.kz, [&](Tile& t) { return tracer_ptr(t, field, itr - 1); });
    if (field == RCMDYN_TR_B0 || field == RCMDYN_TR_BT) tr_bdy_dirty = true;
    else ghosts_stale = true;
  }
  void get_tracer(int field, int itr, double* dst, const Box& b) {
    tracer_check("rcmdyn_get_tracer", field, itr);
    if (field == RCMDYN_TR_PHY) throw std::runtime_error("rcmdyn_get_tracer: TR_PHY is put-only (the host's chiphy)");
    settle();
    if (field == RCMDYN_TR_CHIB3D && !tiles.empty() && !tiles[0].trs3d[itr - 1])
      throw std::runtime_error("rcmdyn_get_tracer: no slice fields yet (rcmdyn_tend_pre_physics)");
    get_window(dst, b, cfg.kz, [&](Tile& t) { return tracer_ptr(t, field, itr - 1); });
  }
  void put_tracer_nudge(const double* cefc, const double* cegc) {
    if (ntr == 0) throw std::runtime_error("rcmdyn_put_tracer_nudge: no tracers are declared (rcmdyn_set_tracers)");
    if (!cefc || !cegc) throw std::runtime_error("rcmdyn_put_tracer_nudge: null table");
    const size_t n = (size_t)cfg.nspgx * cfg.kz;
    bool nz = false;
    for (size_t q = 0; q < n; q++) {
      if (!std::isfinite(cefc[q]) || !std::isfinite(cegc[q]))
        throw std::runtime_error("rcmdyn_put_tracer_nudge: the tables must be finite");
      nz = nz || cefc[q] != 0.0 || cegc[q] != 0.0;
    }
    quiesce();
    HIPCHK(hipMemcpy(tr_cefc, cefc, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(tr_cegc, cegc, n * sizeof(double), hipMemcpyHostToDevice));
    if (nz != tr_relax) invalidate_graphs();         // the term's switch is a kernel argument
    tr_relax = nz;
  }
  // Cumulus mixing of the tracers (cumtran, Main/chemlib/mod_che_cumtran.F90:118-167) inside tend:
  // the switch, the host's three inputs and their read.  The inputs are the tiles' (Tile::cum,
  // allocated at the first switch-on, freed with the tracers, zeroed at every switch-on from off);
  // ncum is a kernel argument, so the captured graphs are dropped when it or the switch changes.  A
  // put writes the buffers the graphs already point to.
  bool cumtran = false;
  int cum_ncum = 1;
  void set_cumtran(int on, int ncum) {
    if (on) {
      if (ntr == 0) throw std::runtime_error("rcmdyn_set_cumtran: no tracers are declared (rcmdyn_set_tracers)");
      if (ncum < 1) throw std::runtime_error("rcmdyn_set_cumtran: ncum must be at least 1 (dtcum / dtsec in steps)");
    }
    quiesce();                                       // a lazy tend replays its graph first
    const bool b = on != 0;
    if (b == cumtran && (!b || ncum == cum_ncum)) return;
    if (b && !cumtran)
      for (auto& t : tiles)
        for (int q = 0; q < RCMDYN_NCUMFIELDS; q++) {
          const size_t n = (size_t)t.g.plane * cum_levels(q);
          if (!t.cum[q]) t.cum[q] = tr_alloc<double>(t, n);
          else HIPCHK(hipMemset(t.cum[q], 0, n * sizeof(double)));
        }
    invalidate_graphs();
    cumtran = b;
    if (b) cum_ncum = ncum;
  }
  int cum_levels(int field) const { return field == RCMDYN_CUM_CLDFRA ? cfg.kz : 1; }
  void cumtran_check(const char* who, int field) const {
    if (!cumtran) throw std::runtime_error(std::string(who) + ": cumtran is off (rcmdyn_set_cumtran)");
    if (field < 0 || field >= RCMDYN_NCUMFIELDS) throw std::runtime_error(std::string(who) + ": unknown cumtran field");
  }
  // a one-level field is level 1 whatever k1, k2 say
  Box cum_box(int field, const Box& b) const {
    return cum_levels(field) == 1 ? Box{b.j1, b.j2, b.i1, b.i2, 1, 1} : b;
  }
  void put_cumtran(int field, const double* src, const Box& host) {
    cumtran_check("rcmdyn_put_cumtran", field);
    const Box b = cum_box(field, host);
    for (size_t q = 0, n = b.cells(); q < n; q++) {
      const double v = src[q];
      if (field == RCMDYN_CUM_DOTRAN && v != 0.0 && v != 1.0)
        throw std::runtime_error("rcmdyn_put_cumtran: CUM_DOTRAN must hold 0 or 1");
      if (field == RCMDYN_CUM_KTOP && (!(v >= 0.0) || !(v <= cfg.kz) || v != std::floor(v)))
        throw std::runtime_error("rcmdyn_put_cumtran: CUM_KTOP must hold integers in 0 .. kz");
      if (field == RCMDYN_CUM_CLDFRA && (!(v >= 0.0) || !(v <= 1.0)))
        throw std::runtime_error("rcmdyn_put_cumtran: CUM_CLDFRA must be finite and lie in [0, 1]");
    }
    // (a pending lazy tend reads the previous values first)
    put_window(src, b, cum_levels(field), [&](Tile& t) { return t.cum[field]; });
  }
  void get_cumtran(int field, double* dst, const Box& host) {
    cumtran_check("rcmdyn_get_cumtran", field);
    get_window(dst, cum_box(field, host), cum_levels(field), [&](Tile& t) { return t.cum[field]; });
  }
  TrCum cum_args(const Tile& t) const {
    return TrCum{t.cum[0], t.cum[1], t.cum[2], trbudget ? t.trbudtab + RCMDYN_TRDIAG_CONV * ntr : nullptr, trb_cfdout,
                 cum_ncum};
  }

  // Tracer budget (ichdiag > 0): the switch, the host's read and its reset.  The accumulators
  // [term][tracer] are the tiles' (allocated at the first switch-on, freed with the tracers, zeroed
  // at every switch-on from off), their pointer table a device array; rw and cfdout are kernel
  // arguments and the switch selects other kernel instances, so the captured graphs are dropped when
  // any of them changes.
  bool trbudget = false;
  double trb_rw = 1.0, trb_cfdout = 1.0;
  void set_tracer_budget(int on, double rw, double cfdout) {
    if (on) {
      if (ntr == 0) throw std::runtime_error("rcmdyn_set_tracer_budget: no tracers are declared (rcmdyn_set_tracers)");
      if (!std::isfinite(rw)) throw std::runtime_error("rcmdyn_set_tracer_budget: rw must be finite");
      if (!std::isfinite(cfdout)) throw std::runtime_error("rcmdyn_set_tracer_budget: cfdout must be finite");
    }
    quiesce();                                       // a lazy tend replays its graph first
    const bool b = on != 0;
    if (b == trbudget && (!b || (rw == trb_rw && cfdout == trb_cfdout))) return;
    if (b && !trbudget)
      for (auto& t : tiles) {
        const size_t P3 = (size_t)t.g.plane * cfg.kz;
        if (t.trbud.empty()) {
          for (int q = 0; q < NTRBUDTERM * ntr; q++) t.trbud.push_back(tr_alloc<double>(t, P3));
          t.trbudtab = tr_alloc<double*>(t, t.trbud.size());
          HIPCHK(hipMemcpy(t.trbudtab, t.trbud.data(), sizeof(double*) * t.trbud.size(), hipMemcpyHostToDevice));
        } else {
          for (double* d : t.trbud) HIPCHK(hipMemset(d, 0, P3 * sizeof(double)));
        }
      }
    invalidate_graphs();
    trbudget = b;
    if (b) { trb_rw = rw; trb_cfdout = cfdout; }
  }
  void get_tracer_budget(int term, int itr, double* dst, const Box& b) {
    if (!trbudget) throw std::runtime_error("rcmdyn_get_tracer_budget: the tracer budget is off (rcmdyn_set_tracer_budget)");
    if (term < 0 || term >= RCMDYN_NTRDIAG) throw std::runtime_error("rcmdyn_get_tracer_budget: unknown budget term");
    if (itr < 1 || itr > ntr)
      throw std::runtime_error("rcmdyn_get_tracer_budget: itr must lie in 1 .. ntr = " + std::to_string(ntr));
    get_window(dst, b, cfg.kz, [&](Tile& t) { return t.trbud[term * ntr + itr - 1]; });
  }
  void reset_tracer_budget() {
    if (!trbudget) throw std::runtime_error("rcmdyn_reset_tracer_budget: the tracer budget is off (rcmdyn_set_tracer_budget)");
    quiesce();
    for (auto& t : tiles)
      for (double* d : t.trbud) HIPCHK(hipMemset(d, 0, (size_t)t.g.plane * cfg.kz * sizeof(double)));
  }
  TrBudget trbud_args(const Tile& t) const { return TrBudget{t.trbudtab, trb_rw, ntr}; }

  // ------------------------------------------------------------------ CHE output stream
  // The tracer fields of the CHE file that the dyn core owns (che_output.hip), off by default and
  // outside the captured step.  rcmdyn_output_che forms the requested fields of a batch of tracers
  // on the compute stream into one of two buffer sets (a compact device buffer and its pinned twin
  // per tile) and copies it on the stage's copy stream behind an event, with the step's sticky
  // error flags of that moment; the sets alternate, so a call waits only for the copy issued two
  // calls back, and rcmdyn_get_output_che waits for the copy of the snapshot it serves alone.  The
  // stream is the stage's own: a CHE batch is many times an ATM record, which would queue behind it
  // on rcmdyn_output_atm's.  Neither stage can wait on the other: a copy stream waits only for an
  // event recorded on the compute stream, the compute stream for no copy stream, the host for copy
  // events already recorded.  The buffers are freed with the tracers and at a switch-off.
  struct CheSlot {
    hipEvent_t ev_out = nullptr, ev_copied = nullptr;
    StepState* flags = nullptr;       // pinned: the device clock and flags at the snapshot
    std::vector<void*> dev, host;     // per tile
    uint32_t mask = 0;                // the fields of the snapshot (0: none)
    int itr1 = 0, itr2 = 0;           // its tracers
    long long lcount = 0;             // its clock
    unsigned long seq = 0;            // its place in the order of the calls
  };
  bool cheon = false;
  int che_prec = 8, che_nbatch = 0;
  unsigned long che_seq = 0;
  hipStream_t cstream = nullptr;
  CheSlot che[2];
  static constexpr const char* CHE_NAME[RCMDYN_NCHE] = {"CHE_MIXRAT", "CHE_BURDEN", "CHE_ADVH", "CHE_ADVV",
                                                        "CHE_BDY",    "CHE_DIFH",   "CHE_CONV"};
  // elements one tracer of a snapshot with this mask takes on a tile, and where field f starts in them
  size_t che_stride(const Geom& g, uint32_t mask, int upto = RCMDYN_NCHE) const {
    size_t n = 0;
    if (g.jci2 < g.jci1 || g.ici2 < g.ici1) return n;
    for (int f = 0; f < upto; f++)
      if ((mask >> f) & 1u) n += out_cells(g) * che_levels(f, cfg.kz);
    return n;
  }
  void che_free() {
    for (CheSlot& s : che) {
      if (s.ev_copied) (void)hipEventSynchronize(s.ev_copied);
      for (void* p : s.dev) (void)hipFree(p);
      for (void* p : s.host) (void)hipHostFree(p);
      s.dev.clear(); s.host.clear();
      s.mask = 0;
    }
    cheon = false;
  }
  void che_destroy() {
    che_free();
    if (!cstream) return;
    (void)hipStreamSynchronize(cstream);
    for (CheSlot& s : che) {
      (void)hipEventDestroy(s.ev_out);
      (void)hipEventDestroy(s.ev_copied);
      (void)hipHostFree(s.flags);
      s = CheSlot{};
    }
    (void)hipStreamDestroy(cstream);
    cstream = nullptr;
  }
  void set_output_che(int on, int prec, int nbatch) {
    if (on) {
      if (ntr == 0) throw std::runtime_error("rcmdyn_set_output_che: no tracers are declared (rcmdyn_set_tracers)");
      if (prec != 4 && prec != 8)
        throw std::runtime_error("rcmdyn_set_output_che: prec = " + std::to_string(prec) + " is neither 4 (float) nor 8 (double)");
      if (nbatch < 1 || nbatch > ntr)
        throw std::runtime_error("rcmdyn_set_output_che: nbatch = " + std::to_string(nbatch) + " must lie in 1 .. ntr = " +
                                 std::to_string(ntr));
      if (cheon && prec == che_prec && nbatch == che_nbatch) return;      // the same switch: the snapshots are kept
    }
    che_free();                       // waits for both copies; both snapshots are forgotten
    if (!on) return;
    if (!cstream) {
      HIPCHK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
      for (CheSlot& s : che) {
        HIPCHK(hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s.ev_copied, hipEventDisableTiming));
        HIPCHK(hipHostMalloc((void**)&s.flags, sizeof(StepState), hipHostMallocDefault));
        std::memset(s.flags, 0, sizeof(StepState));
      }
    }
    try {
      // room for every field of nbatch tracers: one plane and RCMDYN_NCHE - 1 fields of kz levels
      for (CheSlot& s : che)
        for (auto& t : tiles) {
          const size_t bytes = std::max<size_t>(che_stride(t.g, (1u << RCMDYN_NCHE) - 1) * nbatch * prec, 8);
          void *d = nullptr, *p = nullptr;
          HIPCHK(hipMalloc(&d, bytes));
          s.dev.push_back(d);
          HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
          s.host.push_back(p);
        }
    } catch (...) {
      che_free();
      throw;
    }
    cheon = true;
    che_prec = prec;
    che_nbatch = nbatch;
  }
  void output_che(uint32_t mask, int itr1, int itr2) {
    if (!cheon) throw std::runtime_error("rcmdyn_output_che: the CHE output stage is off (rcmdyn_set_output_che)");
    if (mask == 0) throw std::runtime_error("rcmdyn_output_che: mask = 0 names no field");
    if (mask >> RCMDYN_NCHE)
      throw std::runtime_error("rcmdyn_output_che: mask = " + std::to_string(mask) + " has a bit beyond the last field (" +
                               std::to_string(RCMDYN_NCHE - 1) + ")");
    if (itr1 < 1 || itr2 > ntr || itr1 > itr2)
      throw std::runtime_error("rcmdyn_output_che: itr1 = " + std::to_string(itr1) + ", itr2 = " + std::to_string(itr2) +
                               " must satisfy 1 <= itr1 <= itr2 <= ntr = " + std::to_string(ntr));
    if (itr2 - itr1 + 1 > che_nbatch)
      throw std::runtime_error("rcmdyn_output_che: itr1 .. itr2 holds " + std::to_string(itr2 - itr1 + 1) +
                               " tracers, more than nbatch = " + std::to_string(che_nbatch) + " (rcmdyn_set_output_che)");
    for (int f = RCMDYN_CHE_ADVH; f < RCMDYN_NCHE; f++)
      if (((mask >> f) & 1u) && !trbudget)
        throw std::runtime_error(std::string("rcmdyn_output_che: ") + CHE_NAME[f] +
                                 ": the tracer budget is off (rcmdyn_set_tracer_budget)");
    const bool burden = (mask >> RCMDYN_CHE_BURDEN) & 1u;
    if (burden && !tiles.empty() && !(have(fieldtab::SLICE) && tiles[0].trs3d[0]))
      throw std::runtime_error(std::string("rcmdyn_output_che: CHE_BURDEN: ") + WAITS_FOR[fieldtab::SLICE]);
    settle();                         // a lazy tend replays its graph first
    CheSlot& s = che[che_seq & 1];
    HIPCHK(hipEventSynchronize(s.ev_copied));      // the copy issued two calls back leaves the set first
    s.mask = 0;
    const int nb = itr2 - itr1 + 1;
    const bool nh = cfg.idynamic == 2;
    each([&](Tile& t) {
      const Geom& g = t.g;
      if (g.jci2 < g.jci1 || g.ici2 < g.ici1) return;
      const size_t ti = &t - tiles.data();
      CheArgs a{};
      for (int f = 0; f < RCMDYN_NCHE; f++) a.off[f] = (long)che_stride(g, mask, f);
      a.stride = (long)che_stride(g, mask);
      a.psb = t.psb_[t.cur];
      a.tab = tr_args(t).tab;
      a.acc = trbudget ? t.trbudtab : nullptr;
      if (burden) {
        a.chib3d = t.trsout;
        a.rhob3d = t.atms[RCMDYN_ATMS_RHOB3D - RCMDYN_ATMS_UBX3D];
        if (nh) a.zf0 = nhf[ti].zf0;
        else a.dzq = t.atms[RCMDYN_ATMS_DZQ - RCMDYN_ATMS_UBX3D];
      }
      a.out = s.dev[ti];
      a.mask = mask; a.itr0 = itr1 - 1; a.nb = nb; a.ntr = ntr;
      const dim3 grid = grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, cfg.kz * nb);
      if (che_prec == 4) KLAUNCH(k_output_che<float>, grid, BLK, 0, stream, g, cfg.kz, a);
      else KLAUNCH(k_output_che<double>, grid, BLK, 0, stream, g, cfg.kz, a);
    });
    HIPCHK(hipEventRecord(s.ev_out, stream));
    HIPCHK(hipStreamWaitEvent(cstream, s.ev_out, 0));
    for (size_t ti = 0; ti < tiles.size(); ti++) {
      const size_t n = che_stride(tiles[ti].g, mask) * nb;
      if (n) HIPCHK(hipMemcpyAsync(s.host[ti], s.dev[ti], n * (size_t)che_prec, hipMemcpyDeviceToHost, cstream));
    }
    HIPCHK(hipMemcpyAsync(s.flags, ds, sizeof(StepState), hipMemcpyDeviceToHost, cstream));
    HIPCHK(hipEventRecord(s.ev_copied, cstream));
    s.mask = mask; s.itr1 = itr1; s.itr2 = itr2;
    s.lcount = hs.lcount;
    s.seq = ++che_seq;
  }
  void get_output_che(int f, int itr, void* dst, const Box& b) {
    if (!cheon) throw std::runtime_error("rcmdyn_get_output_che: the CHE output stage is off (rcmdyn_set_output_che)");
    if (f < 0 || f >= RCMDYN_NCHE) throw std::runtime_error("rcmdyn_get_output_che: unknown field " + std::to_string(f));
    CheSlot* s = nullptr;
    for (CheSlot& c : che)
      if (((c.mask >> f) & 1u) && itr >= c.itr1 && itr <= c.itr2 && (!s || c.seq > s->seq)) s = &c;
    if (!s)
      throw std::runtime_error(std::string("rcmdyn_get_output_che: ") + CHE_NAME[f] + " of tracer " + std::to_string(itr) +
                               " is in neither of the two held snapshots of rcmdyn_output_che");
    HIPCHK(hipEventSynchronize(s->ev_copied));
    // the steps issued before the snapshot: their sticky flags travelled with it
    if (s->flags->nanflag || s->flags->slflag) {
      const int sl = s->flags->slflag;
      const long long lc = s->lcount;
      for (CheSlot& c : che) c.mask = 0;
      fail(sl, lc, "by step ");
    }
    for (size_t ti = 0; ti < tiles.size(); ti++) {
      const Geom& g = tiles[ti].g;
      const int ncj = g.jci2 - g.jci1 + 1, nci = g.ici2 - g.ici1 + 1;
      const long off = (long)(che_stride(g, s->mask) * (size_t)(itr - s->itr1) + che_stride(g, s->mask, f));
      const Staging st{g.jci1, g.ici1, ncj, nci, ncj, (long)ncj * nci, che_levels(f, cfg.kz), off};
      if (che_prec == 4) gather((float*)dst, b, (const float*)s->host[ti], st, g.jci1, g.jci2, g.ici1, g.ici2);
      else gather((double*)dst, b, (const double*)s->host[ti], st, g.jci1, g.jci2, g.ici1, g.ici2);
    }
  }

  // tend's tracer launches after the forecast's exchange: the fix and filter, the serial chains,
  // then (cumtran on) the cumulus mixing of the filtered levels, ahead of the step's clock advance
  void tracer_fix(Tile& t) {
    const Geom& g = t.g;
    const int kz = cfg.kz, ng = tr_groups();
    KLAUNCH_AS("k_tr_fix", k_qx_fix<FamTr>, grid3(g.jdx2() - g.jdx1() + 1, g.idx2() - g.idx1() + 1, ng * kz), BLK, 0,
               stream, g, dc, tr_args(t));
    KLAUNCH_AS("k_tr_serial", k_qx_serial<FamTr>, dim3(ng * NQXH * kz), dim3(negfix_threads(g)),
               sizeof(double) * negfix_lds(g), stream, g, dc, tr_args(t));
    KLAUNCH_AS("k_tr_post", k_qx_post<FamTr>, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, ng * NQXH * kz), BLK, 0,
               stream, g, dc, tr_args(t));
    if (cumtran)
      KLAUNCH(k_tr_cumtran, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, ntr), BLK, 0, stream, g, dc, ds, tr_args(t),
              ntr, cum_args(t));
  }
  // chem_bdyval_coupled of every tile; integ / pre_clock as k_bdyval_chi
  void tracer_bdyval(int integ, int pre_clock) {
    if (!ntr) return;
    each([&](Tile& t) {
      KLAUNCH(k_bdyval_chi, dim3(cfg.kz, ntr), dim3(256), 0, stream, t.g, ds, tr_args(t), ntr, integ, pre_clock,
              cfg.dtsec);
    });
  }
  // mkslice's chib3d (run_slice)
  void tracer_slice_allocs() {
    if (!ntr || dry) return;
    for (auto& t : tiles) {
      if (t.trs3d[0]) continue;
      for (int q = 0; q < ntr; q++) t.trs3d[q] = tr_alloc<double>(t, (size_t)t.g.plane * cfg.kz);
      HIPCHK(hipMemcpy(t.trsout, t.trs3d.data(), sizeof(double*) * ntr, hipMemcpyHostToDevice));
    }
  }
  void tracer_slice() {
    if (!ntr) return;
    each([&](Tile& t) {
      const Geom& g = t.g;
      KLAUNCH(k_tr_slice, grid3(g.jce2 - g.jce1 + 1, g.ice2 - g.ice1 + 1, ntr * cfg.kz), BLK, 0, stream, g, cfg.kz, ntr,
              tr_args(t), t.rpsb, t.trsout);
    });
  }

  // Mass check of tend (Main/mod_massck.F90:190-306): the switch, the launches tend issues after
  // its prologue exchange, and the host's read of the log.  The log's capacity is a kernel
  // argument, so the captured graphs are dropped when it or the switch changes.
  static constexpr int MCK_HEAD = 8;     // doubles before the first record (the device counter)
  long long* mck_count() const { return reinterpret_cast<long long*>(mck_log); }
  void set_massck(int on, int cap) {
    if (on && (cap < 1 || cap > 65536))
      throw std::runtime_error("rcmdyn_set_massck: cap must be between 1 and 65536 records");
    quiesce();                                       // a lazy tend replays its graph first
    const bool b = on != 0;
    if (b == massck && (!b || cap == mck_cap)) return;   // the same switch: the log is kept
    invalidate_graphs();
    if (b) {
      if (!mck_part) {
        int off = 0;
        for (auto& t : tiles) {
          const Geom& g = t.g;
          const int line = std::max(g.ice2 - g.ice1 + 1, g.jci2 - g.jci1 + 1);
          const int nbchunk = std::max(1, (line + 255) / 256);
          MassckTile m{off, 4 * nbchunk * cfg.kz, (g.ici2 - g.ici1 + MCK_ROWS) / MCK_ROWS, nbchunk};
          off += 2 * m.nbdy + (hc.nqx * cfg.kz + 1) * m.nchunk;
          mck_lay.push_back(m);
        }
        HIPCHK(hipMalloc((void**)&mck_part, sizeof(double) * (size_t)off));
        HIPCHK(hipMemset(mck_part, 0, sizeof(double) * (size_t)off));
        HIPCHK(hipMalloc((void**)&mck_tab, sizeof(MassckTile) * mck_lay.size()));
        HIPCHK(hipMemcpy(mck_tab, mck_lay.data(), sizeof(MassckTile) * mck_lay.size(), hipMemcpyHostToDevice));
      }
      if (mck_log) { (void)hipFree(mck_log); mck_log = nullptr; }
      const size_t n = sizeof(double) * (MCK_HEAD + (size_t)cap * MCK_NREC);
      HIPCHK(hipMalloc((void**)&mck_log, n));
      HIPCHK(hipMemset(mck_log, 0, n));
      mck_cap = cap;
      mck_seen = 0;
    }
    massck = b;
  }
  // k_massck of every owned tile, then k_massck_final, on the engine's stream: after the exchange
  // that fills the ghost points the boundary lines read (u at i + 1, v at j + 1), before anything
  // of the step writes atm1 or p* of the current parity
  void massck_launch() {
    if (!massck) return;
    for (size_t q = 0; q < tiles.size(); q++) {
      Tile& t = tiles[q];
      const MassckTile& m = mck_lay[q];
      MassckArgs a{};
      a.u = fptr(t, FK::A1U); a.v = fptr(t, FK::A1V); a.psa = fptr(t, FK::PSA);
      a.qx[0] = fptr(t, FK::A1QV); a.qx[1] = fptr(t, FK::A1QC);
      for (int n = 0; n < hc.nsp; n++) a.qx[2 + n] = fptr(t, fkq(FK::A1QX0, n));
      a.nqx = hc.nqx;
      a.part = mck_part + m.off;
      a.nbdy = m.nbdy; a.nbchunk = m.nbchunk; a.nchunk = m.nchunk;
      KLAUNCH(k_massck, dim3(m.nbdy + (hc.nqx * cfg.kz + 1) * m.nchunk), BLK, 0, stream, t.g, dc, ds, a);
    }
    KLAUNCH(k_massck_final, dim3(1), dim3(256), 0, stream, dc, ds, mck_part, mck_tab, (int)tiles.size(), hc.nqx,
            mck_log + MCK_HEAD, mck_count(), mck_cap);
  }
  void get_massck(double* out, int cap, int32_t* count, int64_t* lost) {
    settle();
    if (!massck) throw std::runtime_error("rcmdyn_get_massck: the mass check is off (rcmdyn_set_massck)");
    if (cap < 0) throw std::runtime_error("rcmdyn_get_massck: cap must not be negative");
    HIPCHK(hipStreamSynchronize(stream));
    check_now();
    std::vector<double> ring(MCK_HEAD + (size_t)mck_cap * MCK_NREC);
    HIPCHK(hipMemcpy(ring.data(), mck_log, sizeof(double) * ring.size(), hipMemcpyDeviceToHost));
    long long now = 0;
    std::memcpy(&now, ring.data(), sizeof(now));
    const long long fresh = now - mck_seen;
    const int n = (int)std::min<long long>(fresh, std::min(cap, mck_cap));
    for (int q = 0; q < n; q++)            // the newest n records, oldest first
      std::memcpy(out + (size_t)q * MCK_NREC, ring.data() + MCK_HEAD + (size_t)((now - n + q) % mck_cap) * MCK_NREC,
                  sizeof(double) * MCK_NREC);
    if (n > 0 && comm && cfg.tile_count < ntiles) {   // sumall over the ranks: the four sums of every record
      double* d = nullptr;
      HIPCHK(hipMalloc(&d, sizeof(double) * 4 * (size_t)n));
      std::vector<double> hv(4 * (size_t)n);
      for (int q = 0; q < n; q++)
        for (int e = 0; e < 4; e++) hv[4 * (size_t)q + e] = out[(size_t)q * MCK_NREC + 2 + e];
      HIPCHK(hipMemcpy(d, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice));
      comm->allreduce_sum(d, hv.size(), stream);
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(hv.data(), d, sizeof(double) * hv.size(), hipMemcpyDeviceToHost));
      (void)hipFree(d);
      for (int q = 0; q < n; q++)
        for (int e = 0; e < 4; e++) out[(size_t)q * MCK_NREC + 2 + e] = hv[4 * (size_t)q + e];
    }
    mck_seen = now;
    *count = n;
    *lost = fresh - n;
  }

  // ------------------------------------------------------------------ halo exchange
  // Every exchange stages the owned edge boxes of its fields per neighbour direction
  // (0 L, 1 R, 2 B, 3 T, 4 BL, 5 BR, 6 TL, 7 TR) with k_pack_segs, moves each direction's
  // contiguous span to the peer (device copy for a tile on this GPU, RCCL for a remote one)
  // and unpacks the ghost boxes.  sides: 0 exchange, 1 exchange_lb, 2 exchange_rt.
  static constexpr int DJ[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
  static constexpr int DI[8] = {0, 0, -1, 1, -1, -1, 1, 1};
  static constexpr int OPP[8] = {1, 0, 3, 2, 7, 6, 5, 4};
  static bool recv_dir(int sides, int d) {
    if (sides == 0) return true;
    if (sides == 1) return d == 0 || d == 2 || d == 4;
    return d == 1 || d == 3 || d == 7;
  }
  int peer_of(const Tile& t, int d) const {
    int lj = t.lj + DJ[d];
    int li = t.li + DI[d];
    if (cfg.i_band) lj = (lj + cfg.nproc_j) % cfg.nproc_j;       // periodic in j (may be t itself)
    if (cfg.i_crm) li = (li + cfg.nproc_i) % cfg.nproc_i;        // CRM: periodic in i too
    return (lj >= 0 && lj < cfg.nproc_j && li >= 0 && li < cfg.nproc_i) ? lj * cfg.nproc_i + li : -1;
  }
  Tile* local_tile(int idx) {
    int o = idx - cfg.tile_first;
    return (o >= 0 && o < (int)tiles.size()) ? &tiles[o] : nullptr;
  }
  struct XField { FK f; int nk; int width = 0; int sides = -1; int n = 0; };  // 0/-1: the call's default; n: tracer
  // (j1,j2,i1,i2) of the box sent toward d (send) or received from d (recv)
  static void box(const Geom& g, int d, int w, bool send, int b[4]) {
    b[0] = g.jde1; b[1] = g.jde2; b[2] = g.ide1; b[3] = g.ide2;
    if (send) {
      if (DJ[d] < 0) b[1] = g.jde1 + w - 1;
      if (DJ[d] > 0) b[0] = g.jde2 - w + 1;
      if (DI[d] < 0) b[3] = g.ide1 + w - 1;
      if (DI[d] > 0) b[2] = g.ide2 - w + 1;
    } else {
      if (DJ[d] < 0) { b[0] = g.jde1 - w; b[1] = g.jde1 - 1; }
      if (DJ[d] > 0) { b[0] = g.jde2 + 1; b[1] = g.jde2 + w; }
      if (DI[d] < 0) { b[2] = g.ide1 - w; b[3] = g.ide1 - 1; }
      if (DI[d] > 0) { b[2] = g.ide2 + 1; b[3] = g.ide2 + w; }
    }
  }
  // segment builder: appends the segments of direction d (send or recv) for tile t
  using SegFn = std::function<void(Tile&, int, bool, std::vector<Seg>&)>;
  struct Layout {
    std::vector<Seg> segs;
    long start[8], count[8];
    uint64_t sig[8];       // shape signature of each direction's message (FNV-1a of nk, nj, ni)
  };
  Layout layout(Tile& t, const SegFn& fn, bool send, const std::function<bool(int)>& dir_on) {
    Layout L;
    long off = 0;
    for (int d = 0; d < 8; d++) {
      L.start[d] = off; L.count[d] = 0;
      uint64_t h = 1469598103934665603ull;
      auto mix = [&h](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
      if (peer_of(t, d) < 0 || !dir_on(d)) { L.sig[d] = 0; continue; }
      std::vector<Seg> v;
      fn(t, d, send, v);
      for (Seg& s : v) {
        s.off = off;
        off += (long)(s.j2 - s.j1 + 1) * (s.i2 - s.i1 + 1) * s.nk;
        mix((uint64_t)s.nk); mix((uint64_t)(s.j2 - s.j1 + 1)); mix((uint64_t)(s.i2 - s.i1 + 1));
        L.segs.push_back(s);
      }
      L.count[d] = off - L.start[d];
      L.sig[d] = h & 0x7fffffffffffffffull;
    }
    if (off > staging_cap) throw std::runtime_error("rcmdyn: halo staging buffer too small");
    return L;
  }
  void launch_segs(const std::vector<Seg>& segs, double* buf, int unpack) {
    for (size_t a = 0; a < segs.size(); a += MAXSEG) {
      SegList L{};
      L.n = (int)std::min<size_t>(MAXSEG, segs.size() - a);
      for (int q = 0; q < L.n; q++) L.s[q] = segs[a + q];
      KLAUNCH(k_pack_segs, dim3(32, L.n), dim3(256), 0, stream, L, buf, unpack);
    }
  }
  void exchange_generic(const SegFn& fn, const std::function<bool(int)>& send_on,
                        const std::function<bool(int)>& recv_on) {
    if (!halo) return;
    // staging of the stream this exchange is issued on (the two streams' exchanges overlap)
    auto SB = [&](Tile& x) { return on2 ? x.sbuf2 : x.sbuf; };
    auto RB = [&](Tile& x) { return on2 ? x.rbuf2 : x.rbuf; };
    std::vector<Layout> S, R;
    for (auto& t : tiles) {
      S.push_back(layout(t, fn, true, send_on));
      R.push_back(layout(t, fn, false, recv_on));
    }
    for (size_t q = 0; q < tiles.size(); q++) launch_segs(S[q].segs, SB(tiles[q]), 0);
    std::vector<Xfer> sends, recvs;
    for (size_t q = 0; q < tiles.size(); q++) {
      Tile& t = tiles[q];
      for (int d = 0; d < 8; d++) {
        const int p = peer_of(t, d);
        if (p < 0) continue;
        Tile* pt = local_tile(p);
        if (S[q].count[d] && pt && sw.force_rccl && comm) {
          // one-rank communicator: the n-th send to self matches the n-th receive
          const size_t pq = pt - tiles.data();
          if (R[pq].count[OPP[d]] != S[q].count[d]) throw std::runtime_error("rcmdyn: halo size mismatch");
          sends.push_back({comm->rank(), SB(t) + S[q].start[d], (size_t)S[q].count[d], S[q].sig[d]});
          recvs.push_back({comm->rank(), RB(*pt) + R[pq].start[OPP[d]], (size_t)S[q].count[d], R[pq].sig[OPP[d]]});
          continue;
        }
        if (S[q].count[d] && pt) {
          const size_t pq = pt - tiles.data();
          if (R[pq].count[OPP[d]] != S[q].count[d]) throw std::runtime_error("rcmdyn: halo size mismatch");
          DHIPCHK(hipMemcpyAsync(RB(*pt) + R[pq].start[OPP[d]], SB(t) + S[q].start[d],
                                 S[q].count[d] * sizeof(double), hipMemcpyDeviceToDevice, stream));
        }
        if (R[q].count[d] && !pt) recvs.push_back({p, RB(t) + R[q].start[d], (size_t)R[q].count[d], R[q].sig[d]});
      }
      // remote sends in the order of the receiver's directions: the n-th message between two
      // ranks matches the n-th receive, and in a band of two tiles in j one peer is both the
      // left and the right neighbour
      for (int e = 0; e < 8; e++) {
        const int d = OPP[e], p = peer_of(t, d);
        if (p < 0 || !S[q].count[d] || local_tile(p)) continue;
        sends.push_back({p, SB(t) + S[q].start[d], (size_t)S[q].count[d], S[q].sig[d]});
      }
    }
    if (!sends.empty() || !recvs.empty()) {
      if (!comm) throw std::runtime_error("rcmdyn: remote neighbour without a communicator");
      comm->sendrecv(sends, recvs, stream, on2 ? 1 : 0);
    }
    for (size_t q = 0; q < tiles.size(); q++) launch_segs(R[q].segs, RB(tiles[q]), 1);
  }

  Seg field_seg(Tile& t, double* p, int nk, int d, int w, bool send) {
    int b[4];
    box(t.g, d, w, send, b);
    Seg s{};
    s.p = p; s.kstride = t.g.plane; s.pitch = t.g.pitch; s.j0 = t.g.j0; s.i0 = t.g.i0;
    s.j1 = b[0]; s.j2 = b[1]; s.i1 = b[2]; s.i2 = b[3]; s.nk = nk;
    return s;
  }

  // exchange / exchange_lb / exchange_rt of several fields at once
  // One exchange point: every field travels in the same per-neighbour message, each with its
  // own width and sides (0 exchange, 1 exchange_lb, 2 exchange_rt).
  void xch(std::initializer_list<XField> fields, int width = 1, int sides = 0) {
    xchv(std::vector<XField>(fields), width, sides);
  }
  void xchv(std::vector<XField> fs, int width = 1, int sides = 0) {
    if (!halo) return;
    for (XField& x : fs) {
      if (x.width == 0) x.width = width;
      if (x.sides < 0) x.sides = sides;
    }
    auto fn = [&](Tile& t, int d, bool send, std::vector<Seg>& v) {
      for (const XField& x : fs)
        if (recv_dir(x.sides, send ? OPP[d] : d)) v.push_back(field_seg(t, fptr(t, x.f, x.n), x.nk, d, x.width, send));
    };
    auto all = [](int) { return true; };
    exchange_generic(fn, all, all);
  }

  // Halo/compute overlap (north star): issue an exchange point on the second
  // stream, forked from the first at this point of the step; the first stream goes on with
  // kernels that do not read these fields' ghost rings and waits for it in xch_join.  Both
  // streams' RCCL calls go to one communicator in the same order on every rank; captured
  // into the step graph as a fork/join.
  void fork_point() {
    if (!halo) return;
    DHIPCHK(hipEventRecord(evfork, stream));
  }
  // one communicator for both streams (RCMDYN_RCCL_CHAN2=one): the second stream's exchange
  // forks after the first stream's preceding exchange instead, so the two grouped calls are
  // never in flight together; the overlap with the kernels that follow stays
  void fork_after_exchange() {
    if (comm && comm->shared_channels()) fork_point();
  }
  void xch_begin(std::vector<XField> fs, int slot = 0) {
    if (!halo) return;
    DHIPCHK(hipStreamWaitEvent(stream2, evfork, 0));
    std::swap(stream, stream2);
    on2 = true;
    try {
      xchv(std::move(fs));
    } catch (...) {
      on2 = false;
      std::swap(stream, stream2);
      throw;
    }
    on2 = false;
    std::swap(stream, stream2);
    DHIPCHK(hipEventRecord(evjoin[slot], stream2));
    join_pending[slot] = true;
  }
  void xch_join(int slot = 0) {
    if (!join_pending[slot]) return;
    DHIPCHK(hipStreamWaitEvent(stream, evjoin[slot], 0));
    join_pending[slot] = false;
  }
  // The round-3 overlap form: every exchange stays on the engine's stream (RCCL calls are
  // captured on the capture's origin stream only; the RCCL 2.26 that torch bundles crashed a
  // captured step whose first exchange ran on the forked stream), and the kernels that read no
  // point of it run on the second stream: side_begin forks the second stream from the engine's
  // at this point and sends the following launches there, side_end records their completion
  // (slot) and sends launches back, side_join makes the engine's stream wait for them.
  void side_begin() {
    if (!halo) return;
    DHIPCHK(hipEventRecord(evfork, stream));
    DHIPCHK(hipStreamWaitEvent(stream2, evfork, 0));
    std::swap(stream, stream2);
  }
  void side_end(int slot) {
    if (!halo) return;
    DHIPCHK(hipEventRecord(evjoin[slot], stream));
    std::swap(stream, stream2);
    join_pending[slot] = true;
  }
  void side_join(int slot) { xch_join(slot); }

  // exchange_lb of xdelh = delh(:,:,l,src) (Main/mod_split.F90:498-499)
  void xch_delh_slot(int l, int src) {
    if (!halo) return;
    const long off = ((long)(src - 1) * cfg.nsplit + (l - 1));
    auto fn = [&](Tile& t, int d, bool send, std::vector<Seg>& v) {
      v.push_back(field_seg(t, t.delh + off * t.g.plane, 1, d, 1, send));
    };
    exchange_generic(fn, [&](int d) { return recv_dir(1, OPP[d]); }, [&](int d) { return recv_dir(1, d); });
  }

  // width-w exchange of 2-D planes held in the tiles' wide frames (fused split step)
  void xch_wide(std::initializer_list<std::pair<double* Tile::*, int>> fields, int w) {
    if (!halo) return;
    std::vector<std::pair<double* Tile::*, int>> fs(fields);
    auto fn = [&](Tile& t, int d, bool send, std::vector<Seg>& v) {
      int b[4];
      box(t.gw, d, w, send, b);
      for (auto& x : fs) {
        Seg sg{};
        sg.p = t.*(x.first); sg.kstride = t.gw.plane; sg.pitch = t.gw.pitch; sg.j0 = t.gw.j0; sg.i0 = t.gw.i0;
        sg.j1 = b[0]; sg.j2 = b[1]; sg.i1 = b[2]; sg.i2 = b[3]; sg.nk = x.second;
        v.push_back(sg);
      }
    };
    auto all = [](int) { return true; };
    exchange_generic(fn, all, all);
  }
  // the fused split step is exact on a decomposition when every tile is at least SPX wide
  // (its depth-SPX halo then comes from the direct neighbours only)
  bool wide_ok() const {
    if (!halo) return true;
    for (const Geom& g : all)
      if (g.jde2 - g.jde1 + 1 < SPX || g.ide2 - g.ide1 + 1 < SPX) return false;
    return true;
  }
  // The decomposed hydrostatic step runs without the post-prologue exchanges when the fused
  // split step applies (every tile at least SPX wide, every mode within SPH sub-steps): its
  // kernels then compute the ghost rings their consumers read.
  bool split_fused() const {
    bool f = wide_ok();
    for (int l = 1; l <= cfg.nsplit; l++) f = f && ((int)hc.aam[l - 1] * 2 <= SPH);
    return f;
  }
  void copy_wide(Tile& t, const double* src, double* dst, int nplanes) {
    KLAUNCH(k_copy_frame, grid3(t.g.jde2 - t.g.jde1 + 1, t.g.ide2 - t.g.ide1 + 1, 1), BLK, 0, stream, t.g, t.gw,
            nplanes, src, (long)t.g.plane, dst, (long)t.gw.plane);
  }

  // exchange_bdy_lr / exchange_bdy_bt of the bdyuv slices (Main/mod_bdycod.F90:1063-1089):
  // south/north slices (by j) with the left/right tiles, west/east slices (by i) with the
  // bottom/top tiles; width 1, every level.
  void xch_slices() {
    if (!halo) return;
    const int kz = cfg.kz;
    auto fn = [&](Tile& t, int d, bool send, std::vector<Seg>& v) {
      const Geom& g = t.g;
      std::vector<int> ids;
      int lo, hi, origin;
      if (d == 0 || d == 1) {
        if (g.bt) ids.insert(ids.end(), {10, 11, 14, 15});
        if (g.bb) ids.insert(ids.end(), {8, 9, 12, 13});
        lo = g.jde1; hi = g.jde2; origin = g.j0;
      } else {
        if (g.bl) ids.insert(ids.end(), {0, 1, 4, 5});
        if (g.br) ids.insert(ids.end(), {2, 3, 6, 7});
        lo = g.ide1; hi = g.ide2; origin = g.i0;
      }
      const bool low = (d == 0 || d == 2);
      const int x = send ? (low ? lo : hi) : (low ? lo - 1 : hi + 1);
      for (int s : ids) {
        Seg sg{};
        sg.p = t.sl[s]; sg.kstride = slen; sg.pitch = 0; sg.j0 = origin; sg.i0 = 0;
        sg.j1 = x; sg.j2 = x; sg.i1 = 0; sg.i2 = 0; sg.nk = kz;
        v.push_back(sg);
      }
    };
    auto on = [&](int d) { return d < 4; };
    exchange_generic(fn, on, on);
  }

  // the acoustic update forms dprddx / dprddy from atm0%pr as the reference
  // defines them (Main/mod_params.F90:2676-2686); values a host put must be exactly those, or
  // the engine would silently compute with others
  void check_dprd() {
    if (cfg.idynamic != 2 || dry) { dprd_put = false; return; }
    int* bad = nullptr;
    HIPCHK(hipMalloc(&bad, sizeof(int)));
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(int), stream));
    for (auto& t : tiles) {
      const Geom& g = t.g;
      KLAUNCH(k_nh_check_dprd, grid3(g.jdi2 - g.jdi1 + 1, g.idi2 - g.idi1 + 1, cfg.kz), BLK, 0, stream, g,
              nhf[&t - tiles.data()], bad);
    }
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipFree(bad));
    // a mismatch stays pending: every later call fails the same way until a put corrects it
    if (n) throw std::runtime_error("rcmdyn: DPRDDX/DPRDDY differ from atm0%pr's four-point differences at " +
                                    std::to_string(n) + " points (Main/mod_params.F90:2676-2686)");
    dprd_put = false;
  }

  // ------------------------------------------------------------------ the step
  template <class F>
  void each(F fn) { for (auto& t : tiles) fn(t); }

  void prepare() {
    if (statics_dirty) {
      xch({{FK::MSFX, 1}, {FK::MSFD, 1}, {FK::HT, 1}, {FK::CORIOL, 1}}, 2, 0);
      each([&](Tile& t) {
        KLAUNCH(k_prepare_static, grid3(t.g.nj, t.g.ni, 1), BLK, 0, stream, t.g, dc, cfg.diffu_hgtf,
                t.msfx, t.msfd, t.ht, t.xmsf, t.dmsf, t.hgfact, t.mapf);
      });
      if (halo) {
        each([&](Tile& t) {
          copy_wide(t, t.msfx, t.wmsfx, 1);
          copy_wide(t, t.msfd, t.wmsfd, 1);
          copy_wide(t, t.mapf, t.wmapf, 1);
        });
        xch_wide({{&Tile::wmsfx, 1}, {&Tile::wmsfd, 1}, {&Tile::wmapf, 1}}, SPX);
      }
      statics_dirty = false;
      invalidate_graphs();
    }
    if (dprd_put) check_dprd();
    if (bdy_dirty) {
      const int kz = cfg.kz;
      // width 2: the ghost-ring kernels relax at ghost points (stencil radius 1)
      xch({{FK::UB0, kz}, {FK::UBT, kz}, {FK::VB0, kz}, {FK::VBT, kz}}, 2, 0);
      xch({{FK::TB0, kz}, {FK::TBT, kz}, {FK::QB0, kz}, {FK::QBT, kz}, {FK::PB0, 1}, {FK::PBT, 1}}, 2, 0);
      bdy_dirty = false;
      invalidate_graphs();
    }
    if (tr_bdy_dirty) {
      // chib0 / chibt as the b0 / bt of the other families: the relaxation reads them one point
      // out of the ghost-ring points it runs at
      std::vector<XField> v;
      add_tr(v, FK::TRB0, cfg.kz, 2);
      add_tr(v, FK::TRBT, cfg.kz, 2);
      for (size_t a = 0; a < v.size(); a += 8) xchv(std::vector<XField>(v.begin() + a, v.begin() + std::min(v.size(), a + 8)));
      tr_bdy_dirty = false;
    }
    if (kpbl_dirty) {
      // the physics puts kpbl on its own points (a rank puts its interior); vadv4d ind = 3 of
      // the fused hydrostatic step reads it on the ghost ring k_scalars computes in place of
      // the cqv/cqc exchange (Main/mod_advection.F90:898-925)
      xch({{FK::KPBL, 1}}, 1, 0);
      kpbl_dirty = false;
    }
  }

  // R of a tile: the column-box points whose k_columns work reads no ghost point toward a
  // neighbour (atm1 at j+1 / i+1, p* at +-1, psdot's j-1 / i-1), i.e. the owned points one in
  // from every side that has a neighbour; and the k_momentum / k_scalars blocks whose staged
  // halo-2 tile lies in R (their part-1 blocks, the same test as part_skip)
  void setup_overlap(Tile& t) {
    const Geom& g = t.g;
    t.rja = g.bl ? g.jdx1() : g.jde1 + 1;
    t.rjb = g.br ? g.jdx2() : g.jde2 - 1;
    t.ria = g.bb ? g.idx1() : g.ide1 + 1;
    t.rib = g.bt ? g.idx2() : g.ide2 - 1;
    if (t.rja > t.rjb || t.ria > t.rib) return;
    const long box = (long)(g.jdx2() - g.jdx1() + 1) * (g.idx2() - g.idx1() + 1);
    const long rin = (long)(t.rjb - t.rja + 1) * (t.rib - t.ria + 1);
    t.rnxb = (t.rjb - t.rja + COLW) / COLW;
    t.nint = t.rnxb * (t.rib - t.ria + 1);
    t.nring = (int)((box - rin + COLW - 1) / COLW);
    t.nred = t.nint + t.nring;
    auto inner = [&](int J0, int I0, int bj, int bi) {
      return J0 - 2 >= t.rja && J0 + bj + 1 <= t.rjb && I0 - 2 >= t.ria && I0 + bi + 1 <= t.rib;
    };
    // the block columns of k_momentum / k_scalars start at j1 or, shifted back by 64 - s, at
    // j1 + s - 64 (a partial first column): the origin that puts the most points of the tile in
    // blocks wholly inside R (on a 96-wide tile no default-aligned 64-wide block with its halo
    // fits, and part 1 would be empty)
    const int mj2 = g.br ? g.jdi2 : g.jde2 + 1, mi2 = g.bt ? g.idi2 : g.ide2 + 1;
    auto best = [&](int j1, int j2, int i1, int i2, int BJ, int BI, int& org, long& npts) {
      long top = 0;
      org = j1;
      for (int sft = 0; sft < BJ; sft++) {
        const int o = sft ? j1 + sft - BJ : j1;
        long pts = 0;
        for (int I0 = i1; I0 <= i2; I0 += BI)
          for (int J0 = o; J0 <= j2; J0 += BJ)
            if (inner(J0, I0, BJ, BI))
              pts += (long)(std::min(J0 + BJ - 1, j2) - std::max(J0, j1) + 1) * (std::min(I0 + BI - 1, i2) - I0 + 1);
        if (pts > top) { top = pts; org = o; }
      }
      npts = top;
      return top > 0;
    };
    t.mom_in = best(g.jdi1, mj2, g.idi1, mi2, MBJ, MBI, t.mj0, t.mom_p1);
    t.sca_in = best(g.jcx1(), g.jcx2(), g.icx1(), g.icx2(), SBJ, SBI, t.sj0, t.sca_p1);
  }
  Fields fields(Tile& t, int part) {
    Fields f = fields(t);
    f.pt = Part{part, t.rja, t.rjb, t.ria, t.rib, t.rnxb, t.nint, t.mj0, t.sj0};
    return f;
  }

  // the instance of k_momentum / k_scalars / k_update a launch with the argument
  // block f takes (optset.hpp): from the configuration and the pointers the launch passes
  OptInstance opt_instance(const Fields& f) const {
    OptQuery q{};
    q.iboudy = cfg.iboudy; q.idiffu = cfg.idiffu; q.ipgf = cfg.ipgf; q.isladvec = cfg.isladvec;
    q.ibltyp = cfg.ibltyp; q.iuwvadv = cfg.iuwvadv; q.nqx_extra = hc.nsp;
    q.budget = budget; q.no_optset = sw.no_optset; q.condtq = condtq;
    q.tten = f.tten; q.uten = f.uten; q.vten = f.vten; q.qvten = f.qvten; q.qcten = f.qcten;
    q.omega = f.omega; q.xkcs = f.xkcs;
    q.tphy = f.tphy; q.qvphy = f.qvphy; q.qcphy = f.qcphy; q.uphy = f.uphy; q.vphy = f.vphy;
    q.kpbl = f.kpbl;
    return optset_instance(q);
  }

  // dynamic LDS of the two-phase column kernels: 4 x kz x 64 doubles
  size_t col_lds() const { return sizeof(double) * 4 * COLW * (size_t)cfg.kz; }

  // all buffers of one tile for its current parity (see Fields)
  Fields fields(Tile& t) {
    const int c = t.cur, n = 1 - c, q = thp(t), o = 1 - q;
    Fields f{};
    f.a1u = t.a1u[c]; f.a1v = t.a1v[c]; f.a1t = t.a1t[q]; f.a1qv = t.a1qv[q]; f.a1qc = t.a1qc[q];
    f.a2u = t.a2u[c]; f.a2v = t.a2v[c]; f.a2t = t.a2t[q]; f.a2qv = t.a2qv[q]; f.a2qc = t.a2qc[q];
    f.psa = t.psa_[c]; f.psb = t.psb_[c];
    f.b1u = t.a1u[n]; f.b1v = t.a1v[n]; f.b1t = t.a1t[o]; f.b1qv = t.a1qv[o]; f.b1qc = t.a1qc[o];
    f.b2u = t.a2u[n]; f.b2v = t.a2v[n]; f.b2t = t.a2t[o]; f.b2qv = t.a2qv[o]; f.b2qc = t.a2qc[o];
    f.bpsa = t.psa_[n]; f.bpsb = t.psb_[n];
    f.msfx = t.msfx; f.msfd = t.msfd; f.coriol = t.coriol; f.ht = t.ht; f.xmsf = t.xmsf; f.dmsf = t.dmsf;
    f.hgfact = t.hgfact; f.mapf = t.mapf;
    f.rgcr = t.rgcr; f.rgdt = t.rgdt; f.ibcr = t.ibcr; f.ibdt = t.ibdt;
    f.ub0 = t.ub0; f.ubt = t.ubt; f.vb0 = t.vb0; f.vbt = t.vbt; f.tb0 = t.tb0; f.tbt = t.tbt;
    f.qb0 = t.qb0; f.qbt = t.qbt; f.pb0 = t.pb0; f.pbt = t.pbt;
    f.rpsa = t.rpsa; f.rpsb = t.rpsb; f.rpsda = t.rpsda; f.rpsdb = t.rpsdb; f.psc = t.psc;
    f.psdota = t.psdota; f.psdotb = t.psdotb; f.pten = t.pten; f.ptenn = t.pten + t.g.plane;
    f.qdot = t.qdot; f.phi = t.phi; f.slqv = t.slqv; f.slqc = t.slqc; f.cqv = t.cqv; f.cqc = t.cqc; f.fqv = t.fqv; f.fqc = t.fqc;
    f.d6u = t.d6[0]; f.d6v = t.d6[1]; f.d6t = t.d6[2]; f.d6qv = t.d6[3]; f.d6qc = t.d6[4];
    f.depplane = t.depplane;
    if (diag) {
      f.tten = t.tten; f.uten = t.uten; f.vten = t.vten; f.qvten = t.qvten; f.qcten = t.qcten;
      f.omega = t.omega; f.xkcs = t.xkcs;
    }
    if (cfg.ibltyp == 2) f.xkcs = t.xkcs;     // the TKE diffusion reads xkcf from it
    if (hc.iqxvadv == 3) f.kpbl = t.kpbl;    // vadv4d ind = 3 of qc
    f.tphy = phy_tqc(t, 0); f.qvphy = phy_tqc(t, 1); f.qcphy = phy_tqc(t, 2); f.uphy = t.phy[3]; f.vphy = t.phy[4];
    f.red = red; f.red_off = t.red_off;
    f.qfuse = qfuse() ? 1 : 0; f.negcnt = t.negcnt; f.neglist = t.neglist;
    for (int n = 0; n < hc.nsp; n++) f.qxa1[n] = t.a1qx[n][c];
    if (hc.nsp || ntr) f.xkcs = t.xkcs;       // k_qx_tend's diffusion reads the scaled xkc (the tracers' too)
    return f;
  }

  // the hydrometeors beyond qc (nqx = 5) for the current parity: a* current, b* next (the
  // hydrostatic ping-pong; the NH core updates a* in place)
  QxArgs qx_args(Tile& t, int par = -1) {
    const int c = par < 0 ? t.cur : par, n1 = 1 - c;
    QxArgs q{};
    q.nsp = hc.nsp;
    for (int n = 0; n < hc.nsp; n++) {
      q.a1[n] = t.a1qx[n][c]; q.a2[n] = t.a2qx[n][c];
      const bool nh = cfg.idynamic == 2;
      q.b1[n] = t.a1qx[n][nh ? c : n1]; q.b2[n] = t.a2qx[n][nh ? c : n1];
      q.cq[n] = t.cqx[n]; q.fq[n] = t.fqx[n]; q.sl[n] = t.slqx[n]; q.d6[n] = t.d6qx[n]; q.phy[n] = t.phyx[n];
    }
    q.dep = t.depx;
    q.depf = t.depxf;
    return q;
  }
  // the XField entries of the hydrometeors beyond qc for one kind (A1QX0 ..), width w
  void add_qx(std::vector<XField>& v, FK base, int nk, int w) const {
    for (int n = 0; n < hc.nsp; n++) v.push_back({fkq(base, n), nk, w});
  }
  // the same of the declared tracers (TRA1 ..): they join the species' grouped exchanges
  void add_tr(std::vector<XField>& v, FK kind, int nk, int w) const {
    for (int n = 0; n < ntr; n++) v.push_back({kind, nk, w, -1, n});
  }

  // istep of sound (Main/mod_sound.F90:201-205) for the host time mirror
  int nh_istep() const {
    int istep = (int)(hs.dt / cfg.nh_dtsmax);
    if (istep < 2) istep = 2;
    if (hs.lcount > 0 && istep < 4) istep = 4;
    return istep;
  }
  // alarm_day (Main/mpplib/mod_timer.F90:277-337): active at the start and at the first step
  // whose start time reaches the next multiple of a day
  bool nh_day_alarm() const { return nh_day_alarm_at(hs.lcount); }
  bool nh_day_alarm_at(long long lc) const {
    const double tnow = (double)lc * cfg.dtsec;
    return lc == 0 || !nh_tmask_valid ||
           std::floor(tnow / 86400.0) != std::floor((tnow - cfg.dtsec) / 86400.0);
  }
  bool nh_tmask_valid = false;

  // tend, non-hydrostatic (Main/mod_tendency.F90:212-616 with idynamic = 2).  Exchange points
  // follow the reference's exchange calls: decouple (atm1 width 1, atm2 width idif, pp, w),
  // compute_omega (cr, qdot), calc_coeff (xkc), the moisture forecast (atmc%qx), and per
  // acoustic sub-step dp'/dp0 with pp, then u and v (Main/mod_sound.F90:262-263, 294-295);
  // the upper radiative condition's estore gather (:496-497) becomes a 6-deep halo.
  void nh_tend(int phase, bool slice) {
    const int kz = cfg.kz, kp = kz + 1;
    const int istep = nh_istep();
    const bool alarm = nh_day_alarm();
    // halo/compute overlap of a whole tend on a decomposed domain: the cr/qdot/xkcr exchange
    // on the second stream beside k_nh_tend_c (which reads them at its own point only), the
    // cqv/cqc exchange beside k_nh_tend_d (which does not read them)
    const bool ovl = halo && !sw.no_overlap && phase == TEND_ALL && !slice && cfg.isladvec != 1;
    struct Grids { dim3 fr, ce1, ci1; };
    auto grids = [&](const Geom& g) {
      const int nce_j = g.jce2 - g.jce1 + 1, nce_i = g.ice2 - g.ice1 + 1;
      const int nci_j = g.jci2 - g.jci1 + 1, nci_i = g.ici2 - g.ici1 + 1;
      return Grids{grid3(g.nj, g.ni, kp), grid3(nce_j, nce_i, 1), grid3(nci_j, nci_i, 1)};
    };
    if (phase & TEND_PRE) {
    // isladvec = 1: k_sladv forms ud*msfd two points out (the reference exchanges atmx%ud 2
    // wide, :995-997) and interpolates atm2 qx up to three points out (max(idif, 4), :1073-1075)
    // idiffu = 3: atm2 idif = 3 wide, p*b 4 wide (p*dotb on k_nh_diffu6's 3-deep dot rings)
    const int wd = cfg.idiffu == 3 ? 3 : 2;
    const int wu = cfg.isladvec == 1 ? 2 : 1, wq = std::max(cfg.isladvec == 1 ? 3 : 2, wd);
    // atm2 on the second stream, overlapped with decouple and compute_omega (atm1 only)
    std::vector<XField> pro{{FK::PSA, 1, 3}, {FK::PSB, 1, wd + 1}, {FK::A1U, kz, wu}, {FK::A1V, kz, wu}, {FK::A1T, kz},
                            {FK::A1QV, kz}, {FK::A1QC, kz}, {FK::A1PP, kz}, {FK::A1W, kp}};
    std::vector<XField> pro2{{FK::A2U, kz, wd}, {FK::A2V, kz, wd}, {FK::A2T, kz, wd}, {FK::A2QV, kz, wq},
                             {FK::A2QC, kz, wq}, {FK::A2PP, kz, wd}, {FK::A2W, kp, wd}};
    if (cfg.ibltyp == 2) { pro.push_back({FK::A1TKE, kp, 1}); pro2.push_back({FK::A2TKE, kp, wd}); }
    add_qx(pro, FK::A1QX0, kz, 1);
    add_qx(pro2, FK::A2QX0, kz, wq);
    add_tr(pro, FK::TRA1, kz, 1);         // Main/mod_tendency.F90:874, 1087-1089
    add_tr(pro2, FK::TRA2, kz, wq);
    fork_point();
    xchv(pro);
    fork_after_exchange();
    xch_begin(pro2);
    massck_launch();
    each([&](Tile& t) {
      const Geom& g = t.g;
      const NHFields f = nhfields(t);
      const Grids q = grids(g);
      KLAUNCH(k_surface_pressures, grid3(g.nj, g.ni, 1), BLK, 0, stream, g, fields(t));
      KLAUNCH(k_nh_decouple, q.fr, BLK, 0, stream, g, dc, f);
      KLAUNCH(k_nh_omega, q.ce1, BLK, 0, stream, g, dc, f);
    });
    xch_join();
    if (cfg.idiffu == 3)       // the tendency kernels compute owned points only: no exchange
      each([&](Tile& t) {
        const Geom& g = t.g;
        KLAUNCH(k_nh_diffu6, dim3((g.ide2 - g.ide1 + 64) / 64, kp, 6 + hc.nsp), dim3(64), 0, stream, g, dc,
                nhfields(t), qx_args(t));
      });
    each([&](Tile& t) {
      const Geom& g = t.g;
      const NHFields f = nhfields(t);
      const Grids q = grids(g);
      KLAUNCH(k_nh_coeff_raw, q.ce1, BLK, 0, stream, g, dc, f);
    });
    // ovl: the exchange is issued in TEND_POST, after k_nh_tend_c went to the second stream
    if (!ovl) xch({{FK::NCR, kz}, {FK::QDOT, kp}, {FK::NXKCR, kz}});
    if (slice) run_slice();
    }
    subex_mid(phase);
    if (!(phase & TEND_POST)) return;
    each([&](Tile& t) {
      const Geom& g = t.g;
      const NHFields f = nhfields(t);
      // init_tendencies (:1227-1240): the zero is the leading summand of each tendency's first
      // writer (k_nh_uv_adv, k_nh_scalar_adv, the iboudy = 4 sponges, k_nh_forecast), which
      // covers every point a later kernel reads.  With diagnostics on, the total tendencies
      // are also zeroed, so a get shows 0 at the points no kernel writes.
      if (diag) {
        const size_t b3 = sizeof(double) * g.plane * kz, b4 = sizeof(double) * g.plane * kp;
        for (double* p : {f.tten, f.qvten, f.qcten, f.uten, f.vten, f.ppten}) HIPCHK(hipMemsetAsync(p, 0, b3, stream));
        HIPCHK(hipMemsetAsync(f.wten, 0, b4, stream));
      }
      if (cfg.isladvec == 1)
        KLAUNCH(k_sladv, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, kz), BLK, 0, stream, g, dc, ds, fields(t),
                qx_args(t));
      // the tendency chains (advection, curvature/adiabatic, boundary, diffusion, forecast)
      if (!ovl) {
        tend_d_launch(t, f, istep);
        tend_c_launch(t, f, istep);
      }
    });
    if (ovl) {
      // second stream: k_nh_tend_c, then (after the cr/qdot/xkcr exchange) k_nh_tend_d; the
      // engine's stream: that exchange, then (after k_nh_tend_c) the cqv/cqc exchange
      side_begin();
      each([&](Tile& t) { tend_c_launch(t, nhfields(t), istep); });
      side_end(0);
      xch({{FK::NCR, kz}, {FK::QDOT, kp}, {FK::NXKCR, kz}});
      side_begin();
      each([&](Tile& t) { tend_d_launch(t, nhfields(t), istep); });
      side_end(1);
      side_join(0);
      xchv(cq_fields());
      side_join(1);
      tke_step();
    } else {
      tke_step();
      xchv(cq_fields());
    }
    each([&](Tile& t) {
      const Geom& g = t.g;
      const NHFields f = nhfields(t);
      const Grids q = grids(g);
      if (hc.nsp) {
        // the hydrometeors beyond qc: their fix and RAW filter in place (they feed nothing
        // else of the step; k_nh_tend_c read atm1 for the water load before)
        KLAUNCH_AS("k_qx_fix", k_qx_fix<FamQx>, grid3(g.jdx2() - g.jdx1() + 1, g.idx2() - g.idx1() + 1, kz), BLK, 0,
                   stream, g, dc, qx_args(t));      // the column box, as the hydrostatic launch: its jci x ici fix
        KLAUNCH_AS("k_qx_serial", k_qx_serial<FamQx>, dim3(hc.nsp * kz), dim3(negfix_threads(g)),
                   sizeof(double) * negfix_lds(g), stream, g, dc, qx_args(t));
        KLAUNCH_AS("k_qx_post", k_qx_post<FamQx>, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, hc.nsp * kz), BLK, 0,
                   stream, g, dc, qx_args(t));
      }
      if (ntr) tracer_fix(t);        // the tracers likewise, in place
      KLAUNCH(k_nh_negfix, dim3(1024), dim3(256), 0, stream, g, dc, f);
      KLAUNCH(k_nh_negfix_serial, dim3(2 * kz), dim3(negfix_threads(g)), sizeof(double) * negfix_lds(g), stream, g, dc, f);
      // tend's time filters (tfuse = 0) with part A of the first acoustic sub-step (sound, :163-718)
      if (sw.nh_tfuse)     // part A alone: one column walk per cross column
        KLAUNCH(k_nh_a1_col, q.ce1, BLK, 0, stream, g, dc, f);
      else
        KLAUNCH(k_nh_tfilter_a1, grid3(g.jce2 - g.jce1 + 1, g.ice2 - g.ice1 + 1, kp), BLK, 0, stream, g, dc, f);
    });
    if (sw.nh_tfuse) for (auto& t : tiles) t.tq = 1 - t.tq;     // the filtered t, qv, qc
    // sound, Main/mod_sound.F90:163-718
    for (int it = 1; it <= istep; it++) {
      // part A: sub-step 1 in k_nh_tfilter_a1, the later ones in the previous k_nh_sound_cd
      // the dp'/dp0, pp exchange beside part 1 of k_nh_sound_uv (the points that read no ghost),
      // then the strip of the others
      auto sound_uv = [&](Tile& t, int part) {
        const Geom& g = t.g;
        const int fin = (int)(it == istep), first = (int)(it == 1);
        if (part == 2) {
          const int n = (g.bl ? 0 : g.ide2 - g.ide1 + 1) + (g.bb ? 0 : g.jde2 - g.jde1 + (g.bl ? 0 : 1));
          if (n > 0)
            KLAUNCH(k_nh_sound_uv, dim3((n + 127) / 128, kz), dim3(128), 0, stream, g, dc, ds, nhfields(t), istep,
                    fin, first, 2);
          return;
        }
        KLAUNCH(k_nh_sound_uv, grid3(g.jde2 - g.jde1 + 1, g.ide2 - g.ide1 + 1, kz),
                BLK, 0, stream, g, dc, ds, nhfields(t), istep, fin, first, part);
      };
      if (halo && !sw.no_overlap) {
        side_begin();
        each([&](Tile& t) { sound_uv(t, 1); });
        side_end(0);
        xch({{FK::NCDT, kz}, {FK::NCPP, kz}});
        side_join(0);
        each([&](Tile& t) { sound_uv(t, 2); });
      } else {
        xch({{FK::NCDT, kz}, {FK::NCPP, kz}});
        each([&](Tile& t) { sound_uv(t, 0); });
      }
      xch({{FK::NCU, kz}, {FK::NCV, kz}});
      each([&](Tile& t) {
        const Geom& g = t.g;
        const NHFields f = nhfields(t);
        const Grids q = grids(g);
        KLAUNCH(k_nh_sound_bc, q.ci1, BLK, 0, stream, g, dc, ds, f, istep, it);
      });
      if (cfg.ifupr == 1) {
        if (it == 1 && alarm) {
          each([&](Tile& t) {
            KLAUNCH(k_nh_tmask_gather, grids(t.g).ci1, BLK, 0, stream, t.g, dc, nhfields(t), nh_gbuf);
          });
          if (comm) comm->allreduce_sum(nh_gbuf, 2 * (size_t)cfg.jx * cfg.iy, stream);
          KLAUNCH(k_nh_tmask, dim3(1), dim3(256), 0, stream, tiles[0].g, dc, nh_gbuf, nhf[0].tmask);
          nh_tmask_valid = true;
        }
        if (halo) {
          each([&](Tile& t) { copy_wide(t, nhf[&t - tiles.data()].estore, t.westore, 1); });
          xch_wide({{&Tile::westore, 1}}, 6);
        }
      }
      each([&](Tile& t) {
        const Geom& g = t.g;
        const NHFields f = nhfields(t);
        const Grids q = grids(g);
        if (halo)
          KLAUNCH(k_nh_sound_cd, q.ci1, BLK, 0, stream, g, t.gw, t.westore, dc, ds, f, istep, (int)(it == istep),
                  (int)(it < istep));
        else
          KLAUNCH(k_nh_sound_cd, q.ci1, BLK, 0, stream, g, g, f.estore, dc, ds, f, istep, (int)(it == istep),
                  (int)(it < istep));
      });
    }
    each([&](Tile& t) {
      KLAUNCH(k_nh_sound_final, dim3((nh_frame_ring(t.g) + 255) / 256, kz + 1), dim3(256), 0, stream, t.g, dc,
              nhfields(t));
    });
    KLAUNCH(k_nh_advance, dim3(1), dim3(256), 0, stream, dc, ds, nhf[0]);
    hs.lcount += 1;
    if (hs.lcount == 2) hs.dt = 2.0 * cfg.dtsec;
  }

  void tend_d_launch(Tile& t, const NHFields& f, int istep) {
    const Geom& g = t.g;
    const dim3 gd((g.jdi2 - g.jdi1 + 64) / 64, (g.idi2 - g.idi1 + TD_I) / TD_I, cfg.kz);
    KLAUNCH(k_nh_tend_d, dim3(gd.z, gd.x, gd.y), dim3(64, TD_I), 0, stream, g, dc, ds, f, istep);
  }
  void tend_c_launch(Tile& t, const NHFields& f, int istep) {
    const Geom& g = t.g;
    const dim3 grid(cfg.kz + 1, (g.nj + TC_J - 1) / TC_J, (g.ni + TC_I - 1) / TC_I), blk(TC_J, TC_I);
    if (hc.nsp) {
      // nqx = 5 belongs to ipptls = 2 and condtq to ipptls = 1 (set_condtq refuses the pair): the
      // QX instances exist with and without Budget only
      auto launch = [&](auto... x) {
        constexpr auto kern = k_nh_tend_c<true, decltype(x)...>;
        KLAUNCH_AS("k_nh_tend_c<true>", kern, grid, blk, 0, stream, g, dc, ds, f, (int)diag, istep, x...);
      };
      if (budget) launch(budget_args(t));
      else launch();
      // the chains of qi, qr, qs after it on the same stream
      KLAUNCH_AS("k_nh_qx_tend", k_nh_qx_tend<FamQx>, grid3(g.jce2 - g.jce1 + 1, g.ice2 - g.ice1 + 1, cfg.kz), BLK, 0,
                 stream, g, dc, ds, f, qx_args(t));
    } else {
      with_extras(t, [&](auto... x) {
        constexpr auto kern = k_nh_tend_c<false, decltype(x)...>;
        KLAUNCH_AS("k_nh_tend_c<false>", kern, grid, blk, 0, stream, g, dc, ds, f, (int)diag, istep, x...);
      });
    }
    // the tracers' chains after it on the same stream, a group of NQXH per z slice of kz levels
    if (ntr) {
      const dim3 tg = grid3(g.jce2 - g.jce1 + 1, g.ice2 - g.ice1 + 1, tr_groups() * cfg.kz);
      if (trbudget) {
        constexpr auto kern = k_nh_qx_tend<FamTr, TrBudget>;
        KLAUNCH_AS("k_nh_tr_tend<budget>", kern, tg, BLK, 0, stream, g, dc, ds, f, tr_args(t), trbud_args(t));
      } else {
        KLAUNCH_AS("k_nh_tr_tend", k_nh_qx_tend<FamTr>, tg, BLK, 0, stream, g, dc, ds, f, tr_args(t));
      }
    }
  }
  // the forecasts exchanged after the tendency kernels (atmc%qx, :381)
  std::vector<XField> cq_fields() const {
    std::vector<XField> v{{FK::CQV, cfg.kz}, {FK::CQC, cfg.kz}};
    add_qx(v, FK::CQX0, cfg.kz, 1);
    add_tr(v, FK::TRCQ, cfg.kz, 1);       // atmc%chi, Main/mod_tendency.F90:570
    return v;
  }

  // bdyval, non-hydrostatic: u, v, t, qv as the hydrostatic core (p* untouched), pp and w,
  // then the moisture inflow/outflow rules and the clock
  void nh_bdyval() {
    const int kz = cfg.kz;
    auto slices = [&](Tile& t) {
      Slices sl;
      for (int q = 0; q < 16; q++) sl.s[q] = t.sl[q];
      return sl;
    };
    each([&](Tile& t) {
      const Geom& g = t.g;
      KLAUNCH(k_bdyval_set, dim3((std::max(g.jde2 - g.jde1, g.ide2 - g.ide1) + 65) / 64, 6, kz), dim3(64), 0,
              stream, g, ds, bdy_args(t, 0));
      const int nperim = 2 * (g.ici2 - g.ici1 + 1) + 2 * (g.jce2 - g.jce1 + 1);
      KLAUNCH(k_nh_bdyval, dim3((nperim + 63) / 64, kz + 1), dim3(64), 0, stream, g, kz, ds, nhfields(t));
      KLAUNCH(k_nh_bdyval_w1, dim3(1), dim3(256), 0, stream, g, nhfields(t));
    });
    xch_slices();
    tracer_bdyval(-1, 0);                      // before the last tile's clock advance below
    for (size_t q = 0; q < tiles.size(); q++) {
      Tile& t = tiles[q];
      const int c = t.cur;
      if (hc.nsp)
        KLAUNCH(k_bdyval_qx, dim3(kz, hc.nsp), dim3(256), 0, stream, t.g, ds, qx_args(t), -1, (int)!cfg.present_qc,
                t.psa_[c], slices(t), slen);
      KLAUNCH(k_bdyval_qc, dim3(kz), dim3(256), 0, stream, t.g, (int)!cfg.present_qc, (int)(cfg.iboudy == 3 || cfg.iboudy == 4),
              t.a1qc[thp(t)], t.a1qv[thp(t)], t.psa_[c], slices(t), slen, ds, cfg.dtsec, (int)(q + 1 == tiles.size()),
              dflags);
    }
    tke_bdyval();
    hs.xbctime = hs.xbctime + cfg.dtsec;
  }

  // tend, whole or one of its two phases (TEND_PRE, TEND_POST); corr: what the hydrostatic
  // TEND_POST does with the split corrections
  void tend(Corr corr, int phase = TEND_ALL, bool slice = false) {
    if (subex && (phase & TEND_PRE)) slice = true;     // subex reads the export of this tend
    if (cfg.idynamic == 2) nh_tend(phase, slice);
    else {
      // part 1 of k_momentum / k_scalars beside the prologue exchange only in a whole tend (no
      // host work between) without the semi-Lagrangian pass that precedes them; a split tend
      // never runs it, so nothing is carried from one phase's call to the other's
      const bool post_inner = (phase & TEND_PRE) && tend_pre(slice, phase == TEND_ALL && !slice && cfg.isladvec != 1);
      subex_mid(phase);
      if (phase & TEND_POST) tend_post(corr, post_inner);
    }
    // the hydrostatic step's snapshot is written by k_split_correct's clock lane
    if ((phase & TEND_POST) && cfg.idynamic == 2) KLAUNCH(k_flag_snapshot, dim3(1), dim3(64), 0, stream, ds, dflags);
  }

  // returns whether part 1 of k_momentum / k_scalars ran beside the exchange (with_post allows it)
  bool tend_pre(bool slice, bool with_post) {
    const int kz = cfg.kz;
    // One exchange point for the whole prologue (Main/mod_tendency.F90:815-1116,
    // Main/mod_slice.F90:102-300): the decoupled fields are recomputed where read, so their
    // exchanges become exchanges of atm1 (width 1) and atm2 (idif = 2); p* travels 3 wide so
    // psdot and its reciprocals are formed on the ghost ring locally (no psdot exchanges).
    // atm1 travels 2 wide and atm2 3 wide: one more than the reference's widths, for the
    // ghost rings the kernels below compute in place of the later exchanges.
    // Halo/compute overlap (overlap()): the exchange on the engine's stream, part 1 of
    // k_columns (and of k_momentum / k_scalars) on the second; RCMDYN_NO_OVERLAP: the atm2 part
    // on the second stream beside k_columns, which reads only atm1 and p*.
    // (idiffu = 3: p*b 4 wide, for p*dotb on k_diffu6's 3-deep dot ghost rings)
    std::vector<XField> pro{{FK::PSA, 1, 3}, {FK::PSB, 1, cfg.idiffu == 3 ? 4 : 3}, {FK::A1U, kz, 2}, {FK::A1V, kz, 2},
                            {FK::A1T, kz, 2}, {FK::A1QV, kz, 2}, {FK::A1QC, kz, 2}};
    std::vector<XField> pro2{{FK::A2U, kz, 3}, {FK::A2V, kz, 3}, {FK::A2T, kz, 3}, {FK::A2QV, kz, 3},
                             {FK::A2QC, kz, 3}};
    add_qx(pro, FK::A1QX0, kz, 2);        // nqx = 5: qi, qr, qs with qc
    add_qx(pro2, FK::A2QX0, kz, 3);
    add_tr(pro, FK::TRA1, kz, 2);         // the tracers, as the species
    add_tr(pro2, FK::TRA2, kz, 3);
    // UW TKE: atm1 1 wide, atm2 idif wide (Main/mod_tendency.F90:871, 1079)
    if (cfg.ibltyp == 2) {
      pro.push_back({FK::A1TKE, kz + 1, 1});
      pro2.push_back({FK::A2TKE, kz + 1, cfg.idiffu == 3 ? 3 : 2});
    }
    // surface_pressures + 2-D reciprocals (:815-834), compute_omega columns, new_pressure,
    // geopotential in one launch (calc_coeff is formed where it is read, in k_momentum and
    // k_scalars)
    // ring: the trailing blocks too (the frame points outside the column box, then with qfuse
    // the copies of keep_point on the box's two outer rows and columns, every level)
    auto columns = [&](Tile& t, int part, int ncol, bool ring) {
      const Geom& g = t.g;
      int nsp = 0;
      if (ring) {
        const int W = g.jdx2() - g.jdx1() + 1, H = g.idx2() - g.idx1() + 1;
        const long nkeep = qfuse() ? (long)(4 * W + 4 * std::max(H - 4, 0)) * kz : 0;
        nsp = (int)((g.nj * (long)g.ni + COLT - 1) / COLT + (nkeep + COLT - 1) / COLT);
      }
      if (hc.nsp)
        KLAUNCH(k_columns<true>, dim3(ncol + nsp), dim3(COLT), col_lds(), stream, g, dc, ds, fields(t, part), t.ncolx, ncol);
      else
        KLAUNCH(k_columns<false>, dim3(ncol + nsp), dim3(COLT), col_lds(), stream, g, dc, ds, fields(t, part), t.ncolx, ncol);
    };
    if (overlap()) {
      // the whole exchange on the second stream; meanwhile part 1 of k_columns and, in a whole
      // step (k_momentum / k_scalars follow with no host work between), of k_momentum and
      // k_scalars; part 2 of each after the join
      pro.insert(pro.end(), pro2.begin(), pro2.end());
      side_begin();
      each([&](Tile& t) { if (t.nint) columns(t, 1, t.nint, false); });
      if (with_post) each([&](Tile& t) { post_launch(t, 1); });
      side_end(0);
      xchv(pro);
      ghosts_stale = false;
      massck_launch();
      side_join(0);
      each([&](Tile& t) { columns(t, t.nint ? 2 : 0, t.nint ? t.nring : t.nred, true); });
    } else {
      fork_point();
      xchv(pro);
      fork_after_exchange();
      xch_begin(pro2);
      ghosts_stale = false;
      massck_launch();
      each([&](Tile& t) { columns(t, 0, t.nred, true); });
      xch_join();
    }
    if (cfg.idiffu == 3) diffu6();
    if (slice) run_slice();
    return overlap() && with_post;
  }

  // idiffu = 3: the column terms of every tile, then (decomposed) one width-1 exchange so the
  // ring k_momentum / k_scalars compute holds the left neighbour's column as it computes it
  void diffu6() {
    const int kz = cfg.kz;
    each([&](Tile& t) {
      const Geom& g = t.g;
      KLAUNCH(k_diffu6, dim3((g.ide2 - g.ide1 + 64) / 64, kz, 4 + hc.nsp), dim3(64), 0, stream, g, dc, fields(t),
              qx_args(t));
    });
    if (halo) {
      std::vector<XField> d6{{FK::D6U, kz}, {FK::D6V, kz}, {FK::D6T, kz}, {FK::D6QV, kz}, {FK::D6QC, kz}};
      add_qx(d6, FK::D6QX0, kz, 0);
      xchv(d6);
    }
  }

  // k_momentum and k_scalars of one tile: part 1 the blocks in R (when it has any), part 2 the
  // others; part 0 all
  void post_launch(Tile& t, int part) {
    const Geom& g = t.g;
    const int mj2 = g.br ? g.jdi2 : g.jde2 + 1, mi2 = g.bt ? g.idi2 : g.ide2 + 1;
    const int pm = part == 0 ? 0 : (t.nint && t.mom_in ? part : (part == 1 ? -1 : 0));
    const int ps = part == 0 ? 0 : (t.nint && t.sca_in ? part : (part == 1 ? -1 : 0));
    const int mo = pm > 0 ? t.mj0 : g.jdi1, so = ps > 0 ? t.sj0 : g.jcx1();     // block-column origins
    const int mnx = (mj2 - mo + MBJ) / MBJ, mny = (mi2 - g.idi1 + MBI) / MBI;
    const int snx = (g.jcx2() - so + SBJ) / SBJ, sny = (g.icx2() - g.icx1() + SBI) / SBI;
    // o: the policy of the instances (an OptDefault or OptGeneric value), x: the extra blocks
    auto launch = [&](auto o, auto... x) {
      using O = decltype(o);
      if (sw.fuse_update && pm >= 0 && ps >= 0) {
        const int xcd = (int)((long)(g.jde2 - g.jde1 + 1) * (g.ide2 - g.ide1 + 1) < UPD_XCD_BELOW);
        constexpr auto kern = k_update<O, decltype(x)...>;
        KLAUNCH_AS(tend_name<decltype(x)...>("k_update", "k_update_bud"), kern,
                   dim3(std::max(mnx, snx), std::max(mny, sny), 2 * cfg.kz), dim3(SBT), 0, stream, g, dc, ds,
                   fields(t, pm), fields(t, ps), mnx, mny, snx, sny, xcd, x...);
        return;
      }
      if (pm >= 0)
        KLAUNCH_AS("k_momentum", k_momentum<O>, dim3(mnx, mny, cfg.kz), dim3(MBT), 0, stream, g, dc, ds,
                   fields(t, pm));
      if (ps >= 0) {
        constexpr auto kern = k_scalars<O, decltype(x)...>;
        KLAUNCH_AS(tend_name<decltype(x)...>("k_scalars", "k_scalars_bud"), kern, dim3(snx, sny, cfg.kz), dim3(SBT),
                   0, stream, g, dc, ds, fields(t, ps), x...);
      }
    };
    // the default-set instances take no extra block (optset_instance: generic with any of them)
    if (opt_instance(fields(t)) == OPT_DEFAULT) launch(OptDefault{});
    else with_extras(t, [&](auto... x) { launch(OptGeneric{}, x...); });
  }

  void tend_post(Corr corr, bool post_inner) {
    const int kz = cfg.kz, ns = cfg.nsplit;
    const bool fused = split_fused();
    // semi-Lagrangian moisture advection (isladvec = 1): owned points, then the ring k_scalars
    // also computes comes from the neighbours
    if (cfg.isladvec == 1) {
      each([&](Tile& t) {
        const Geom& g = t.g;
        KLAUNCH(k_sladv, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, kz), BLK, 0, stream, g, dc, ds, fields(t),
                qx_args(t));
      });
      std::vector<XField> sl{{FK::SLQV, kz}, {FK::SLQC, kz}};
      add_qx(sl, FK::SLQX0, kz, 0);
      xchv(sl, 1, 0);
    }
    // fused tendencies + forecast + time filter (part 2 when tend_pre ran part 1)
    each([&](Tile& t) { post_launch(t, post_inner ? 2 : 0); });
    tke_step();
    if (hc.nsp) {
      // nqx = 5: the hydrometeors beyond qc, their forecast (and ring), then the fix and filter
      each([&](Tile& t) {
        const Geom& g = t.g;
        KLAUNCH_AS("k_qx_tend", k_qx_tend<FamQx>,
                   dim3((g.jcx2() - g.jcx1() + QBJ) / QBJ, (g.icx2() - g.icx1() + QBI) / QBI, kz), dim3(QBT), 0, stream, g,
                   dc, ds, fields(t), qx_args(t));
      });
      if (!fused) {
        std::vector<XField> cq;
        add_qx(cq, FK::CQX0, kz, 1);
        xchv(cq);
      }
      each([&](Tile& t) {
        const Geom& g = t.g;
        KLAUNCH_AS("k_qx_fix", k_qx_fix<FamQx>, grid3(g.jdx2() - g.jdx1() + 1, g.idx2() - g.idx1() + 1, kz), BLK, 0,
                   stream, g, dc, qx_args(t));
        if (serial_with_corr()) return;          // the serial chains then run in launch_corrections
        KLAUNCH_AS("k_qx_serial", k_qx_serial<FamQx>, dim3(hc.nsp * kz), dim3(negfix_threads(g)),
                   sizeof(double) * negfix_lds(g), stream, g, dc, qx_args(t));
        KLAUNCH_AS("k_qx_post", k_qx_post<FamQx>, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, hc.nsp * kz), BLK, 0,
                   stream, g, dc, qx_args(t));
      });
    }
    if (ntr) {
      // the tracers after the species, on the same qdot, scaled xkc and mass fluxes: a group of
      // NQXH per z slice of kz levels; the forecast on the ring as the species', so no exchange
      // of atmc%chi unless the split step is not fused; the serial chains straight after the fix
      // (nothing of the step waits for them)
      each([&](Tile& t) {
        const Geom& g = t.g;
        const Fields f = fields(t);
        const dim3 tg((g.jcx2() - g.jcx1() + QBJ) / QBJ, (g.icx2() - g.icx1() + QBI) / QBI, tr_groups() * kz);
        if (trbudget) {
          constexpr auto kern = k_qx_tend<FamTr, TrBudget>;
          KLAUNCH_AS("k_tr_tend<budget>", kern, tg, dim3(QBT), 0, stream, g, dc, ds, f, tr_args(t), trbud_args(t));
        } else {
          KLAUNCH_AS("k_tr_tend", k_qx_tend<FamTr>, tg, dim3(QBT), 0, stream, g, dc, ds, f, tr_args(t));
        }
      });
      if (!fused) {
        std::vector<XField> cq;
        add_tr(cq, FK::TRCQ, kz, 1);
        xchv(cq);
      }
      each([&](Tile& t) { tracer_fix(t); });
    }
    if (!fused) xch({{FK::CQV, kz}, {FK::CQC, kz}});     // else k_scalars computed the ring
    // negative-moisture fix + p* RA filter + qv/qc RAW filter; then the new level is current
    // (qfuse: done by k_columns, k_scalars and the extra blocks below)
    each([&](Tile& t) {
      if (!qfuse()) KLAUNCH(k_qfilter, grid3((t.g.nj + 1) / 2, t.g.ni, kz), BLK, 0, stream, t.g, dc, fields(t));
      t.cur = 1 - t.cur;
    });
    // splitf, Main/mod_split.F90:243-461
    if (!fused) xch({{FK::PSA, 1}, {FK::A1U, kz, 1, 2}, {FK::A1V, kz, 1, 2}, {FK::A2U, kz, 1, 2}, {FK::A2V, kz, 1, 2}});
    const bool wide = fused && halo;     // k_split_project also fills the wide frames
    each([&](Tile& t) {
      const Geom& g = t.g;
      const int c = t.cur, o = 1 - c;
      const QFix q = qfix(t);
      const int nxp = (g.jdx2() - g.jde1 + SPC) / SPC, nproj = nxp * (g.idx2() - g.ide1 + 1);
      // extra blocks: qfuse the parallel fix of the listed negatives (grid-stride), else the
      // serial sweeps of the planes k_qfilter flagged
      const int nextra = qfuse() ? NEGFIX_BLOCKS * 512 / (SPC * SPG) : 2 * kz;   // 32 768 threads
      KLAUNCH(k_split_project, dim3(nproj + nextra), dim3(SPC * SPG), sizeof(double) * 4 * SPC * (size_t)kz, stream, g,
              dc, t.a1u[c], t.a1v[c],
                         t.a2u[c], t.a2v[c], t.a1t[c], t.a2t[c], t.psa_[c], t.psb_[c], t.msfd, t.mapf, t.dstor,
                         t.hstor, t.deld, t.delh, t.psdota, nxp, nproj, q, t.gw, wide ? t.wdeld : nullptr,
                         t.wdelh, t.wpsdota, t.wpsa, t.a2u[o], t.a2v[o]);
    });
    // spstep, :463-669: forward step then leapfrog, two time slots + forcing slot 3
    if (wide) {
      // one depth-SPX exchange of every split-step input instead of three per sub-step
      xch_wide({{&Tile::wdeld, 3 * ns}, {&Tile::wdelh, 3 * ns}, {&Tile::wpsa, 1}, {&Tile::wpsdota, 1}}, SPX);
    }
    if (fused) {
      each([&](Tile& t) {
        const Geom& g = t.g;
        // 16 x 16 owned points per block, or 8 x 8 when that leaves most CUs idle (a rank tile
        // of a multi-GPU run): the sub-step chain is the block's latency, and 8 x 8 blocks cut
        // it per block (576 region points instead of 1024) at the price of more halo points
        const int W = g.jcx2() - g.jcx1() + 1, H = g.icx2() - g.icx1() + 1;
        const bool small = (long)((W + 15) / 16) * ((H + 15) / 16) * ns < SP8_BELOW;
        const Geom& w = halo ? t.gw : g;
        const double *dd = halo ? t.wdeld : t.deld, *dh = halo ? t.wdelh : t.delh;
        const double *mx = halo ? t.wmsfx : t.msfx, *md = halo ? t.wmsfd : t.msfd;
        const double *pd = halo ? t.wpsdota : t.psdota, *mp = halo ? t.wmapf : t.mapf;
        const double* pa = halo ? t.wpsa : t.psa_[t.cur];
        if (small)
          KLAUNCH(k_spstep_fused<8>, dim3((W + 7) / 8, (H + 7) / 8, ns), dim3(8 + 2 * SPH, 8 + 2 * SPH), 0, stream, g, w,
                  dc, dd, dh, mx, md, pd, mp, pa, t.ddsum, t.dhsum);
        else
          KLAUNCH(k_spstep_fused<16>, dim3((W + 15) / 16, (H + 15) / 16, ns), dim3(16 + 2 * SPH, 16 + 2 * SPH), 0,
                  stream, g, w, dc, dd, dh, mx, md, pd, mp, pa, t.ddsum, t.dhsum);
      });
    } else {
      each([&](Tile& t) {
        const Geom& g = t.g;
        KLAUNCH(k_spstep_init, grid3(g.jde2 - g.jde1 + 1, g.ide2 - g.ide1 + 1, 1), BLK, 0, stream, g,
                           dc, t.deld, t.delh, t.ddsum, t.dhsum);
      });
    }
    for (int l = 1; l <= ns && !fused; l++) {
      int n0 = 1, n1 = 2, n2 = n0;
      const int m2 = (int)hc.aam[l - 1] * 2;
      sp_substep(l, n0, n0, n0, n1, 0);
      for (int n = 2; n <= m2; n++) {
        sp_substep(l, n1, n0, n1, n2, 1);
        n0 = n1; n1 = n2; n2 = n0;
      }
    }
    // the fused split step also produced ddsum/dhsum on the left/bottom ghost ring
    if (!fused) xch({{FK::DHSUM, ns}}, 1, 1);
    // corrections + rcmtimer advance (last tile's launch); deferred to bdyval in the drop-in pair
    if (corr != Corr::Defer) launch_corrections(corr == Corr::WithBdy);
    hs.lcount += 1;
    if (hs.lcount == 2) hs.dt = 2.0 * cfg.dtsec;
  }

  // the split corrections + rcmtimer advance (last tile's launch); bdy: with bdyval's boundary
  // lines (k_split_correct_bdy; k_bdyval_qc then advances the clock)
  void launch_corrections(bool bdy) {
    const int kz = cfg.kz, ns = cfg.nsplit;
    for (size_t q = 0; q < tiles.size(); q++) {
      Tile& t = tiles[q];
      const Geom& g = t.g;
      const int c = t.cur;
      const long npts = (long)((g.jdx2() - g.jde1 + 2) / 2) * (g.idx2() - g.ide1 + 1);   // point pairs per level
      dim3 gr((unsigned)((npts + 255) / 256), 1, kz);
      const int adv = (int)(q + 1 == tiles.size());
      // qfuse: trailing z slices run the serial sweeps of the flagged moisture planes
      const QFix qf = qfix(t);
      // (nqx = 5: in a launch of their own after the corrections, k_negfix_serial, whose block per
      // plane can run the dense wavefront; the patchy hydrometeor fields come with patchy qc)
      const bool own = hc.nsp > 0;
      const int nser = qfuse() && !own ? (int)((2 * kz + gr.x * gr.y - 1) / (gr.x * gr.y)) : 0;
      gr.z += nser;
      const size_t slds = nser ? sizeof(double) * negfix_sweep_lds(g) : 0;     // the sweeps' LDS (row sweeps only)
      if (bdy) {
        // the bdyval blocks: leading z slices of 6 lines x bdy_chunks 64-point chunks x kz
        // levels, 4 per block
        const unsigned per = 4 * gr.x * gr.y;
        gr.z += (6 * bdy_chunks(g) * kz + per - 1) / per;
        const BdyArgs ba = bdy_args(t, 1);
#define RCM_SCB(NS_) KLAUNCH(k_split_correct_bdy<NS_>, gr, BLK, slds, stream, g, dc, t.ddsum, t.dhsum, t.psdota, t.msfd, \
                             ds, adv, red, red_total, ba, qf, nser)
        switch (ns) { case 1: RCM_SCB(1); break; case 2: RCM_SCB(2); break; case 3: RCM_SCB(3); break; default: RCM_SCB(4); }
#undef RCM_SCB
      } else {
#define RCM_SC(NS_) KLAUNCH(k_split_correct<NS_>, gr, BLK, slds, stream, g, dc, t.ddsum, t.dhsum, t.psdota, t.msfd,   \
                            t.psa_[c], t.psb_[c], t.a1t[c], t.a2t[c], t.a1u[c], t.a1v[c], t.a2u[c], t.a2v[c], ds, adv, \
                            red, red_total, dflags, qf, nser)
        switch (ns) { case 1: RCM_SC(1); break; case 2: RCM_SC(2); break; case 3: RCM_SC(3); break; default: RCM_SC(4); }
#undef RCM_SC
      }
      if (serial_with_corr()) {
        // the qv / qc and the species planes' serial chains in one launch (the species' operands
        // of the step before tend_post's flip), then their filters
        const QxArgs qx = qx_args(t, 1 - t.cur);
        KLAUNCH(k_negfix_serial_qx, dim3((2 + hc.nsp) * kz), dim3(negfix_threads(g)), sizeof(double) * negfix_lds(g),
                stream, g, dc, qf, qx);
        KLAUNCH(k_negfix_post, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, 2 * kz), BLK, 0, stream, g, dc, qf);
        KLAUNCH_AS("k_qx_post", k_qx_post<FamQx>, grid3(g.jci2 - g.jci1 + 1, g.ici2 - g.ici1 + 1, hc.nsp * kz), BLK, 0,
                   stream, g, dc, qx);
      } else if (qfuse() && own) {
        KLAUNCH(k_negfix_serial, dim3(2 * kz), dim3(negfix_threads(g)), sizeof(double) * negfix_lds(g), stream, g, dc,
                qf);
      }
    }
  }
  // not with a communicator: a rank-local call (a get) between tend and bdyval would then issue
  // the step's flag reduction on one rank only
  bool can_defer() const {
    return cfg.idynamic != 2 && !comm && !sw.no_fuse_bdy && !sw.no_defer_corr && (!halo || split_fused());
  }
  Corr drop_in_corr() const { return can_defer() ? Corr::Defer : Corr::Launch; }
  // a call other than rcmdyn_bdyval after a tend that deferred its corrections: launch them
  void settle() {
    if (pend == Pending::Tend) {  // the lazy tend's own graph (captured with deferred corrections)
      replay(Graph::Tend, pend_par);
      pend = Pending::Corrections;
    }
    if (pend != Pending::Corrections) return;
    launch_corrections(false);     // if this throws, the corrections stay pending for the next call
    pend = Pending::None;
    note_step(hs.lcount);
  }
  // rcmdyn_bdyval after a deferring tend: the corrections with the boundary lines, then the
  // rest of bdyval as rcmdyn_step runs it
  void fused_bdyval() {
    launch_corrections(true);
    pend = Pending::None;
    bdyval(true);
  }

  // one spstep substep: gradient of delh(src) -> (uu,vv) -> divergence -> mode update
  void sp_substep(int l, int src, int n0, int n1, int nn, int leap) {
    xch_delh_slot(l, src);
    each([&](Tile& t) {
      const Geom& g = t.g;
      KLAUNCH(k_spstep_grad, grid3(g.jdi2 - g.jdi1 + 1, g.idi2 - g.idi1 + 1, 1), BLK, 0, stream, g, dc, l,
                         src, t.delh, t.msfx, t.msfd, t.psdota, t.uu, t.vv);
    });
    xch({{FK::UU, 1}, {FK::VV, 1}}, 1, 2);
    each([&](Tile& t) {
      const Geom& g = t.g;
      KLAUNCH(k_spstep_update, grid3(g.jce2 - g.jce1 + 1, g.ice2 - g.ice1 + 1, 1), BLK, 0, stream, g, dc,
                         l, n0, n1, nn, leap, t.uu, t.vv, t.mapf, t.psa_[t.cur], t.deld, t.delh, t.ddsum, t.dhsum);
    });
  }

  // the moisture fix-up operands for the current parity (after the flip of tend_post): the
  // forecasts and fixed values, the old (o*) and new (n*) q buffers, the filtered p*
  QFix qfix(Tile& t) {
    const int c = t.cur, o = 1 - c;
    QFix q{t.cqv, t.cqc, t.fqv, t.fqc, t.a1qv[o], t.a1qc[o], t.a2qv[o], t.a2qc[o],
           t.a1qv[c], t.a1qc[c], t.a2qv[c], t.a2qc[c], t.psa_[c], t.psb_[c], t.psc, t.psa_[o], t.psb_[o],
           t.depplane, nullptr, nullptr, nullptr};
    if (qfuse()) { q.negcnt = t.negcnt; q.neglist = t.neglist; q.depf = t.depqf; }
    return q;
  }

  BdyArgs bdy_args(Tile& t, int set_ps) {
    const int c = t.cur, q = thp(t);
    BdyArgs a{};
    a.a1u = t.a1u[c]; a.a1v = t.a1v[c]; a.a1t = t.a1t[q]; a.a1qv = t.a1qv[q]; a.a1qc = t.a1qc[q];
    a.a2u = t.a2u[c]; a.a2v = t.a2v[c]; a.a2t = t.a2t[q]; a.a2qv = t.a2qv[q]; a.a2qc = t.a2qc[q];
    a.psa = t.psa_[c]; a.psb = t.psb_[c];
    a.ub0 = t.ub0; a.ubt = t.ubt; a.vb0 = t.vb0; a.vbt = t.vbt; a.tb0 = t.tb0; a.tbt = t.tbt;
    a.qb0 = t.qb0; a.qbt = t.qbt; a.pb0 = t.pb0; a.pbt = t.pbt;
    for (int q = 0; q < 16; q++) a.sl.s[q] = t.sl[q];
    a.slen = slen;
    a.set_ps = set_ps;
    return a;
  }

  // lines_done: the boundary lines and slices were set by k_split_correct_bdy (Corr::WithBdy),
  // and the clock advance of the step moves here (last tile's launch)
  void bdyval(bool lines_done) {
    if (cfg.idynamic == 2) { nh_bdyval(); return; }
    const int kz = cfg.kz;
    if (!lines_done) {
      each([&](Tile& t) {
        const Geom& g = t.g;
        KLAUNCH(k_bdyval_set, dim3((std::max(g.jde2 - g.jde1, g.ide2 - g.ide1) + 65) / 64, 6, kz), dim3(64), 0,
                stream, g, ds, bdy_args(t, 1));
      });
      // the ghost-ring step wrote the slice entries past the tile itself (k_bdyval_set)
      if (ghosts_stale || !split_fused()) xch_slices();
    }
    tracer_bdyval(lines_done ? 1 : -1, (int)lines_done);      // before the last tile's clock advance below
    for (size_t q = 0; q < tiles.size(); q++) {
      Tile& t = tiles[q];
      const int adv = q + 1 == tiles.size() ? (lines_done ? 2 : 1) : 0;
      if (hc.nsp)
        KLAUNCH(k_bdyval_qx, dim3(kz, hc.nsp), dim3(256), 0, stream, t.g, ds, qx_args(t), lines_done ? 1 : -1,
                (int)!cfg.present_qc, t.psa_[t.cur], bdy_args(t, 1).sl, slen);
      KLAUNCH(k_bdyval_qc, dim3(kz), dim3(256), 0, stream, t.g, (int)!cfg.present_qc, (int)(cfg.iboudy == 3 || cfg.iboudy == 4),
              t.a1qc[t.cur], t.a1qv[t.cur], t.psa_[t.cur], bdy_args(t, 1).sl, slen, ds, cfg.dtsec, adv, dflags);
    }
    tke_bdyval();
    hs.xbctime = hs.xbctime + cfg.dtsec;
  }

  // one tend + bdyval of rcmdyn_step (no host work between them): the hydrostatic bdyval's
  // boundary lines and slices then run in k_split_correct_bdy, only its moisture
  // inflow/outflow pass in a launch of its own.  A decomposed domain needs no slice exchange
  // then (split_fused: every tile computes its ghost ring).
  void step_once() {
    const bool with_bdy = cfg.idynamic != 2 && !sw.no_fuse_bdy && (!halo || split_fused());
    tend(with_bdy ? Corr::WithBdy : Corr::Launch);
    bdyval(with_bdy);
  }

  // ------------------------------------------------------------------ graph replay
  // graph replay applies: not profiling, not an RCCL transport that cannot be captured, and
  // for NH not a step of another shape (istep on the first two steps, the day alarm's
  // radiative coefficients)
  bool graph_ok(int nsteps = 1) const {
    if (sw.no_graph || prof || (comm && !comm->graph_safe())) return false;
    if (cfg.idynamic != 2) return true;
    for (int q = 0; q < nsteps; q++)
      if (hs.lcount + q < 2 || nh_day_alarm_at(hs.lcount + q)) return false;
    return true;
  }
  // host bookkeeping of a replayed tend / bdyval (what tend() and bdyval() do on the host)
  void replayed_tend() {
    if (cfg.idynamic != 2) for (auto& t : tiles) t.cur = 1 - t.cur;
    else if (sw.nh_tfuse) for (auto& t : tiles) t.tq = 1 - t.tq;
    hs.lcount += 1;
    if (hs.lcount == 2) hs.dt = 2.0 * cfg.dtsec;
    sbx_pre = sbx_ran = false;         // a whole tend ends the split path's state, as subex_mid does eagerly
  }
  void replayed_bdyval() { hs.xbctime = hs.xbctime + cfg.dtsec; }

  void step(int n) {
    condtq_ready("rcmdyn_step");
    subex_ready("rcmdyn_step");
    prepare();
    settle();
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, stream));
    for (int s = 0; s < n; s++) {
      check(FLAG_LAG);
      const bool two = sw.graph_steps == 2 && s + 1 < n && graph_ok(2);
      if (two || graph_ok()) {
        replay(two ? Graph::TwoSteps : Graph::Step, gpar());
        replayed_tend();
        replayed_bdyval();
      } else {
        step_once();
      }
      if (two) {                       // the second step of the graph
        note_step(hs.lcount);
        replayed_tend();
        replayed_bdyval();
        s++;
      }
      note_step(hs.lcount, s == n - 1);
    }
    HIPCHK(hipEventRecord(e1, stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    last_ms = n > 0 ? (double)ms / n : 0.0;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    check(0);
  }

  // the drop-in call sequence of RCM_run (Main/mod_regcm_interface.F90:189,208): each call
  // replays its own captured graph and returns without synchronising the stream
  void tend_call() {
    condtq_ready("rcmdyn_tend");
    subex_ready("rcmdyn_tend");
    begin_tend();
    const int par = gpar();
    const Corr corr = drop_in_corr();
    if (graph_ok()) {
      ensure(Graph::Tend, par);
      if (sw.lazy_tend && corr == Corr::Defer && !ghosts_stale) {
        ensure(Graph::Step, par);
        pend = Pending::Tend;
        pend_par = par;
        replayed_tend();               // the clock and parities as after the launch
        return;                        // note_step: at the launch
      }
      replay(Graph::Tend, par);
      replayed_tend();
    } else {
      tend(corr);
    }
    tend_done(corr);
  }
  void begin_tend() { prepare(); settle(); check(FLAG_LAG); }     // every drop-in tend entry point starts so
  // a tend was launched: its corrections are pending, or else its flags are noted (now, not at their launch)
  void tend_done(Corr corr) {
    if (corr == Corr::Defer) pend = Pending::Corrections;
    else note_step(hs.lcount);
  }
  // rcmdyn_tend_pre_physics / rcmdyn_tend_post_physics: tend's two phases, run eagerly around
  // the host's physics; the corrections go with the next rcmdyn_bdyval as after rcmdyn_tend
  void tend_pre_physics() { begin_tend(); tend(Corr::Launch, TEND_PRE, true); }
  void tend_post_physics() {
    condtq_ready("rcmdyn_tend_post_physics");
    subex_ready("rcmdyn_tend_post_physics");
    if (subex && !sbx_pre)
      throw std::runtime_error("rcmdyn_tend_post_physics: subex is on and no rcmdyn_tend_pre_physics ran for this tend");
    begin_tend();
    const Corr corr = drop_in_corr();
    tend(corr, TEND_POST);
    tend_done(corr);
  }
  void bdyval_call() {
    prepare();
    if (pend == Pending::Tend) {  // the lazy tend and this bdyval: one step graph
      replay(Graph::Step, pend_par);
      pend = Pending::None;
      replayed_bdyval();
      note_step(hs.lcount);
      return;
    }
    // after a put the ghost rings are not step results: bdyval runs eagerly (its slice
    // exchange depends on that, bdyval())
    const bool graph = graph_ok() && !ghosts_stale;
    if (pend == Pending::Corrections) {
      if (graph) {
        replay(Graph::CorrBdyval, gpar());
        pend = Pending::None;
        replayed_bdyval();
      } else {
        fused_bdyval();
      }
      note_step(hs.lcount);
    } else if (graph) {
      replay(Graph::Bdyval, gpar());
      replayed_bdyval();
    } else {
      bdyval(false);
    }
  }

  // record one graph for the ping-pong parity the engine is at (par = gpar()); the host
  // bookkeeping done in tend() / bdyval() and the pending state are rolled back, the replay
  // redoes them per launch
  void capture(Graph kind, int par) {
    const StepState save = hs;
    const Pending saved = pend;
    const bool saved_pre = sbx_pre, saved_ran = sbx_ran;
    std::vector<int> curs, tqs;
    for (auto& t : tiles) { curs.push_back(t.cur); tqs.push_back(t.tq); }
    hipGraph_t graph;
    if (subex) slice_allocs();        // a whole tend with subex on holds the mkslice export
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    switch (kind) {
      case Graph::Step: step_once(); break;
      case Graph::TwoSteps: step_once(); step_once(); break;
      case Graph::Tend: tend(drop_in_corr()); break;
      case Graph::Bdyval: bdyval(false); break;
      case Graph::CorrBdyval: fused_bdyval(); break;
      case Graph::Count: break;
    }
    HIPCHK(hipStreamEndCapture(stream, &graph));
    HIPCHK(hipGraphInstantiate(&graphs[(int)kind][par], graph, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(graph));
    hs = save;
    pend = saved;
    sbx_pre = saved_pre; sbx_ran = saved_ran;
    for (size_t q = 0; q < tiles.size(); q++) { tiles[q].cur = curs[q]; tiles[q].tq = tqs[q]; }
  }
  void ensure(Graph kind, int par) { if (!graphs[(int)kind][par]) capture(kind, par); }
  // launch a graph, captured first if absent; the caller moves the pending state only after this
  // returns.  RCMDYN_INJECT_LAUNCH_FAILURE=n counts the launches that carry a lazy tend (settle's
  // Tend, bdyval_call's Step): the n-th fails before it is issued.
  void replay(Graph kind, int par) {
    ensure(kind, par);
    if (pend == Pending::Tend && inject_fail > 0 && --inject_fail == 0)
      throw std::runtime_error("rcmdyn: injected launch failure");
    HIPCHK(hipGraphLaunch(graphs[(int)kind][par], stream));
  }

  // rcmdyn_exchange_plan: the communication calls of put + bdyval + nsteps x (tend + bdyval),
  // the drop-in's start (the initial bdyval after the state put, with its slice exchange) and
  // the eager step sequence every rank runs (graph replay issues the same calls in the same order)
  void plan_run(int nsteps) {
    prepare();
    ghosts_stale = true;           // as after rcmdyn_put
    bdyval(false);
    for (int s = 0; s < nsteps; s++) {
      step_once();
      note_step(hs.lcount, s == nsteps - 1);
    }
  }

  void kernel_times(int nsteps, int cap, char* names, int32_t* launches, double* avg, int32_t* count) {
    condtq_ready("rcmdyn_kernel_times");
    subex_ready("rcmdyn_kernel_times");
    prepare();
    quiesce();
    KernelProf kp;
    {
      struct Scope { KernelProf*& p; ~Scope() { p = nullptr; } } profiling{prof = &kp};   // however the steps end
      for (int s = 0; s < nsteps; s++) step_once();
    }
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<std::string> order;
    std::vector<double> tot;
    std::vector<int> cnt;
    for (auto& r : kp.rec) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, r.second.first, r.second.second));
      size_t q = std::find(order.begin(), order.end(), r.first) - order.begin();
      if (q == order.size()) { order.push_back(r.first); tot.push_back(0.0); cnt.push_back(0); }
      tot[q] += ms;
      cnt[q] += 1;
    }
    const int n = std::min<int>(cap, (int)order.size());
    for (int q = 0; q < n; q++) {
      std::memset(names + 48 * q, 0, 48);
      std::strncpy(names + 48 * q, order[q].c_str(), 47);
      launches[q] = cnt[q];
      avg[q] = tot[q] / cnt[q];
    }
    *count = n;
  }

  void set_time(long long lcount, double dt, double xbctime) {
    quiesce();
    pending.clear();
    gpending.clear();
    StepState st;
    HIPCHK(hipMemcpy(&st, ds, sizeof(st), hipMemcpyDeviceToHost));
    st.lcount = lcount; st.dt = dt; st.xbctime = xbctime; st.nanflag = 0; st.slflag = 0;
    HIPCHK(hipMemcpy(ds, &st, sizeof(st), hipMemcpyHostToDevice));
    hs.lcount = lcount; hs.dt = dt; hs.xbctime = xbctime;
  }

  void reductions(double out[3]) {
    settle();
    check(0);
    HIPCHK(hipStreamSynchronize(stream));
    StepState st;
    HIPCHK(hipMemcpy(&st, ds, sizeof(st), hipMemcpyDeviceToHost));
    out[0] = st.ptntot; out[1] = st.pt2tot; out[2] = cfg.idynamic == 2 ? st.cflmax : 0.0;
    if (comm && cfg.tile_count < ntiles) {        // sumall / maxall over the ranks
      double* d = nullptr;
      HIPCHK(hipMalloc(&d, 3 * sizeof(double)));
      double hv[3] = {out[0], out[1], out[2]};
      HIPCHK(hipMemcpy(d, hv, sizeof(hv), hipMemcpyHostToDevice));
      comm->allreduce_sum(d, 2, stream);
      comm->allreduce_max_d(d + 2, 1, stream);
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(hv, d, sizeof(hv), hipMemcpyDeviceToHost));
      (void)hipFree(d);
      out[0] = hv[0]; out[1] = hv[1]; out[2] = hv[2];
    }
  }

  void diagnostics(double out[4]) {
    quiesce();
    check_now();
    StepState st;
    HIPCHK(hipMemcpy(&st, ds, sizeof(st), hipMemcpyDeviceToHost));
    out[0] = st.ptntot; out[1] = st.pt2tot; out[2] = std::isnan(st.ptntot) ? 1.0 : 0.0; out[3] = st.nanflag;
  }
};

// ======================================================================== C-ABI
namespace {
template <class F>
int guard(rcmdyn_t* h, F fn) {
  try {
    fn();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    if (h) h->err = e.what();
    return 1;
  }
}
}  // namespace

extern "C" {

// RCMDYN_SEGV_TRACE=1 (opt-in host debugging aid): print the native backtrace of a
// segmentation fault, then hand the signal to the handler that was installed before (Python's
// faulthandler, a host's own), or the default action
static struct sigaction g_prev_segv;
static void segv_trace(int sig, siginfo_t* info, void* uc) {
  void* bt[64];
  const int n = backtrace(bt, 64);
  const char msg[] = "rcmdyn: fatal signal, native backtrace:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(bt, n, 2);
  sigaction(sig, &g_prev_segv, nullptr);
  if (g_prev_segv.sa_flags & SA_SIGINFO) {
    if (g_prev_segv.sa_sigaction) { g_prev_segv.sa_sigaction(sig, info, uc); return; }
  } else if (g_prev_segv.sa_handler != SIG_DFL && g_prev_segv.sa_handler != SIG_IGN) {
    g_prev_segv.sa_handler(sig);
    return;
  }
  std::raise(sig);
}
static void install_segv_trace() {
  static bool done = false;
  if (done || !std::getenv("RCMDYN_SEGV_TRACE")) return;
  done = true;
  void* warm[1];
  (void)backtrace(warm, 1);           // loads the unwinder now: backtrace's first call allocates
  struct sigaction sa {};
  sa.sa_sigaction = segv_trace;
  sa.sa_flags = SA_SIGINFO | SA_NODEFER;
  sigemptyset(&sa.sa_mask);
  sigaction(SIGSEGV, &sa, &g_prev_segv);
}

int rcmdyn_create(const rcmdyn_config* cfg, rcmdyn_t** out) {
  if (!cfg || !out) { g_last_error = "rcmdyn_create: null argument"; return 1; }
  install_segv_trace();
  auto* h = new rcmdyn_engine();
  int rc = guard(h, [&] { h->create(cfg); });
  if (rc) {
    g_last_error = h->err;
    h->destroy();
    delete h;
    *out = nullptr;
    return rc;
  }
  *out = h;
  return 0;
}

int rcmdyn_exchange_plan(const rcmdyn_config* cfg, int32_t nsteps, int64_t* ops, int64_t cap, int64_t* count) {
  if (!cfg || !count || nsteps < 0 || cap < 0 || (cap > 0 && !ops)) {
    g_last_error = "rcmdyn_exchange_plan: bad argument";
    return 1;
  }
  std::vector<PlanOp> log;
  auto* h = new rcmdyn_engine();
  int rc = guard(h, [&] {
    h->create(cfg, &log);
    h->plan_run(nsteps);
  });
  if (rc) g_last_error = h->err;
  h->destroy();
  delete h;
  if (rc) return rc;
  *count = (int64_t)log.size();
  for (int64_t q = 0; q < std::min<int64_t>(cap, (int64_t)log.size()); q++) {
    const PlanOp& o = log[q];
    const int64_t v[7] = {o.seq, o.kind, o.chan, o.dir, o.peer, o.count, o.sig};
    std::memcpy(ops + 7 * q, v, sizeof(v));
  }
  return 0;
}

int rcmdyn_overlap_shares(const rcmdyn_config* cfg, int32_t* out, int32_t cap) {
  if (!cfg || !out || cap < 0) {
    g_last_error = "rcmdyn_overlap_shares: bad argument";
    return 1;
  }
  std::vector<PlanOp> log;
  auto* h = new rcmdyn_engine();
  int rc = guard(h, [&] {
    h->create(cfg, &log);
    for (size_t q = 0; q < h->tiles.size() && (int)q < cap; q++) {
      const Tile& t = h->tiles[q];
      const Geom& g = t.g;
      const int mj2 = g.br ? g.jdi2 : g.jde2 + 1, mi2 = g.bt ? g.idi2 : g.ide2 + 1;
      const bool ov = h->overlap() && t.rja <= t.rjb && t.ria <= t.rib;
      const int32_t v[6] = {
          ov ? (int32_t)((long)(t.rjb - t.rja + 1) * (t.rib - t.ria + 1)) : 0,
          (int32_t)((long)(g.jdx2() - g.jdx1() + 1) * (g.idx2() - g.idx1() + 1)),
          ov ? (int32_t)t.mom_p1 : 0, (int32_t)((long)(mj2 - g.jdi1 + 1) * (mi2 - g.idi1 + 1)),
          ov ? (int32_t)t.sca_p1 : 0, (int32_t)((long)(g.jcx2() - g.jcx1() + 1) * (g.icx2() - g.icx1() + 1))};
      std::memcpy(out + 6 * q, v, sizeof(v));
    }
  });
  if (rc) g_last_error = h->err;
  h->destroy();
  delete h;
  return rc;
}

int rcmdyn_destroy(rcmdyn_t* h) {
  if (!h) return 0;
  // a lazy tend (or deferred corrections) still pending is launched first, so the host's last
  // tend is not dropped without a word: its failure is this call's return code
  const int rc0 = guard(h, [&] { h->settle(); });
  const std::string err0 = h->err;
  const int rc = guard(h, [&] { h->destroy(); });
  if (rc0 || rc) g_last_error = rc0 ? err0 : h->err;      // h is gone: rcmdyn_last_error(NULL)
  delete h;
  return rc0 ? rc0 : rc;
}

const char* rcmdyn_last_error(rcmdyn_t* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int rcmdyn_set_nproc(int32_t nproc, int32_t jx, int32_t iy, int32_t cpus[2]) {
  // Main/mpplib/mod_mppparam.F90:1152-1186
  if (nproc < 1 || !cpus) return 1;
  if (nproc == 1) { cpus[0] = 1; cpus[1] = 1; return 0; }
  if (nproc < 4) { cpus[0] = nproc; cpus[1] = 1; return 0; }
  int cj = ((int)std::lround(std::sqrt((double)nproc)) / 2) * 2;
  if (iy > (int)(1.5 * (double)jx)) {
    cj -= 1;
    while (nproc % cj != 0) cj -= 1;
  } else if (jx > (int)(1.5 * (double)iy)) {
    cj += 1;
    while (nproc % cj != 0) cj += 1;
  } else {
    while (nproc % cj != 0) cj += 1;
  }
  cpus[0] = cj; cpus[1] = nproc / cj;
  return 0;
}

int rcmdyn_tile_extent(int32_t jx, int32_t iy, int32_t nproc_j, int32_t nproc_i, int32_t tile, int32_t ext[8],
                       int32_t bdy[4]) {
  if (tile < 0 || tile >= nproc_j * nproc_i) return 1;
  tile_extent(jx, iy, nproc_j, nproc_i, tile, ext, bdy);
  return 0;
}

int rcmdyn_tile_extent_cfg(const rcmdyn_config* cfg, int32_t tile, int32_t ext[8], int32_t bdy[4]) {
  if (!cfg || !ext || !bdy) return 1;
  if (tile < 0 || cfg->nproc_j < 1 || cfg->nproc_i < 1 || tile >= cfg->nproc_j * cfg->nproc_i) return 1;
  if ((cfg->i_band != 0 && cfg->i_band != 1) || (cfg->i_crm != 0 && cfg->i_crm != 1)) return 1;
  if (cfg->i_crm && !cfg->i_band) return 1;              // CRM is built over the band only (create refuses it)
  tile_extent(cfg->jx, cfg->iy, cfg->nproc_j, cfg->nproc_i, tile, ext, bdy, cfg->i_band, cfg->i_crm);
  return 0;
}

int rcmdyn_put(rcmdyn_t* h, int32_t field, const double* src, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
               int32_t k1, int32_t k2) {
  return guard(h, [&] { h->put(field, src, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_get(rcmdyn_t* h, int32_t field, double* dst, int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1,
               int32_t k2) {
  return guard(h, [&] { h->get(field, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_set_time(rcmdyn_t* h, int64_t lcount, double dt, double xbctime) {
  return guard(h, [&] { h->set_time(lcount, dt, xbctime); });
}

int rcmdyn_get_time(rcmdyn_t* h, int64_t* lcount, double* dt, double* xbctime) {
  return guard(h, [&] {
    *lcount = h->hs.lcount; *dt = h->hs.dt; *xbctime = h->hs.xbctime;
  });
}

int rcmdyn_tend(rcmdyn_t* h) { return guard(h, [&] { h->tend_call(); }); }

int rcmdyn_tend_pre_physics(rcmdyn_t* h) { return guard(h, [&] { h->tend_pre_physics(); }); }

int rcmdyn_tend_post_physics(rcmdyn_t* h) { return guard(h, [&] { h->tend_post_physics(); }); }

int rcmdyn_bdyin(rcmdyn_t* h) {
  return guard(h, [&] {
    h->bdyin();
    HIPCHK(hipStreamSynchronize(h->stream));
  });
}

int rcmdyn_bdyval(rcmdyn_t* h) { return guard(h, [&] { h->bdyval_call(); }); }

int rcmdyn_step(rcmdyn_t* h, int32_t nsteps) { return guard(h, [&] { h->step(nsteps); }); }

int rcmdyn_synchronize(rcmdyn_t* h) {
  return guard(h, [&] {
    h->settle();                                     // a deferred step's flags are checked here
    if (h->comm) h->note_step(h->hs.lcount, true);   // collective: every rank synchronizes
    HIPCHK(hipStreamSynchronize(h->stream));
    h->check(0);
  });
}

int rcmdyn_diagnostics(rcmdyn_t* h, double out[4]) { return guard(h, [&] { h->diagnostics(out); }); }

int rcmdyn_reductions(rcmdyn_t* h, double out[3]) { return guard(h, [&] { h->reductions(out); }); }

int rcmdyn_runtime_info(char* buf, int32_t len) {
  try {
    Dl_info info{};
    std::string hip = dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname ? info.dli_fname : "?";
    std::string s = "hip=" + hip + "; rccl=" + rccl_describe();
    if (buf && len > 0) {
      std::strncpy(buf, s.c_str(), (size_t)len - 1);
      buf[len - 1] = 0;
    }
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return 1;
  }
}

int rcmdyn_comm_unique_id(uint8_t out[128]) {
  try {
    comm_unique_id(out);
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return 1;
  }
}

int rcmdyn_last_step_ms(rcmdyn_t* h, double* ms) { return guard(h, [&] { *ms = h->last_ms; }); }

int rcmdyn_set_diagnostics(rcmdyn_t* h, int32_t on) {
  return guard(h, [&] {
    h->quiesce();                                    // a lazy tend replays its graph first
    if (h->diag != (on != 0)) {
      h->diag = (on != 0);
      h->invalidate_graphs();
    }
  });
}

int rcmdyn_set_budget(rcmdyn_t* h, int32_t on, int32_t idgq, double rw) {
  return guard(h, [&] { h->set_budget(on, idgq, rw); });
}

int rcmdyn_get_budget(rcmdyn_t* h, int32_t term, double* dst, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
                      int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_budget(term, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_reset_budget(rcmdyn_t* h) { return guard(h, [&] { h->reset_budget(); }); }

int rcmdyn_set_massck(rcmdyn_t* h, int32_t on, int32_t cap) {
  return guard(h, [&] { h->set_massck(on, cap); });
}

int rcmdyn_get_massck(rcmdyn_t* h, double* out, int32_t cap, int32_t* count, int64_t* lost) {
  return guard(h, [&] { h->get_massck(out, cap, count, lost); });
}

int rcmdyn_set_condtq(rcmdyn_t* h, int32_t on, double conf) {
  return guard(h, [&] { h->set_condtq(on, conf); });
}

int rcmdyn_put_rh0adj(rcmdyn_t* h, const double* src, int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1,
                      int32_t k2) {
  return guard(h, [&] { h->put_rh0adj(src, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_get_condtq(rcmdyn_t* h, int32_t term, double* dst, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
                      int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_condtq(term, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_set_subex(rcmdyn_t* h, int32_t on, double rhmax, double rhmin, double tc0, int32_t larcticcorr, int32_t iconvlwp,
                     int32_t rem, int32_t icldfrac, int32_t icldmstrat, int32_t lsecind) {
  return guard(h, [&] { h->set_subex(on, rhmax, rhmin, tc0, larcticcorr, iconvlwp, rem, icldfrac, icldmstrat, lsecind); });
}

int rcmdyn_put_subex(rcmdyn_t* h, int32_t field, const double* src, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
                     int32_t k1, int32_t k2) {
  return guard(h, [&] { h->put_subex(field, src, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_get_subex(rcmdyn_t* h, int32_t field, double* dst, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
                     int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_subex(field, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_physics_subex(rcmdyn_t* h) { return guard(h, [&] { h->physics_subex(); }); }

int rcmdyn_set_tracers(rcmdyn_t* h, int32_t ntr, int32_t ichebdy) {
  return guard(h, [&] { h->set_tracers(ntr, ichebdy); });
}

int rcmdyn_put_tracer(rcmdyn_t* h, int32_t field, int32_t itr, const double* src, int32_t j1, int32_t j2, int32_t i1,
                      int32_t i2, int32_t k1, int32_t k2) {
  return guard(h, [&] { h->put_tracer(field, itr, src, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_get_tracer(rcmdyn_t* h, int32_t field, int32_t itr, double* dst, int32_t j1, int32_t j2, int32_t i1,
                      int32_t i2, int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_tracer(field, itr, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_put_tracer_nudge(rcmdyn_t* h, const double* cefc, const double* cegc) {
  return guard(h, [&] { h->put_tracer_nudge(cefc, cegc); });
}

int rcmdyn_set_cumtran(rcmdyn_t* h, int32_t on, int32_t ncum) {
  return guard(h, [&] { h->set_cumtran(on, ncum); });
}

int rcmdyn_put_cumtran(rcmdyn_t* h, int32_t field, const double* src, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
                       int32_t k1, int32_t k2) {
  return guard(h, [&] { h->put_cumtran(field, src, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_get_cumtran(rcmdyn_t* h, int32_t field, double* dst, int32_t j1, int32_t j2, int32_t i1, int32_t i2,
                       int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_cumtran(field, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_set_tracer_budget(rcmdyn_t* h, int32_t on, double rw, double cfdout) {
  return guard(h, [&] { h->set_tracer_budget(on, rw, cfdout); });
}

int rcmdyn_get_tracer_budget(rcmdyn_t* h, int32_t term, int32_t itr, double* dst, int32_t j1, int32_t j2, int32_t i1,
                             int32_t i2, int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_tracer_budget(term, itr, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_reset_tracer_budget(rcmdyn_t* h) {
  return guard(h, [&] { h->reset_tracer_budget(); });
}

int rcmdyn_set_output(rcmdyn_t* h, int32_t on, int32_t prec) {
  return guard(h, [&] { h->set_output(on, prec); });
}
int rcmdyn_output_atm(rcmdyn_t* h, uint32_t mask) { return guard(h, [&] { h->output_atm(mask); }); }
int rcmdyn_get_output(rcmdyn_t* h, int32_t field, void* dst, int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1,
                      int32_t k2) {
  return guard(h, [&] { h->get_output(field, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_set_output_che(rcmdyn_t* h, int32_t on, int32_t prec, int32_t nbatch) {
  return guard(h, [&] { h->set_output_che(on, prec, nbatch); });
}
int rcmdyn_output_che(rcmdyn_t* h, uint32_t mask, int32_t itr1, int32_t itr2) {
  return guard(h, [&] { h->output_che(mask, itr1, itr2); });
}
int rcmdyn_get_output_che(rcmdyn_t* h, int32_t field, int32_t itr, void* dst, int32_t j1, int32_t j2, int32_t i1,
                          int32_t i2, int32_t k1, int32_t k2) {
  return guard(h, [&] { h->get_output_che(field, itr, dst, Box{j1, j2, i1, i2, k1, k2}); });
}

int rcmdyn_kernel_times(rcmdyn_t* h, int32_t nsteps, int32_t cap, char* names, int32_t* launches, double* avg_ms,
                        int32_t* count) {
  return guard(h, [&] { h->kernel_times(nsteps, cap, names, launches, avg_ms, count); });
}

}  // extern "C"
