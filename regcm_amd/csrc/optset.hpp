// optset.hpp -- which instance of a hydrostatic tendency kernel a launch takes.  Host only, no
// HIP: the engine includes it, and a stand-alone host program can (tests/test_optset_cpu.py).
//
// k_momentum, k_scalars and k_update are templates on an option policy (kernels.hpp; the
// policies OptGeneric / OptDefault, pointops.hpp): the generic instance reads every model option
// at run time (Consts, the optional pointers of Fields); the default-set instance was compiled
// for the options of the configurations C1-C4 and holds no code, pointer or register of any
// alternative.  The instances with an extra argument block (Budget, Condtq) are generic.  optset_instance() is evaluated where a launch is issued, on the configuration
// and the very pointers that launch passes, so a captured graph holds the instance that matches
// its arguments; attaching the physics seam, the budget, an export or kpbl invalidates the
// graphs (engine.hip) and the next capture selects again.
#pragma once
#include <cstdlib>

namespace rcm {

enum OptInstance { OPT_GENERIC = 0, OPT_DEFAULT = 1 };

// the options of the default set (OptDefault returns these constants)
constexpr int OPT_IBOUDY = 5, OPT_IDIFFU = 1, OPT_IPGF = 0, OPT_ISLADVEC = 0;

// what a launch of the hydrostatic tendency kernels depends on beyond the state
struct OptQuery {
  int iboudy, idiffu, ipgf, isladvec;
  int ibltyp, iuwvadv;                  // ibltyp = 2: xkcs is exported (TKE); with iuwvadv = 1 kpbl is read
  int nqx_extra;                        // hydrometeors beyond qc (nqx = 5): xkcs exported
  bool budget;                          // the budget instances stay generic
  bool no_optset;                       // RCMDYN_NO_OPTSET
  // the optional pointers of the launch's Fields (null: absent)
  const void *tten, *uten, *vten, *qvten, *qcten, *omega, *xkcs;   // exports
  const void *tphy, *qvphy, *qcphy, *uphy, *vphy;                   // physics tendencies of the seam
  const void* kpbl;
  bool condtq;                          // the condtq instances stay generic (rcmdyn_set_condtq)
};

// RCMDYN_NO_OPTSET (present = the generic instances everywhere; Switches::read, engine.hip)
inline bool optset_disabled_by_env() { return std::getenv("RCMDYN_NO_OPTSET") != nullptr; }

inline OptInstance optset_instance(const OptQuery& q) {
  if (q.no_optset || q.budget || q.condtq) return OPT_GENERIC;
  if (q.iboudy != OPT_IBOUDY || q.idiffu != OPT_IDIFFU || q.ipgf != OPT_IPGF || q.isladvec != OPT_ISLADVEC)
    return OPT_GENERIC;
  if (q.ibltyp == 2 || q.nqx_extra > 0) return OPT_GENERIC;
  if (q.tten || q.uten || q.vten || q.qvten || q.qcten || q.omega || q.xkcs) return OPT_GENERIC;
  if (q.tphy || q.qvphy || q.qcphy || q.uphy || q.vphy) return OPT_GENERIC;
  if (q.kpbl) return OPT_GENERIC;
  return OPT_DEFAULT;
}

}  // namespace rcm
