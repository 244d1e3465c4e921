// Prints the instance id optset_instance() (regcm_amd/csrc/optset.hpp) gives each configuration
// read from standard input, one per line:
//   iboudy idiffu ipgf isladvec ibltyp iuwvadv nqx_extra budget export phys kpbl
// export: 0 none, 1..7 the n-th export pointer (tten, uten, vten, qvten, qcten, omega, xkcs)
// attached; phys: 0 none, 1..5 the n-th physics-tendency pointer (tphy, qvphy, qcphy, uphy,
// vphy); kpbl: 0 / 1.  RCMDYN_NO_OPTSET is read from the environment as the engine reads it.
// Host only: no GPU, no HIP header.
#include <cstdio>

#include "../../regcm_amd/csrc/optset.hpp"

int main() {
  static const double buf = 0.0;     // what an attached pointer points at
  int v[11];
  for (;;) {
    int n = 0;
    while (n < 11 && std::scanf("%d", &v[n]) == 1) n++;
    if (n < 11) break;
    rcm::OptQuery q{};
    q.iboudy = v[0]; q.idiffu = v[1]; q.ipgf = v[2]; q.isladvec = v[3];
    q.ibltyp = v[4]; q.iuwvadv = v[5]; q.nqx_extra = v[6];
    q.budget = v[7] != 0;
    q.no_optset = rcm::optset_disabled_by_env();
    const void** ex[7] = {&q.tten, &q.uten, &q.vten, &q.qvten, &q.qcten, &q.omega, &q.xkcs};
    const void** ph[5] = {&q.tphy, &q.qvphy, &q.qcphy, &q.uphy, &q.vphy};
    if (v[8] >= 1 && v[8] <= 7) *ex[v[8] - 1] = &buf;
    if (v[9] >= 1 && v[9] <= 5) *ph[v[9] - 1] = &buf;
    if (v[10]) q.kpbl = &buf;
    std::printf("%d\n", (int)rcm::optset_instance(q));
  }
  return 0;
}
