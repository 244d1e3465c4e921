// condtq_point.cpp -- the per-point condtq of regcm_amd/csrc/condtq.hpp on the host: reads rows of
// twelve doubles (t2 qv2 qc2 tt tqv tqc psc pres qs rh0adj dt conf; C99 hexadecimal or decimal)
// from stdin and prints tmp2, wwlh and the three coupled increments of each row in hexadecimal,
// so tests/test_condtq_cpu.py can hold the header to a transcription of the Fortran bit for bit.
// Build: g++ -O2 -ffp-contract=off -std=c++17.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../regcm_amd/csrc/condtq.hpp"

int main() {
  char word[64];
  double v[12];
  int n = 0;
  while (std::scanf("%63s", word) == 1) {
    v[n++] = std::strtod(word, nullptr);
    if (n < 12) continue;
    n = 0;
    double tmp2, wwlh, it, iqv, iqc;
    rcm::condtq_point(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], tmp2, wwlh);
    rcm::condtq_increments(v[6], tmp2, wwlh, it, iqv, iqc);
    std::printf("%a %a %a %a %a\n", tmp2, wwlh, it, iqv, iqc);
  }
  return n == 0 ? 0 : 1;
}
