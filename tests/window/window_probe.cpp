// Runs scatter() and gather() of regcm_amd/csrc/window.hpp on the cases read from standard input
// and prints the resulting arrays, one line per case.  A case is one line of integers after two
// letters:
//   op type  j0 i0 nj ni pitch plane nk off  jx iy band crm  j1 j2 i1 i2 k1 k2  ja jb ia ib
// op: s scatter, g gather; type: d double, f float; then the staging array, the period rule, the
// box, and gather's range of the array's points (scatter ignores it).
//   s: the array of off + nk * plane elements starts as -(e + 1) at element e, the box src holds
//      q + 1 at cell q; prints the array afterwards.
//   g: the array holds e + 1 at element e, the box dst starts as NaN; prints dst afterwards.
// Every buffer is a heap block of exactly its size (src and dst: Box::cells() elements), so the
// address sanitizer stops any read or write past an end.  Host only: no GPU, no HIP header.
#include <cmath>
#include <cstdio>
#include <memory>

#include "../../regcm_amd/csrc/window.hpp"

template <class T>
static void print(const T* v, size_t n) {
  for (size_t q = 0; q < n; q++) std::printf(q ? " %.9g" : "%.9g", (double)v[q]);
  std::printf("\n");
}

template <class T>
static void run(char op, const rcm::Staging& s, const rcm::Period& p, const rcm::Box& b, const int r[4]) {
  const size_t na = (size_t)s.off + (size_t)s.nk * s.plane, nb = b.cells();
  std::unique_ptr<T[]> a(new T[na]), h(new T[nb]);
  if (op == 's') {
    for (size_t e = 0; e < na; e++) a[e] = -(T)(e + 1);
    for (size_t q = 0; q < nb; q++) h[q] = (T)(q + 1);
    rcm::scatter(a.get(), s, p, (const T*)h.get(), b);
    print(a.get(), na);
  } else {
    for (size_t e = 0; e < na; e++) a[e] = (T)(e + 1);
    for (size_t q = 0; q < nb; q++) h[q] = (T)NAN;
    rcm::gather(h.get(), b, (const T*)a.get(), s, r[0], r[1], r[2], r[3]);
    print(h.get(), nb);
  }
}

int main() {
  char op, type;
  while (std::scanf(" %c %c", &op, &type) == 2) {
    long v[22];
    for (long& x : v)
      if (std::scanf("%ld", &x) != 1) return 2;
    const rcm::Staging s{(int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4], v[5], (int)v[6], v[7]};
    const rcm::Period p{(int)v[8], (int)v[9], v[10] != 0, v[11] != 0};
    const rcm::Box b{(int)v[12], (int)v[13], (int)v[14], (int)v[15], (int)v[16], (int)v[17]};
    const int r[4] = {(int)v[18], (int)v[19], (int)v[20], (int)v[21]};
    if (type == 'f') run<float>(op, s, p, b, r);
    else run<double>(op, s, p, b, r);
  }
  return 0;
}
