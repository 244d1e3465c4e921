// window.hpp -- a host box to or from a staging array: the index arithmetic behind every put and
// get of the engine (engine.hip put_window / get_window, rcmdyn_get_output).  Host only, no HIP:
// the engine includes it, and a stand-alone host program can (tests/test_window_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>

namespace rcm {

// The host's box of global Fortran indices, stored j fastest, then i, then k.
struct Box {
  int j1, j2, i1, i2, k1, k2;
  long nj() const { return (long)j2 - j1 + 1; }
  long ni() const { return (long)i2 - i1 + 1; }
  long nk() const { return (long)k2 - k1 + 1; }
  // what the host array holds: nothing when any extent is inverted
  size_t cells() const {
    return (size_t)std::max(0L, nj()) * (size_t)std::max(0L, ni()) * (size_t)std::max(0L, nk());
  }
  size_t at(int k, int i, int j) const { return ((size_t)(k - k1) * ni() + (i - i1)) * nj() + (j - j1); }
  bool holds(int j, int i) const { return j >= j1 && j <= j2 && i >= i1 && i <= i2; }
};

// A staging array of nk levels: the points j0 .. j0 + nj - 1 x i0 .. i0 + ni - 1, rows of `pitch`
// elements, planes of `plane`, the first point at element `off`.  A tile's frame (Geom::ix, plane)
// and the output stream's compact jci1:jci2 x ici1:ici2 buffer (Tile::ooff) are both one of these.
struct Staging {
  int j0, i0, nj, ni;
  long pitch, plane;
  int nk;
  long off;
  size_t at(int k, int i, int j) const {
    return (size_t)off + (size_t)(k - 1) * plane + (size_t)(i - i0) * pitch + (j - j0);
  }
};

// The global index an array point past either end of a period stands for: a band's columns
// (i_band) and the CRM's rows (i_crm) wrap, any other index is itself.
struct Period {
  int jx, iy;
  bool band, crm;
  int j(int v) const { return !band ? v : (v < 1 ? v + jx : (v > jx ? v - jx : v)); }
  int i(int v) const { return !crm ? v : (v < 1 ? v + iy : (v > iy ? v - iy : v)); }
};

// The box src into the array a: every point of the array whose wrapped global index lies in the
// box, on the levels max(k1, 1) .. min(k2, nk).  A tile's frame so takes its ghost ring and the
// points past either end of a period too.
template <class T>
void scatter(T* a, const Staging& s, const Period& p, const T* src, const Box& b) {
  for (int k = std::max(b.k1, 1); k <= std::min(b.k2, s.nk); k++)
    for (int i = s.i0; i <= s.i0 + s.ni - 1; i++)
      for (int j = s.j0; j <= s.j0 + s.nj - 1; j++)
        if (b.holds(p.j(j), p.i(i))) a[s.at(k, i, j)] = src[b.at(k, p.i(i), p.j(j))];
}

// The other way: the array's points [ja, jb] x [ia, ib] (a tile's owned or interior range) that
// lie in the box, on the same levels, into dst; every other cell of dst stays as it was.
template <class T>
void gather(T* dst, const Box& b, const T* a, const Staging& s, int ja, int jb, int ia, int ib) {
  for (int k = std::max(b.k1, 1); k <= std::min(b.k2, s.nk); k++)
    for (int i = std::max(b.i1, ia); i <= std::min(b.i2, ib); i++)
      for (int j = std::max(b.j1, ja); j <= std::min(b.j2, jb); j++) dst[b.at(k, i, j)] = a[s.at(k, i, j)];
}

}  // namespace rcm
