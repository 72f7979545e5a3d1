// Geometry of a general cell, shared by the one-rank ghost builder (neigh.hip) and the brick decomposition (comm.hip): both must see the very same
// s = x . cell^-1 and the very same m_d = rc / h_d, or an atom on a decision plane would be a ghost for one and not for the other.  Host-compilable (no HIP
// beyond the __device__ / __host__ markers, which vanish without a HIP compiler), so stand-alone CPU programs can include it.
//
// cell rows are lattice vectors, s = x . cell^-1 the fractional coordinates, h_d the cell height along d, m_d = rc / h_d.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

#include "fused_shapes.h"      // ArgError

#if !defined(__HIPCC__) && !defined(__device__)
#define __device__
#define __host__
#endif

namespace ahip {

struct CellGeom {
  double h[9];        // lattice vectors (rows)
  double inv[9];      // cell^-1: s_d = sum_k x_k inv[3 k + d]
  double m[3];        // rc / height (borders only)
  int pbc[3];
};
// explicit fma chain: the count and the fill kernel must see the very same s
__device__ __host__ inline double cell_frac(const CellGeom &g, const double *x, int d) {
  return fma(x[2], g.inv[6 + d], fma(x[1], g.inv[3 + d], x[0] * g.inv[d]));
}
// xi += (the integer lattice combination that brings s_d into [0, 1) on every periodic axis); an atom already inside is not touched
__device__ __host__ inline void cell_wrap_row(const CellGeom &g, double *xi) {
  double k[3];
  for (int d = 0; d < 3; ++d) k[d] = g.pbc[d] ? -floor(cell_frac(g, xi, d)) : 0.0;
  if (k[0] == 0.0 && k[1] == 0.0 && k[2] == 0.0) return;
  for (int d = 0; d < 3; ++d) xi[d] += k[0] * g.h[d] + k[1] * g.h[3 + d] + k[2] * g.h[6 + d];
}
// cell (row-major, rows = lattice vectors), its inverse and rc / height, without an exception: 0, or 1 for a non-finite entry, 2 for a singular cell (g is then
// partly written).  Device code calls it where the host has not seen the cell (neigh.hip: k_vcell_decide)
__device__ __host__ inline int cell_geometry_try(const double *cell, const int *pbc, double rc, CellGeom &g) {
  double scale = 0.0;
  for (int k = 0; k < 9; ++k) {
    if (!std::isfinite(cell[k])) return 1;
    g.h[k] = cell[k];
    const double e = std::fabs(cell[k]);
    scale = scale < e ? e : scale;
  }
  const double *a = g.h, *b = g.h + 3, *c = g.h + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
  if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * scale * scale * scale)) return 2;
  const double *cr[3] = {bc, ca, ab};                      // column d of cell^-1 = (cross product of the other two rows) / det
  for (int d = 0; d < 3; ++d) {
    double nrm = 0.0;
    for (int k = 0; k < 3; ++k) { g.inv[3 * k + d] = cr[d][k] / det; nrm += cr[d][k] * cr[d][k]; }
    g.m[d] = rc * std::sqrt(nrm) / std::fabs(det);         // rc / h_d,  h_d = volume / |cross product|
    g.pbc[d] = pbc[d] != 0;
  }
  return 0;
}
// the same with an ArgError for a singular or non-finite cell
static CellGeom cell_geometry(const char *who, const double *cell, const int *pbc, double rc) {
  CellGeom g;
  switch (cell_geometry_try(cell, pbc, rc, g)) {
    case 1: throw ArgError(std::string(who) + ": the cell has a non-finite entry");
    case 2: throw ArgError(std::string(who) + ": the cell is singular");
  }
  return g;
}

}  // namespace ahip
