// Stand-alone driver helpers: GPU cell-list full neighbor list (the list LAMMPS would hand to the
// pair style: REQ_FULL | REQ_GHOST request of /root/reference/pair_nequip_allegro.cpp:143-147,
// skin-inflated, centres = local atoms, neighbours = locals + ghosts) and the NVE half-steps of the
// test deck's `fix nve` (/root/reference/tests/test_python_repro_allegro.py:84-120).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.h"
#include "prims.h"
#include "cell_geom.h"

namespace ahip {

struct NbState {
  DevBuf bin_of, bin_cnt, bin_start, bin_fill, sorted, cnt, off, nlj, ilist, box, mapper;
  DevBuf goff;                             // ahip_compute_cells: the scanned ghost counts of the batch's atoms (they outlive the list build, which scans into `off`)
  long long cap_j = 0;
  DevBuf inv_mass;                         // nve helpers, more than 16 model types: 1 / mass by model type on the device ...
  std::vector<double> inv_mass_host;       // ... and what it holds (uploaded when it changes)
};

struct BinGrid {
  double lo[3];
  double inv[3];
  int nb[3];
};

__device__ inline int bin_coord(double x, double lo, double inv, int nb) {
  int b = (int)floor((x - lo) * inv);
  return b < 0 ? 0 : (b >= nb ? nb - 1 : b);
}

__global__ void k_bin_count(int nall, const double *x, BinGrid g, int *bin_of, int *bin_cnt) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nall) return;
  int bx = bin_coord(x[3 * i], g.lo[0], g.inv[0], g.nb[0]);
  int by = bin_coord(x[3 * i + 1], g.lo[1], g.inv[1], g.nb[1]);
  int bz = bin_coord(x[3 * i + 2], g.lo[2], g.inv[2], g.nb[2]);
  int b = (bz * g.nb[1] + by) * g.nb[0] + bx;
  bin_of[i] = b;
  atomicAdd(&bin_cnt[b], 1);
}

__global__ void k_bin_fill(int nall, const int *bin_of, const int *bin_start, int *bin_fill, int *sorted) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nall) return;
  int b = bin_of[i];
  int slot = atomicAdd(&bin_fill[b], 1);
  sorted[bin_start[b] + slot] = (int)i;
}

// make the within-bin order deterministic (ascending atom index): insertion sort, bins are small
__global__ void k_bin_sort(int nbins, const int *bin_start, int *sorted) {
  long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbins) return;
  int s = bin_start[b], e = bin_start[b + 1];
  for (int p = s + 1; p < e; ++p) {
    int v = sorted[p], q = p - 1;
    while (q >= s && sorted[q] > v) { sorted[q + 1] = sorted[q]; --q; }
    sorted[q + 1] = v;
  }
}

template <bool FILL>
__global__ void k_neigh_pass(int nlocal, const double *x, BinGrid g, const int *bin_start, const int *sorted,
                             double rcsq, int *cnt, const int *off, int *nlj) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlocal) return;
  double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
  int bx = bin_coord(xi, g.lo[0], g.inv[0], g.nb[0]);
  int by = bin_coord(yi, g.lo[1], g.inv[1], g.nb[1]);
  int bz = bin_coord(zi, g.lo[2], g.inv[2], g.nb[2]);
  int c = 0;
  long long w = FILL ? off[i] : 0;
  for (int dz = -1; dz <= 1; ++dz) {
    int z = bz + dz;
    if (z < 0 || z >= g.nb[2]) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      int y = by + dy;
      if (y < 0 || y >= g.nb[1]) continue;
      int x0 = bx > 0 ? bx - 1 : 0, x1 = bx + 1 < g.nb[0] ? bx + 1 : g.nb[0] - 1;
      int rowbase = (z * g.nb[1] + y) * g.nb[0];
      int s = bin_start[rowbase + x0], e = bin_start[rowbase + x1 + 1];     // x-adjacent bins are contiguous
      for (int p = s; p < e; ++p) {
        int j = sorted[p];
        if (j == (int)i) continue;
        double ddx = x[3 * (long long)j] - xi, ddy = x[3 * (long long)j + 1] - yi, ddz = x[3 * (long long)j + 2] - zi;
        if (ddx * ddx + ddy * ddy + ddz * ddz <= rcsq) {
          if (FILL) nlj[w++] = j;
          ++c;
        }
      }
    }
  }
  if (!FILL) cnt[i] = c;
}

__global__ void k_iota(int n, int *p) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (int)i;
}

// The 32-bit row offsets (like the reference's int edge counters) hold at most 2^31 - 1 list entries.  A wrapped scan total need not be
// negative, so the bound is checked in 64 bits: cheaply through n x longest row, exactly (counts summed on the host) only when that
// bound does not settle it.
static void check_list_total(const int *cnt_dev, int n, int maxrow, hipStream_t s) {
  if ((long long)n * (long long)maxrow <= 2147483647LL) return;
  std::vector<int> h((size_t)n);
  AHIP_CHECK(hipStreamSynchronize(s));
  copy_d2h(h.data(), cnt_dev, (size_t)n * sizeof(int));          // pageable vector: staged (engine.h)
  long long tot = 0;
  for (int v : h) tot += v;
  if (tot > 2147483647LL) throw ArgError("neighbor list: more than 2^31 - 1 entries (row offsets are 32-bit, like the reference's)");
}

void neigh_build(Model &m, int nlocal, int nall, const double *x_dev, const double *lo, const double *hi,
                 double rc_list, hipStream_t s) {
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  BinGrid g;
  long long nbins = 1;
  for (int d = 0; d < 3; ++d) {
    double len = hi[d] - lo[d];
    if (!(len > 0)) throw ArgError("ahip_build_neighbors_dev: empty bounding box");
    int nb = (int)std::floor(len / rc_list);
    if (nb < 1) nb = 1;
    if (nb > 1024) nb = 1024;
    g.nb[d] = nb; g.lo[d] = lo[d]; g.inv[d] = nb / len;
    nbins *= nb;
  }
  const unsigned B = 256;
  auto grid = [&](long long n) { return dim3((unsigned)((n + B - 1) / B)); };
  st.bin_of.reserve((size_t)std::max(nall, 1) * sizeof(int));
  st.bin_cnt.reserve((size_t)(nbins + 1) * sizeof(int));
  st.bin_start.reserve((size_t)(nbins + 2) * sizeof(int));
  st.bin_fill.reserve((size_t)(nbins + 1) * sizeof(int));
  st.sorted.reserve((size_t)std::max(nall, 1) * sizeof(int));
  st.cnt.reserve((size_t)(nlocal + 1) * sizeof(int));
  st.off.reserve((size_t)(nlocal + 2) * sizeof(int));
  st.ilist.reserve((size_t)std::max(nlocal, 1) * sizeof(int));
  AHIP_CHECK(hipMemsetAsync(st.bin_cnt.p, 0, (size_t)(nbins + 1) * sizeof(int), s));
  AHIP_CHECK(hipMemsetAsync(st.bin_fill.p, 0, (size_t)(nbins + 1) * sizeof(int), s));
  if (nall > 0) hipLaunchKernelGGL(k_bin_count, grid(nall), dim3(B), 0, s, nall, x_dev, g, st.bin_of.as<int>(), st.bin_cnt.as<int>());
  AHIP_CHECK(prim_exclusive_scan_i32(m.prim, st.bin_cnt.as<int>(), st.bin_start.as<int>(), (int)nbins, s));
  if (nall > 0) hipLaunchKernelGGL(k_bin_fill, grid(nall), dim3(B), 0, s, nall, st.bin_of.as<int>(), st.bin_start.as<int>(), st.bin_fill.as<int>(), st.sorted.as<int>());
  hipLaunchKernelGGL(k_bin_sort, grid(nbins), dim3(B), 0, s, (int)nbins, st.bin_start.as<int>(), st.sorted.as<int>());
  const double rcsq = rc_list * rc_list;
  if (nlocal > 0) {
    hipLaunchKernelGGL(k_neigh_pass<false>, grid(nlocal), dim3(B), 0, s, nlocal, x_dev, g, st.bin_start.as<int>(), st.sorted.as<int>(), rcsq, st.cnt.as<int>(), (const int *)nullptr, (int *)nullptr);
    hipLaunchKernelGGL(k_iota, grid(nlocal), dim3(B), 0, s, nlocal, st.ilist.as<int>());
  }
  AHIP_CHECK(prim_exclusive_scan_i32(m.prim, st.cnt.as<int>(), st.off.as<int>(), nlocal, s));
  int tot = 0, maxrow = 0;
  st.box.reserve(64);
  AHIP_CHECK(prim_max_i32(st.cnt.as<int>(), nlocal, st.box.as<int>(), s));
  AHIP_CHECK(hipMemcpyAsync(&tot, st.off.as<int>() + nlocal, sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipMemcpyAsync(&maxrow, st.box.as<int>(), sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  check_list_total(st.cnt.as<int>(), nlocal, maxrow, s);
  st.nlj.reserve((size_t)std::max(tot, 1) * sizeof(int));
  if (nlocal > 0)
    hipLaunchKernelGGL(k_neigh_pass<true>, grid(nlocal), dim3(B), 0, s, nlocal, x_dev, g, st.bin_start.as<int>(), st.sorted.as<int>(), rcsq, (int *)nullptr, st.off.as<int>(), st.nlj.as<int>());
  AHIP_CHECK(hipGetLastError());
  m.d_ilist = st.ilist.as<int>();
  m.d_nloff = st.off.as<int>();
  m.d_nlj = st.nlj.as<int>();
  m.inum = nlocal; m.nall = nall; m.nneigh = tot; m.have_list = true;
  ++m.list_serial;
  m.max_list_row = maxrow;
  m.h_ilist.clear();
}

// ---------------------------------------------------------------- device-resident LAMMPS list (KOKKOS package layout)
// The KOKKOS package keeps the full list as a padded 2-D table d_neighbors(i, jj) (column-major on a GPU build) with
// d_numneigh[i] valid entries per ATOM index (pair_nequip_allegro_kokkos.cpp:128-131,157-163 reads exactly these).  On a
// rebuild step it is compacted once into the CSR rows every later evaluation walks; the reference instead re-filters the whole
// table every step into a second padded table (:142-181).
__global__ void k_table_counts(int inum, int nall, const int *ilist, const int *numneigh, int *cnt, int *ilist_out, int *bad) {
  long long ii = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ii >= inum) return;
  const int i = ilist[ii];
  if (i < 0 || i >= nall) { atomicMax(bad, 1); cnt[ii] = 0; ilist_out[ii] = 0; return; }
  const int n = numneigh[i];
  if (n < 0) atomicMax(bad, 2);
  cnt[ii] = n < 0 ? 0 : n;
  ilist_out[ii] = i;
}
__global__ void k_table_rows(int inum, int nall, const int *ilist, const int *cnt, const int *off, const int *table, long long stride_atom,
                             long long stride_slot, int mask, int *nlj, int *bad) {
  long long ii = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ii >= inum) return;
  const int i = ilist[ii], n = cnt[ii];
  const int *row = table + (long long)i * stride_atom;
  int *dst = nlj + off[ii];
  for (int jj = 0; jj < n; ++jj) {
    const int j = row[jj * stride_slot] & mask;
    if (j < 0 || j >= nall) atomicMax(bad, 3);
    dst[jj] = j;
  }
}

void neigh_from_table(Model &m, int inum, int nall, const int *ilist_dev, const int *numneigh_dev, const int *table_dev,
                      long long stride_atom, long long stride_slot, int mask, hipStream_t s) {
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  const unsigned B = 256;
  auto grid = [&](long long n) { return dim3((unsigned)((n + B - 1) / B)); };
  st.cnt.reserve((size_t)(inum + 1) * sizeof(int));
  st.off.reserve((size_t)(inum + 2) * sizeof(int));
  st.ilist.reserve((size_t)std::max(inum, 1) * sizeof(int));
  st.box.reserve(64);
  int *bad = st.box.as<int>() + 1;
  AHIP_CHECK(hipMemsetAsync(st.box.p, 0, 64, s));
  if (inum > 0)
    hipLaunchKernelGGL(k_table_counts, grid(inum), dim3(B), 0, s, inum, nall, ilist_dev, numneigh_dev, st.cnt.as<int>(), st.ilist.as<int>(), bad);
  AHIP_CHECK(prim_exclusive_scan_i32(m.prim, st.cnt.as<int>(), st.off.as<int>(), inum, s));
  AHIP_CHECK(prim_max_i32(st.cnt.as<int>(), inum, st.box.as<int>(), s));
  int tot = 0, hb[2] = {0, 0};
  AHIP_CHECK(hipMemcpyAsync(&tot, st.off.as<int>() + inum, sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipMemcpyAsync(hb, st.box.as<int>(), 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  if (hb[1] == 1) throw ArgError("neighbor list: ilist entry out of range");
  if (hb[1] == 2) throw ArgError("neighbor list: negative numneigh");
  check_list_total(st.cnt.as<int>(), inum, hb[0], s);
  st.nlj.reserve((size_t)std::max(tot, 1) * sizeof(int));
  if (inum > 0)
    hipLaunchKernelGGL(k_table_rows, grid(inum), dim3(B), 0, s, inum, nall, st.ilist.as<int>(), st.cnt.as<int>(), st.off.as<int>(), table_dev, stride_atom,
                       stride_slot, mask, st.nlj.as<int>(), bad);
  AHIP_CHECK(hipMemcpyAsync(hb, st.box.as<int>(), 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  if (hb[1] == 3) throw ArgError("neighbor list: neighbour index out of range");
  m.d_ilist = st.ilist.as<int>();
  m.d_nloff = st.off.as<int>();
  m.d_nlj = st.nlj.as<int>();
  m.inum = inum; m.nall = nall; m.nneigh = tot; m.have_list = true;
  ++m.list_serial;
  m.max_list_row = hb[0];
  m.h_ilist.clear();
}

// LAMMPS types (1-based) -> model types through the pair_coeff mapping (pair_nequip_allegro_kokkos.cpp:222-223 does this every
// step; the types of an atom index only change when the list is rebuilt, so callers do it on those steps).
__global__ void k_map_types(int n, const int *type, int ntypes, const int *mapper, int nmodel, int *out, int *bad) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = type[i];
  int mt = (t >= 1 && t <= ntypes) ? mapper[t - 1] : -2;
  if (mt < 0 || mt >= nmodel) { atomicMax(bad, mt == -2 ? 2 : 1); mt = 0; }
  out[i] = mt;
}
void map_types(Model &m, int n, const int *type_dev, int ntypes, const int *mapper_host, int *out_dev, hipStream_t s) {
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  st.mapper.reserve((size_t)std::max(ntypes, 1) * sizeof(int) + 64);
  int *bad = st.mapper.as<int>() + ntypes;
  AHIP_CHECK(hipMemcpyAsync(st.mapper.p, mapper_host, (size_t)ntypes * sizeof(int), hipMemcpyHostToDevice, s));
  AHIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
  AHIP_CHECK(hipStreamSynchronize(s));                        // mapper_host may be a temporary
  if (n > 0) hipLaunchKernelGGL(k_map_types, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, type_dev, ntypes, st.mapper.as<int>(), m.hm.num_types, out_dev, bad);
  int hb = 0;
  AHIP_CHECK(hipMemcpyAsync(&hb, bad, sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  if (hb == 2) throw ArgError("ahip_map_types_dev: atom type out of range");
  if (hb == 1) throw ArgError("ahip_map_types_dev: an atom has a LAMMPS type that is not mapped to a model type (all pair coeffs are not set)");
}

// ---- ghost atoms of a single rank: the periodic images of its own atoms inside the halo (stand-alone driver, `borders` at a re-neighboring) ----
// LAMMPS builds them swap by swap (x, then y over what x produced, then z): for one rank owning the whole periodic box the result is every image
// (s_x, s_y, s_z) != 0 of an atom with s_d = +1 allowed iff x_d < lo_d + rc and s_d = -1 iff x_d >= hi_d - rc.  The driver's torch version is six
// rounds of mask / nonzero / gather / cat (0.8 of the 1.9 ms a re-neighboring of 10 648 atoms costs, every 16 steps at 300 K); this is a count, a scan and a
// fill.  Ghost k of atom i: position x_i + s * box, type of i, source index i, shift s * box -- what ahip_comm_set_plan_local takes.
struct BorderBox { double lo[3], hi[3], box[3], rc; };
__device__ __host__ inline int border_dirs(double xd, double lo, double hi, double rc, int *sgn) {      // shifts available along one dimension, besides 0
  int n = 0;
  if (xd < lo + rc) sgn[n++] = 1;
  if (xd >= hi - rc) sgn[n++] = -1;
  return n;
}
__global__ void k_border_count(int n, const double *x, BorderBox bb, int *cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int sg[2], tot = 1;
  for (int d = 0; d < 3; ++d) tot *= 1 + border_dirs(x[3 * (size_t)i + d], bb.lo[d], bb.hi[d], bb.rc, sg);
  cnt[i] = tot - 1;
}
__global__ void k_border_fill(int n, const double *x, const int *mtype, BorderBox bb, const int *off, int capacity, double *xg, int *mtg, long long *src, double *shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int sg[3][3], nd[3];
  for (int d = 0; d < 3; ++d) { sg[d][0] = 0; nd[d] = 1 + border_dirs(x[3 * (size_t)i + d], bb.lo[d], bb.hi[d], bb.rc, &sg[d][1]); }
  int k = off[i];
  for (int a = 0; a < nd[0]; ++a)
    for (int b = 0; b < nd[1]; ++b)
      for (int c = 0; c < nd[2]; ++c) {
        if (a == 0 && b == 0 && c == 0) continue;
        if (k < capacity) {
          const double sh[3] = {sg[0][a] * bb.box[0], sg[1][b] * bb.box[1], sg[2][c] * bb.box[2]};
          for (int d = 0; d < 3; ++d) { xg[3 * (size_t)k + d] = x[3 * (size_t)i + d] + sh[d]; shift[3 * (size_t)k + d] = sh[d]; }
          mtg[k] = mtype[i];
          src[k] = i;
        }
        ++k;
      }
}
int borders_local(Model &m, int nlocal, const double *x, const int *mtype, const double *lo, const double *hi, const double *box, double rc, int capacity,
                  double *xg, int *mtg, long long *src, double *shift, hipStream_t s) {
  if (nlocal <= 0) return 0;
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  BorderBox bb;
  for (int d = 0; d < 3; ++d) {
    bb.lo[d] = lo[d]; bb.hi[d] = hi[d]; bb.box[d] = box[d];
    if (!(box[d] >= rc)) throw ArgError("ahip_borders_local_dev: the box is thinner than the halo (one image per direction and dimension only)");
  }
  bb.rc = rc;
  st.cnt.reserve(((size_t)nlocal + 1) * sizeof(int));
  st.off.reserve(((size_t)nlocal + 2) * sizeof(int));
  ++m.list_serial;        // (st.off also carries the row offsets of a list built by neigh_build: a hold on that list ends here)
  const unsigned B = 256, G = (unsigned)((nlocal + B - 1) / B);
  hipLaunchKernelGGL(k_border_count, dim3(G), dim3(B), 0, s, nlocal, x, bb, st.cnt.as<int>());
  AHIP_CHECK(prim_exclusive_scan_i32(m.prim, st.cnt.as<int>(), st.off.as<int>(), nlocal, s));
  int tot = 0;
  AHIP_CHECK(hipMemcpyAsync(&tot, st.off.as<int>() + nlocal, sizeof(int), hipMemcpyDeviceToHost, s));
  hipLaunchKernelGGL(k_border_fill, dim3(G), dim3(B), 0, s, nlocal, x, mtype, bb, st.off.as<int>(), capacity, xg, mtg, src, shift);
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  return tot;             // > capacity: nothing beyond the capacity was written; the caller retries with larger arrays
}

// ---- any periodic cell: wrap (LAMMPS' Domain::remap) and the ghost shell of one rank (Comm::borders on a 1 x 1 x 1 grid of a triclinic or thin box) ----
// cell rows are lattice vectors, s = x . cell^-1 the fractional coordinates, h_d the cell height along d, m_d = rc / h_d.  The image n = (n1, n2, n3) != 0 of
// atom i is a ghost iff for every d: n_d == 0 where the axis is open, -m_d <= s_id + n_d < 1 + m_d where it is periodic -- LAMMPS' slab criterion in fractional
// coordinates.  It is complete (every j + n . cell within rc of a wrapped atom satisfies it), reduces to the rule of border_dirs on an orthogonal box with
// box_d >= rc, and allows any number of images per direction (a 3.61 A cell at rc = 16 has 856 per atom).
// The admissible n_d are an integer interval [lo_d, hi_d], so the count is closed-form per atom; the fill runs one thread per OUTPUT row (a thread per atom would
// serialise 856 images on four lanes): binary search of the scanned offsets for the source atom, n decoded from the rank inside the atom's image box, n3 fastest,
// the zero image skipped.  Order: ascending source atom, then (n1, n2, n3) lexicographic.
// CellGeom, cell_frac, cell_wrap_row and cell_geometry live in cell_geom.h: the brick decomposition (comm.hip) decides with the same s and the same m_d.
__device__ __host__ inline int cell_clamp_int(double v) { return v < -1073741824.0 ? -1073741824 : (v > 1073741824.0 ? 1073741824 : (int)v); }
// images admitted along d: lo <= n_d <= hi (an open axis: 0 only); returns their number
__device__ __host__ inline int cell_image_range(const CellGeom &g, const double *x, int d, int *lo) {
  if (!g.pbc[d]) { *lo = 0; return 1; }
  const double s = cell_frac(g, x, d);
  const int l = cell_clamp_int(ceil(-g.m[d] - s)), h = cell_clamp_int(ceil(1.0 + g.m[d] - s)) - 1;      // -m <= s + n  and  s + n < 1 + m
  *lo = l;
  return h >= l ? h - l + 1 : 0;
}
// the image box of one atom: lo[3], count[3]; returns the number of ghosts (the box without the zero image) and the rank `zero` of that image in it (-1: outside)
__device__ __host__ inline long long cell_image_box(const CellGeom &g, const double *x, int *lo, int *c, long long *zero) {
  for (int d = 0; d < 3; ++d) c[d] = cell_image_range(g, x, d, &lo[d]);
  const long long tot = (long long)c[0] * c[1] * c[2];
  bool in = tot > 0;
  for (int d = 0; d < 3; ++d) in = in && lo[d] <= 0 && -lo[d] < c[d];
  *zero = in ? ((long long)(-lo[0]) * c[1] + (-lo[1])) * c[2] + (-lo[2]) : -1;
  return in ? tot - 1 : tot;
}
// The three per-row bodies below serve the single-cell kernels (geometry in the kernel arguments) and the batch kernels (geometry looked up per atom) alike,
// so the two paths cannot drift apart.
// ghosts of one atom, saturated to 32 bits (the host has bounded the sum for wrapped input; a far-away atom saturates instead of wrapping)
__device__ inline int cell_count_row(const CellGeom &g, const double *xi) {
  int lo[3], c[3];
  long long zero;
  const long long k = cell_image_box(g, xi, lo, c, &zero);
  return k > 2147483647LL ? 2147483647 : (int)k;
}
// ghost number `r` of the atom at xi (its rank among the atom's ghosts, n3 fastest, the zero image skipped) -> output row k; false when the atom has none
__device__ inline bool cell_fill_row(const CellGeom &g, const double *xi, long long r, long long k, double *xg, double *shift) {
  int lo[3], c[3];
  long long zero;
  if (cell_image_box(g, xi, lo, c, &zero) <= 0) return false;    // (cannot happen behind a consistent scan: no row belongs to an atom without images)
  if (zero >= 0 && r >= zero) ++r;
  const int n3 = lo[2] + (int)(r % c[2]);
  r /= c[2];
  const int n2 = lo[1] + (int)(r % c[1]), n1 = lo[0] + (int)(r / c[1]);
  for (int d = 0; d < 3; ++d) {
    const double sh = n1 * g.h[d] + n2 * g.h[3 + d] + n3 * g.h[6 + d];
    shift[3 * k + d] = sh;
    xg[3 * k + d] = xi[d] + sh;
  }
  return true;
}
// largest a in [0, n) with off[a] <= k, for 0 <= k < off[n]: the source atom of output row k
__device__ inline int cell_row_atom(const int *off, int n, long long k) {
  int a = 0, b = n;                                       // (off[a] <= k < off[b] throughout)
  while (b - a > 1) {
    const int mid = a + (b - a) / 2;
    if (off[mid] <= (int)k) a = mid; else b = mid;
  }
  return a;
}
__global__ void k_cell_count(int n, const double *x, CellGeom g, int *cnt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cnt[i] = cell_count_row(g, x + 3 * i);
}
__global__ void k_cell_fill(int n, const double *x, const int *mtype, CellGeom g, const int *off, int capacity, double *xg, int *mtg, long long *src, double *shift) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= capacity || k >= off[n]) return;
  const int a = cell_row_atom(off, n, k);
  if (!cell_fill_row(g, x + 3 * (long long)a, k - off[a], k, xg, shift)) return;
  mtg[k] = mtype[a];
  src[k] = a;
}
__global__ void k_cell_wrap(int n, double *x, CellGeom g) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cell_wrap_row(g, x + 3 * i);
}
// images of n wrapped atoms: at most 2 ceil(m_d) + 1 each along a periodic axis
static double cell_most_images(const CellGeom &g, int n) {
  double most = (double)n;
  for (int d = 0; d < 3; ++d) if (g.pbc[d]) most *= 2.0 * std::ceil(g.m[d]) + 1.0;
  return most;
}
void wrap_cell(Model &m, int n, double *x, const double *cell, const int *pbc, hipStream_t s) {
  const CellGeom g = cell_geometry("ahip_wrap_cell_dev", cell, pbc, 0.0);
  if (n <= 0) return;
  hipLaunchKernelGGL(k_cell_wrap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, x, g);
  AHIP_CHECK(hipGetLastError());
}
int borders_cell(Model &m, int nlocal, const double *x, const int *mtype, const double *cell, const int *pbc, double rc, int capacity,
                 double *xg, int *mtg, long long *src, double *shift, hipStream_t s) {
  const CellGeom g = cell_geometry("ahip_borders_cell_dev", cell, pbc, rc);
  const double most = cell_most_images(g, nlocal);
  if (!(most <= 2147483647.0)) throw ArgError("ahip_borders_cell_dev: nlocal x images per atom exceeds 2^31 - 1 (the offsets are 32-bit); the cell is too thin for this cutoff");
  if (nlocal <= 0) return 0;
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  st.cnt.reserve(((size_t)nlocal + 1) * sizeof(int));
  st.off.reserve(((size_t)nlocal + 2) * sizeof(int));
  ++m.list_serial;        // (as in borders_local: the scan below overwrites the offsets of a list built by neigh_build)
  const unsigned B = 256;
  hipLaunchKernelGGL(k_cell_count, dim3((unsigned)((nlocal + B - 1) / B)), dim3(B), 0, s, nlocal, x, g, st.cnt.as<int>());
  AHIP_CHECK(prim_exclusive_scan_i32(m.prim, st.cnt.as<int>(), st.off.as<int>(), nlocal, s));
  int tot = 0;
  AHIP_CHECK(hipMemcpyAsync(&tot, st.off.as<int>() + nlocal, sizeof(int), hipMemcpyDeviceToHost, s));
  // one thread per row the caller has room for; the threads beyond the total (known on the device only, so far) leave at once
  if (capacity > 0)
    hipLaunchKernelGGL(k_cell_fill, dim3((unsigned)(((long long)capacity + B - 1) / B)), dim3(B), 0, s, nlocal, x, mtype, g, st.off.as<int>(), capacity, xg, mtg, src, shift);
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  if (tot < 0) throw ArgError("ahip_borders_cell_dev: more than 2^31 - 1 images (positions far outside the cell: wrap them first)");
  return tot;             // > capacity: nothing beyond the capacity was written; the caller retries with larger arrays
}
// bounding box of the cell's eight corners, widened by `margin`: what the list build bins over (a ghost outside it is farther than the margin from the cell in
// one coordinate, hence nobody's neighbour; bin_coord clamps it into an edge bin)
void cell_bounding_box(const double *cell, double margin, double *lo, double *hi) {
  for (int d = 0; d < 3; ++d) {
    double l = 0.0, h = 0.0;
    for (int k = 0; k < 3; ++k) { l += std::min(cell[3 * k + d], 0.0); h += std::max(cell[3 * k + d], 0.0); }
    lo[d] = l - margin; hi[d] = h + margin;
  }
}

// ---- the held list of ahip_compute_cell_reuse ----
// At a rebuild the model keeps, beside the rows and the list: the cell A0, the wrapped atom positions xhold and, per ghost, its integer image n.  A later call
// with positions x and cell A rewrites EVERY row as an exact periodic image in A of the new position: atom a moves by the lattice combination k that brings it
// nearest to where it was held (the caller may have wrapped it in between), ghost (a, n) follows as x_a - k A + n A.  Whether the held list still serves is
// decided on the host from the largest displacement (criterion and proof: include/allegro_hip.h).
__device__ __host__ inline int float_bits(float v) {
  int b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}
// n = round(shift . A0^-1): the shifts are n . A0 to rounding and n is a small integer, so the nearest integer is n itself
__global__ void k_cell_images(int nghost, const double *shift, CellGeom g, int *img) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nghost) return;
  for (int d = 0; d < 3; ++d) img[3 * k + d] = (int)rint(cell_frac(g, shift + 3 * k, d));
}
// one thread per row (atoms, then ghosts); g is the cell of THIS call.  disp[a]: float32 bit pattern of |x_a - k A - xhold_a|^2 rounded up (as k_disp_max
// rounds), 0x7fffffff when it is not finite -- non-negative floats order like their bit patterns, so prim_max_i32 finds the largest
__global__ void k_cell_refresh(int natoms, int nrows, const double *xin, const double *xhold, const long long *src, const int *img, CellGeom g, double *x, int *disp) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  const long long a = r < natoms ? r : src[r - natoms];
  const double dx[3] = {xin[3 * a] - xhold[3 * a], xin[3 * a + 1] - xhold[3 * a + 1], xin[3 * a + 2] - xhold[3 * a + 2]};
  double c[3];                               // the row is x_a + c . A
  for (int d = 0; d < 3; ++d) c[d] = g.pbc[d] ? -floor(cell_frac(g, dx, d) + 0.5) : 0.0;
  if (r < natoms) {
    double u2 = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double u = dx[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
      u2 += u * u;
    }
    const float v = (float)u2 * 1.000001f;   // rounded up: the criterion must not miss
    disp[r] = v >= 0.f && v <= 3.0e38f ? float_bits(v) : 0x7fffffff;
  } else {
    for (int d = 0; d < 3; ++d) c[d] += (double)img[3 * (r - natoms) + d];
  }
  for (int d = 0; d < 3; ++d) x[3 * r + d] = xin[3 * a + d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
}
void cell_hold_take(Model &m, int natoms, int nghost, const double *cell, const int *pbc, double skin, double rc, hipStream_t s) {
  const CellGeom g = cell_geometry("ahip_compute_cell_reuse", cell, pbc, rc);
  Model::CellHold &h = m.hold;
  h.natoms = natoms; h.nghost = nghost; h.skin = skin;
  h.min_height = INFINITY;
  for (int d = 0; d < 3; ++d) {
    h.pbc[d] = g.pbc[d];
    h.images[d] = std::ceil(g.m[d]) + 1.0;                 // M_d = ceil(rc / h0_d) + 1
    if (g.pbc[d]) h.min_height = std::min(h.min_height, rc / g.m[d]);
  }
  std::copy(cell, cell + 9, h.cell);
  m.r_xhold.reserve((size_t)std::max(natoms, 1) * 3 * sizeof(double));
  m.r_img.reserve((size_t)std::max(nghost, 1) * 3 * sizeof(int));
  if (natoms > 0) AHIP_CHECK(hipMemcpyAsync(m.r_xhold.p, m.c_x.p, (size_t)natoms * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (nghost > 0) hipLaunchKernelGGL(k_cell_images, dim3((unsigned)((nghost + 255) / 256)), dim3(256), 0, s, nghost, m.c_shift.as<double>(), g, m.r_img.as<int>());
  AHIP_CHECK(hipGetLastError());
}
bool cell_hold_refresh(Model &m, const double *x_host, const double *cell, hipStream_t s) {
  const Model::CellHold &h = m.hold;
  const CellGeom g = cell_geometry("ahip_compute_cell_reuse", cell, h.pbc, 0.0);
  double sum_g = 0.0, sum_mg = 0.0;          // over the periodic axes: g_d = |a_d - a0_d|
  for (int d = 0; d < 3; ++d) {
    if (!h.pbc[d]) continue;
    double q = 0.0;
    for (int k = 0; k < 3; ++k) { const double e = cell[3 * d + k] - h.cell[3 * d + k]; q += e * e; }
    sum_g += std::sqrt(q);
    sum_mg += h.images[d] * std::sqrt(q);
  }
  if (!(sum_g <= h.min_height) || !(sum_mg <= h.skin)) return false;
  const int natoms = h.natoms, nrows = h.natoms + h.nghost;
  if (natoms == 0) return true;
  m.r_xin.reserve((size_t)natoms * 3 * sizeof(double));
  m.r_disp.reserve(((size_t)natoms + 1) * sizeof(int));
  copy_h2d(m.r_xin.p, x_host, (size_t)natoms * 3 * sizeof(double));
  int *disp = m.r_disp.as<int>(), umax = 0;
  hipLaunchKernelGGL(k_cell_refresh, dim3((unsigned)(((long long)nrows + 255) / 256)), dim3(256), 0, s, natoms, nrows, m.r_xin.as<double>(), m.r_xhold.as<double>(),
                     m.c_src.as<long long>(), m.r_img.as<int>(), g, m.c_x.as<double>(), disp);
  AHIP_CHECK(prim_max_i32(disp, natoms, disp + natoms, s));
  AHIP_CHECK(hipMemcpyAsync(&umax, disp + natoms, sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  if (umax == 0x7fffffff) return false;      // a position that is not finite: the rebuild path treats it as ahip_compute_cell does
  float u2;
  std::memcpy(&u2, &umax, sizeof(u2));
  return 2.0 * std::sqrt((double)u2) + sum_mg <= h.skin;
}

// ---- FIRE with its state on the device (ahip_relax_cell; the algorithm is stated in include/allegro_hip.h) ----
// Per move: k_relax_gather (one thread per atom), the column sums and the two maxima through prims, k_relax_decide (one thread, the only writer of the state),
// k_relax_move (one thread per row).  Once the status is not RUNNING all three return at once, so the positions, the rows and the state stay those of the
// last decision while the host has not looked.  No kernel here needs a barrier.
__global__ void k_relax_gather(int natoms, const double *f, const double *v, const int *fixed, const RelaxState *st, double *part, int *fbits) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= natoms || st->status != RELAX_RUNNING) return;
  double vf = 0.0, ff = 0.0, vv = 0.0;
  if (!(fixed && fixed[i]))
    for (int d = 0; d < 3; ++d) {
      const double fd = f[3 * i + d], vd = v[3 * i + d];
      vf += vd * fd; ff += fd * fd; vv += vd * vd;
    }
  part[3 * i] = vf; part[3 * i + 1] = ff; part[3 * i + 2] = vv;
  const float q = (float)ff;                 // non-negative floats order like their bit patterns (k_cell_refresh)
  fbits[i] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
}
__device__ __host__ inline float bits_float(int b) {
  float v;
  __builtin_memcpy(&v, &b, sizeof(v));
  return v;
}
__global__ void k_relax_decide(RelaxState *st, RelaxFire p) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || st->status != RELAX_RUNNING) return;
  const double vf = st->sums[0], ff = st->sums[1], vv = st->sums[2];
  const double u2 = (double)bits_float(st->ubits), f2 = (double)bits_float(st->fbits);
  st->u2 = u2; st->fmax2 = f2;
  if (st->ubits == 0x7fffffff) { st->status = RELAX_NONFINITE; return; }
  if (2.0 * sqrt(u2) > p.skin) { st->status = RELAX_NEED_REBUILD; return; }
  if (st->fbits == 0x7fffffff || !isfinite(vf) || !isfinite(ff) || !isfinite(vv)) { st->status = RELAX_NONFINITE; return; }
  if (sqrt(f2) <= p.fmax) { st->status = RELAX_CONVERGED; return; }
  double dt = st->dt, c1, c2;
  if (vf > 0.0) {
    c1 = 1.0 - st->alpha;
    c2 = st->alpha * sqrt(vv / ff);
    if (st->npos > p.n_min) {
      dt = fmin(dt * p.f_inc, p.dt_max);
      st->alpha *= p.f_alpha;
    }
    st->npos += 1;
  } else {
    c1 = c2 = 0.0;
    st->alpha = p.alpha_start;
    dt *= p.f_dec;
    st->npos = 0;
  }
  // |dr|^2 = |dt v'|^2 with v' = c1 v + (c2 + dt) F, expanded in the three sums: no second pass over the atoms
  const double k = c2 + dt, dr = dt * sqrt(fmax(c1 * c1 * vv + 2.0 * c1 * k * vf + k * k * ff, 0.0));
  st->dt = dt; st->c1 = c1; st->c2 = c2;
  st->s = dr > p.max_step ? p.max_step / dr : 1.0;
  st->moves += 1;
}
// x' and v' of the row's source atom from the buffers of the move before, the row as k_cell_refresh writes it; atom rows also store x', v' and the
// displacement bits.  xin / vin are never written by this launch.
__global__ void k_relax_move(int natoms, int nrows, const RelaxState *st, const double *xin, const double *vin, const double *f, const int *fixed,
                             const double *xhold, const long long *src, const int *img, CellGeom g, double *xout, double *vout, double *x, int *disp) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows || st->status != RELAX_RUNNING) return;
  const long long a = r < natoms ? r : src[r - natoms];
  const bool fix = fixed && fixed[a];
  const double c1 = st->c1, k = st->c2 + st->dt, sdt = st->s * st->dt;
  double xn[3], vn[3], dx[3];
  for (int d = 0; d < 3; ++d) {
    vn[d] = fix ? 0.0 : c1 * vin[3 * a + d] + k * f[3 * a + d];
    xn[d] = fix ? xin[3 * a + d] : xin[3 * a + d] + sdt * vn[d];
    dx[d] = xn[d] - xhold[3 * a + d];
  }
  double c[3];                               // the row is x'_a + c . A
  for (int d = 0; d < 3; ++d) c[d] = g.pbc[d] ? -floor(cell_frac(g, dx, d) + 0.5) : 0.0;
  if (r < natoms) {
    double u2 = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double u = dx[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
      u2 += u * u;
      xout[3 * r + d] = xn[d]; vout[3 * r + d] = vn[d];
    }
    const float q = (float)u2 * 1.000001f;   // rounded up: the criterion must not miss
    disp[r] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
  } else {
    for (int d = 0; d < 3; ++d) c[d] += (double)img[3 * (r - natoms) + d];
  }
  for (int d = 0; d < 3; ++d) x[3 * r + d] = xn[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
}
void relax_begin(Model &m, int natoms, const double *x_host, const int *fixed_host, double dt_start, double alpha_start, hipStream_t s) {
  const size_t n = (size_t)std::max(natoms, 1);
  for (int k = 0; k < 2; ++k) { m.q_x[k].reserve(n * 3 * sizeof(double)); m.q_v[k].reserve(n * 3 * sizeof(double)); }
  m.q_part.reserve(n * 3 * sizeof(double));
  m.q_fbits.reserve(n * sizeof(int));
  m.q_state.reserve(sizeof(RelaxState));
  m.q_fixed.release();                       // no mask: the kernels take a null pointer
  if (natoms > 0) {
    copy_h2d(m.q_x[0].p, x_host, (size_t)natoms * 3 * sizeof(double));
    AHIP_CHECK(hipMemsetAsync(m.q_v[0].p, 0, (size_t)natoms * 3 * sizeof(double), s));
    if (fixed_host) {
      m.q_fixed.reserve(n * sizeof(int));
      copy_h2d(m.q_fixed.p, fixed_host, (size_t)natoms * sizeof(int));
    }
  }
  RelaxState st{};
  st.dt = dt_start; st.alpha = alpha_start; st.s = 1.0; st.status = RELAX_RUNNING;
  copy_h2d(m.q_state.p, &st, sizeof(st));
}
void relax_rows_fresh(Model &m, int natoms, hipStream_t s) {
  m.r_disp.reserve(((size_t)natoms + 1) * sizeof(int));
  AHIP_CHECK(hipMemsetAsync(m.r_disp.p, 0, ((size_t)natoms + 1) * sizeof(int), s));
}
void relax_step(Model &m, int in, const RelaxFire &p, hipStream_t s) {
  const Model::CellHold &h = m.hold;
  const int natoms = h.natoms, nrows = h.natoms + h.nghost;
  if (natoms == 0) return;
  const CellGeom g = cell_geometry("ahip_relax_cell", h.cell, h.pbc, 0.0);
  RelaxState *st = m.q_state.as<RelaxState>();
  const double *f = m.c_f.as<double>();
  const int *fixed = m.q_fixed.as<int>();
  const unsigned nb = (unsigned)((natoms + 255) / 256);
  hipLaunchKernelGGL(k_relax_gather, dim3(nb), dim3(256), 0, s, natoms, f, m.q_v[in].as<double>(), fixed, st, m.q_part.as<double>(), m.q_fbits.as<int>());
  AHIP_CHECK(prim_sum_columns_f64(m.prim, m.q_part.as<double>(), natoms, 3, st->sums, s));
  AHIP_CHECK(prim_max_i32(m.q_fbits.as<int>(), natoms, &st->fbits, s));
  AHIP_CHECK(prim_max_i32(m.r_disp.as<int>(), natoms, &st->ubits, s));
  hipLaunchKernelGGL(k_relax_decide, dim3(1), dim3(64), 0, s, st, p);
  hipLaunchKernelGGL(k_relax_move, dim3((unsigned)(((long long)nrows + 255) / 256)), dim3(256), 0, s, natoms, nrows, st, m.q_x[in].as<double>(), m.q_v[in].as<double>(), f,
                     fixed, m.r_xhold.as<double>(), m.c_src.as<long long>(), m.r_img.as<int>(), g, m.q_x[in ^ 1].as<double>(), m.q_v[in ^ 1].as<double>(),
                     m.c_x.as<double>(), m.r_disp.as<int>());
  AHIP_CHECK(hipGetLastError());
}
RelaxState relax_read(Model &m, hipStream_t s) {
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  RelaxState st;
  copy_d2h(&st, m.q_state.p, sizeof(st));
  return st;
}
void relax_resume(Model &m, hipStream_t s) {
  const int running = RELAX_RUNNING;
  AHIP_CHECK(hipStreamSynchronize(s));
  copy_h2d(&m.q_state.as<RelaxState>()->status, &running, sizeof(int));
}

// ---- FIRE over the atoms and the cell (ahip_relax_vcell; the algorithm is stated in include/allegro_hip.h) ----
// The generalised coordinates are the reference positions q and c D; the rows of m.c_x are images of x = D q in the cell A0 D^T, whose geometry the decision
// computes on the device (cell_geometry_try) because the host does not look between moves.  Per move: k_vcell_gather (one thread per atom), the reductions,
// k_vcell_decide (one thread, the only writer of the state block), k_vcell_move (one thread per row).  As at fixed cell every kernel returns at once when the
// status is not RUNNING, q and v alternate between two buffers, and no kernel needs a barrier.
__device__ __host__ inline void vcell_apply(const double *D, const double *q, double *x) {
  for (int a = 0; a < 3; ++a) x[a] = D[3 * a] * q[0] + D[3 * a + 1] * q[1] + D[3 * a + 2] * q[2];
}
__device__ __host__ inline double det3(const double *m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// G_i = D^T F_i (0 for a fixed atom), [v.G, G.G, v.v], and the float32 bits of the CARTESIAN |F_i|^2 of a free atom
__global__ void k_vcell_gather(int natoms, const double *f, const double *v, const int *fixed, const VcellState *st, double *gen, double *part, int *fbits) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= natoms || st->status != RELAX_RUNNING) return;
  double vf = 0.0, gg = 0.0, vv = 0.0, ff = 0.0, G[3] = {0.0, 0.0, 0.0};
  if (!(fixed && fixed[i])) {
    const double F[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
    const double *D = st->D;
    for (int d = 0; d < 3; ++d) {
      G[d] = D[d] * F[0] + D[3 + d] * F[1] + D[6 + d] * F[2];
      const double vd = v[3 * i + d];
      vf += vd * G[d]; gg += G[d] * G[d]; vv += vd * vd; ff += F[d] * F[d];
    }
  }
  for (int d = 0; d < 3; ++d) gen[3 * i + d] = G[d];
  part[3 * i] = vf; part[3 * i + 1] = gg; part[3 * i + 2] = vv;
  const float q = (float)ff;
  fbits[i] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
}
__global__ void k_vcell_decide(VcellState *st, const double *engvir, VcellPar p) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || st->status != RELAX_RUNNING) return;
  const double u2 = (double)bits_float(st->ubits), f2 = (double)bits_float(st->fbits);
  st->u2 = u2; st->fmax2 = f2;
  // 1, 2: the largest displacement and the reuse criterion of ahip_compute_cell_reuse, the current cell against the cell of the last rebuild
  if (st->ubits == 0x7fffffff) { st->status = RELAX_NONFINITE; return; }
  double sum_g = 0.0, sum_mg = 0.0;
  for (int d = 0; d < 3; ++d) {
    double q = 0.0;
    for (int k = 0; k < 3; ++k) { const double e = st->geom.h[3 * d + k] - st->hold_cell[3 * d + k]; q += e * e; }
    sum_g += sqrt(q);
    sum_mg += st->hold_images[d] * sqrt(q);
  }
  if (!(sum_g <= st->hold_min_height) || !(2.0 * sqrt(u2) + sum_mg <= p.fire.skin)) { st->status = RELAX_NEED_REBUILD; return; }
  // the generalised force of the strain rows: W_ext = W - pressure V, hydrostatic, mask; G_D = W_ext D^-T / c
  const double *D = st->D;
  const double detD = det3(D), V = fabs(det3(st->geom.h));
  st->detD = detD;
  double W[9] = {engvir[1], engvir[4], engvir[5], engvir[4], engvir[2], engvir[6], engvir[5], engvir[6], engvir[3]};
  for (int a = 0; a < 3; ++a) W[4 * a] -= p.pressure * V;
  if (p.hydrostatic) {
    const double t = (W[0] + W[4] + W[8]) / 3.0;
    for (int k = 0; k < 9; ++k) W[k] = k % 4 == 0 ? t : 0.0;
  }
  const int mk[9] = {p.mask[0], p.mask[3], p.mask[4], p.mask[3], p.mask[1], p.mask[5], p.mask[4], p.mask[5], p.mask[2]};
  double wmax = 0.0;
  for (int k = 0; k < 9; ++k) {
    if (!mk[k]) W[k] = 0.0;
    wmax = fmax(wmax, fabs(W[k]));       // (fmax drops a NaN: the sums below catch it)
  }
  const double sext = wmax / V;
  st->sext = sext;
  // D^-1 by cofactors: inv[3 c + b] = cof[3 b + c] / det
  const double cof[9] = {D[4] * D[8] - D[5] * D[7], D[5] * D[6] - D[3] * D[8], D[3] * D[7] - D[4] * D[6],
                         D[2] * D[7] - D[1] * D[8], D[0] * D[8] - D[2] * D[6], D[1] * D[6] - D[0] * D[7],
                         D[1] * D[5] - D[2] * D[4], D[2] * D[3] - D[0] * D[5], D[0] * D[4] - D[1] * D[3]};
  double GD[9], vf = st->sums[0], ff = st->sums[1], vv = st->sums[2];
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) {
      // (W_ext D^-T)_ac = sum_b W_ab (D^-1)_cb,  (D^-1)_cb = cof[3 b + c] / det
      const double g = (W[3 * a] * cof[c] + W[3 * a + 1] * cof[3 + c] + W[3 * a + 2] * cof[6 + c]) / detD / p.cfac;
      GD[3 * a + c] = g;
      vf += st->vD[3 * a + c] * g; ff += g * g; vv += st->vD[3 * a + c] * st->vD[3 * a + c];
    }
  // 3
  if (st->fbits == 0x7fffffff || !isfinite(vf) || !isfinite(ff) || !isfinite(vv) || !isfinite(V) || !isfinite(sext) || !isfinite(detD) || !(detD > 0.0)) {
    st->status = RELAX_NONFINITE;
    return;
  }
  // 4
  if (sqrt(f2) <= p.fire.fmax && sext <= p.smax) { st->status = RELAX_CONVERGED; return; }
  if (p.check_only) return;
  // 5: FIRE over all natoms + 3 rows
  double dt = st->dt, alpha = st->alpha, c1, c2;
  int npos = st->npos;
  if (vf > 0.0) {
    c1 = 1.0 - alpha;
    c2 = alpha * sqrt(vv / ff);
    if (npos > p.fire.n_min) {
      dt = fmin(dt * p.fire.f_inc, p.fire.dt_max);
      alpha *= p.fire.f_alpha;
    }
    npos += 1;
  } else {
    c1 = c2 = 0.0;
    alpha = p.fire.alpha_start;
    dt *= p.fire.f_dec;
    npos = 0;
  }
  const double k = c2 + dt, dr = dt * sqrt(fmax(c1 * c1 * vv + 2.0 * c1 * k * vf + k * k * ff, 0.0));
  const double sc = dr > p.fire.max_step ? p.fire.max_step / dr : 1.0;
  double Dn[9], vDn[9], An[9];
  for (int e = 0; e < 9; ++e) {
    vDn[e] = c1 * st->vD[e] + k * GD[e];
    Dn[e] = D[e] + sc * dt * vDn[e] / p.cfac;
  }
  for (int d = 0; d < 3; ++d) vcell_apply(Dn, st->A0 + 3 * d, An + 3 * d);      // a_d = D' a0_d
  const int pbc[3] = {1, 1, 1};
  const double detn = det3(Dn);
  CellGeom gn;
  // a move into a cell that is inverted, singular or not finite is not made: the state stays that of the last valid move
  if (!isfinite(detn) || !(detn > 0.0) || cell_geometry_try(An, pbc, 0.0, gn) != 0) { st->status = RELAX_NONFINITE; return; }
  for (int e = 0; e < 9; ++e) { st->D[e] = Dn[e]; st->vD[e] = vDn[e]; }
  st->geom = gn;
  st->dt = dt; st->alpha = alpha; st->npos = npos; st->c1 = c1; st->c2 = c2; st->s = sc;
  st->moves += 1;
}
// q' and v' of the row's source atom from the buffers of the move before and the G of k_vcell_gather, x' = D' q', the row as k_cell_refresh writes it in the
// cell of the state block; atom rows also store q', v' and the displacement bits.  qin / vin / gen are never written by this launch.
__global__ void k_vcell_move(int natoms, int nrows, const VcellState *st, const double *qin, const double *vin, const double *gen, const int *fixed,
                             const double *xhold, const long long *src, const int *img, double *qout, double *vout, double *x, int *disp) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows || st->status != RELAX_RUNNING) return;
  const long long a = r < natoms ? r : src[r - natoms];
  const bool fix = fixed && fixed[a];
  const double c1 = st->c1, k = st->c2 + st->dt, sdt = st->s * st->dt;
  const CellGeom &g = st->geom;
  double qn[3], vn[3], xn[3], dx[3];
  for (int d = 0; d < 3; ++d) {
    vn[d] = fix ? 0.0 : c1 * vin[3 * a + d] + k * gen[3 * a + d];
    qn[d] = fix ? qin[3 * a + d] : qin[3 * a + d] + sdt * vn[d];
  }
  vcell_apply(st->D, qn, xn);
  for (int d = 0; d < 3; ++d) dx[d] = xn[d] - xhold[3 * a + d];
  double c[3];                               // the row is x'_a + c . A'
  for (int d = 0; d < 3; ++d) c[d] = -floor(cell_frac(g, dx, d) + 0.5);
  if (r < natoms) {
    double u2 = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double u = dx[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
      u2 += u * u;
      qout[3 * r + d] = qn[d]; vout[3 * r + d] = vn[d];
    }
    const float q = (float)u2 * 1.000001f;   // rounded up: the criterion must not miss
    disp[r] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
  } else {
    for (int d = 0; d < 3; ++d) c[d] += (double)img[3 * (r - natoms) + d];
  }
  for (int d = 0; d < 3; ++d) x[3 * r + d] = xn[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
}
__global__ void k_vcell_positions(int natoms, const VcellState *st, const double *q, double *x) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= natoms) return;
  double xi[3];
  vcell_apply(st->D, q + 3 * i, xi);
  for (int d = 0; d < 3; ++d) x[3 * i + d] = xi[d];
}
void vcell_begin(Model &m, int natoms, const double *x_host, const int *fixed_host, const double *cell, double dt_start, double alpha_start, hipStream_t s) {
  relax_begin(m, natoms, x_host, fixed_host, dt_start, alpha_start, s);      // q = x, v = 0, the mask
  const size_t n = (size_t)std::max(natoms, 1);
  m.q_g.reserve(n * 3 * sizeof(double));
  m.q_xc.reserve(n * 3 * sizeof(double));
  m.q_vstate.reserve(sizeof(VcellState));
  VcellState st{};
  st.dt = dt_start; st.alpha = alpha_start; st.s = 1.0; st.detD = 1.0; st.status = RELAX_RUNNING;
  const int pbc[3] = {1, 1, 1};
  st.geom = cell_geometry("ahip_relax_vcell", cell, pbc, 0.0);
  for (int k = 0; k < 9; ++k) { st.A0[k] = cell[k]; st.D[k] = k % 4 == 0 ? 1.0 : 0.0; }
  copy_h2d(m.q_vstate.p, &st, sizeof(st));
}
static void vcell_gather_decide(Model &m, int in, const VcellPar &p, hipStream_t s) {
  const int natoms = m.hold.natoms;
  VcellState *st = m.q_vstate.as<VcellState>();
  hipLaunchKernelGGL(k_vcell_gather, dim3((unsigned)((natoms + 255) / 256)), dim3(256), 0, s, natoms, m.c_f.as<double>(), m.q_v[in].as<double>(), m.q_fixed.as<int>(), st,
                     m.q_g.as<double>(), m.q_part.as<double>(), m.q_fbits.as<int>());
  AHIP_CHECK(prim_sum_columns_f64(m.prim, m.q_part.as<double>(), natoms, 3, st->sums, s));
  AHIP_CHECK(prim_max_i32(m.q_fbits.as<int>(), natoms, &st->fbits, s));
  AHIP_CHECK(prim_max_i32(m.r_disp.as<int>(), natoms, &st->ubits, s));
  hipLaunchKernelGGL(k_vcell_decide, dim3(1), dim3(64), 0, s, st, m.c_engvir.as<double>(), p);
}
void vcell_step(Model &m, int in, const VcellPar &p, hipStream_t s) {
  const int natoms = m.hold.natoms, nrows = m.hold.natoms + m.hold.nghost;
  if (natoms == 0) return;
  vcell_gather_decide(m, in, p, s);
  hipLaunchKernelGGL(k_vcell_move, dim3((unsigned)(((long long)nrows + 255) / 256)), dim3(256), 0, s, natoms, nrows, m.q_vstate.as<VcellState>(), m.q_x[in].as<double>(),
                     m.q_v[in].as<double>(), m.q_g.as<double>(), m.q_fixed.as<int>(), m.r_xhold.as<double>(), m.c_src.as<long long>(), m.r_img.as<int>(),
                     m.q_x[in ^ 1].as<double>(), m.q_v[in ^ 1].as<double>(), m.c_x.as<double>(), m.r_disp.as<int>());
  AHIP_CHECK(hipGetLastError());
}
void vcell_check(Model &m, int in, const VcellPar &p, hipStream_t s) {
  if (m.hold.natoms == 0) return;
  VcellPar q = p;
  q.check_only = 1;
  vcell_gather_decide(m, in, q, s);
  AHIP_CHECK(hipGetLastError());
}
void vcell_positions(Model &m, int natoms, int in, hipStream_t s) {
  if (natoms == 0) return;
  hipLaunchKernelGGL(k_vcell_positions, dim3((unsigned)((natoms + 255) / 256)), dim3(256), 0, s, natoms, m.q_vstate.as<VcellState>(), m.q_x[in].as<double>(), m.q_xc.as<double>());
  AHIP_CHECK(hipGetLastError());
}
VcellState vcell_read(Model &m, hipStream_t s) {
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  VcellState st;
  copy_d2h(&st, m.q_vstate.p, sizeof(st));
  return st;
}
// behind a rebuild in the cell st.geom.h: the hold the criterion is taken against from now on, status RUNNING.  The stream is idle (the caller has read st).
void vcell_held(Model &m, VcellState st, hipStream_t s) {
  AHIP_CHECK(hipStreamSynchronize(s));
  for (int k = 0; k < 9; ++k) st.hold_cell[k] = m.hold.cell[k];
  for (int d = 0; d < 3; ++d) st.hold_images[d] = m.hold.images[d];
  st.hold_min_height = m.hold.min_height;
  st.status = RELAX_RUNNING;
  copy_h2d(m.q_vstate.p, &st, sizeof(st));
}
void vcell_resume(Model &m, hipStream_t s) {
  const int running = RELAX_RUNNING;
  AHIP_CHECK(hipStreamSynchronize(s));
  copy_h2d(&m.q_vstate.as<VcellState>()->status, &running, sizeof(int));
}

// ---- MD with its state on the device (ahip_md_cell; the algorithm is stated in include/allegro_hip.h) ----
// BAOAB over the held rows.  Per configuration n: k_md_gather (one thread per atom), the column sum and the two maxima through prims, k_md_decide (one thread,
// the only writer of the state), k_md_move (one thread per row).  As in the relaxation every kernel returns at once when the status is not RUNNING, x and w
// alternate between two buffers, and no kernel needs a barrier.
// Philox4x32-10 (Salmon et al. 2011) with plain 64-bit products
__device__ __host__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned *out) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// xi(atom, step): three standard normals from the counters (atom, step lo, step hi, j), j = 0, 1, by Box-Muller on 53-bit uniforms in (0, 1)
__device__ __host__ inline void md_xi(unsigned long long seed, long long atom, unsigned long long step, double *xi) {
  for (unsigned j = 0; j < 2; ++j) {
    unsigned w[4];
    philox4x32_10((unsigned)atom, (unsigned)step, (unsigned)(step >> 32), j, (unsigned)seed, (unsigned)(seed >> 32), w);
    const double u1 = ((double)(((unsigned long long)w[0] << 21) | (w[1] >> 11)) + 0.5) * 0x1p-53;
    const double u2 = ((double)(((unsigned long long)w[2] << 21) | (w[3] >> 11)) + 0.5) * 0x1p-53;
    const double rad = sqrt(-2.0 * log(u1)), phi = 6.283185307179586 * u2;
    xi[2 * j] = rad * cos(phi);
    if (j == 0) xi[1] = rad * sin(phi);
  }
}
__global__ void k_md_noise(unsigned long long seed, unsigned long long step, int n, double *out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  md_xi(seed, i, step, out + 3 * i);
}
// v_n of every atom from w and the forces of configuration n; m |v_n|^2 and the |F_i|^2 bits as k_relax_gather forms them; the frame row of n
__global__ void k_md_gather(int natoms, const double *f, const double *x, const double *w, const double *mass, const int *fixed, const MdState *st, MdPar p,
                            double *vnow, double *part, int *fbits, double *frames) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= natoms || st->status != MD_RUNNING) return;
  const int n = st->n;
  const bool fix = fixed && fixed[i];
  const double k = n > 0 ? p.hdtf / mass[i] : 0.0;
  double ff = 0.0, vv = 0.0;
  for (int d = 0; d < 3; ++d) {
    const double fd = f[3 * i + d], vd = fix ? 0.0 : w[3 * i + d] + k * fd;
    vnow[3 * i + d] = vd;
    vv += vd * vd;
    if (!fix) ff += fd * fd;
  }
  part[i] = mass[i] * vv;
  const float q = (float)ff;                 // non-negative floats order like their bit patterns (k_cell_refresh)
  fbits[i] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
  if (p.frame_every > 0 && n % p.frame_every == 0) {
    double *row = frames + ((size_t)(n / p.frame_every) * (size_t)natoms + (size_t)i) * 3;
    for (int d = 0; d < 3; ++d) row[d] = x[3 * i + d];
  }
}
__global__ void k_md_decide(MdState *st, MdPar p, const double *engvir, double *thermo) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || st->status != MD_RUNNING) return;
  const double u2 = (double)bits_float(st->ubits), f2 = (double)bits_float(st->fbits);
  st->u2 = u2; st->fmax2 = f2;
  if (st->ubits == 0x7fffffff) { st->status = MD_NONFINITE; return; }
  if (2.0 * sqrt(u2) > p.skin) { st->status = MD_NEED_REBUILD; return; }
  if (st->fbits == 0x7fffffff || !isfinite(st->sums[0]) || !isfinite(engvir[0])) { st->status = MD_NONFINITE; return; }
  const int n = st->n;
  if (n % p.sample_every == 0) {
    double *row = thermo + 8 * (size_t)(n / p.sample_every);
    row[0] = engvir[0];
    row[1] = 0.5 * p.mvv2e * st->sums[0];
    for (int k = 0; k < 6; ++k) row[2 + k] = engvir[1 + k];
  }
  if (n == p.nsteps) { st->status = MD_DONE; return; }
  st->n = n + 1;
}
// The move out of configuration n = st->n - 1 (the decision has counted it already): second half kick, half drift, thermostat, half drift of the row's source
// atom, the row as k_relax_move writes it; atom rows also store x', w' and the displacement bits.  xin / win / vnow are never written by this launch.
__global__ void k_md_move(int natoms, int nrows, const MdState *st, MdPar p, const double *xin, const double *vnow, const double *f, const double *mass,
                          const int *fixed, const double *xhold, const long long *src, const int *img, CellGeom g, double *xout, double *wout, double *x, int *disp) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows || st->status != MD_RUNNING) return;
  const long long a = r < natoms ? r : src[r - natoms];
  const bool fix = fixed && fixed[a];
  const double ma = mass[a], k = p.hdtf / ma, hdt = 0.5 * p.dt;
  double xi[3] = {0.0, 0.0, 0.0}, sig = 0.0;
  if (p.gamma > 0.0 && !fix) {
    md_xi(p.seed, a, p.step0 + (unsigned long long)(st->n - 1), xi);
    sig = p.c2 * sqrt(p.kT / (ma * p.mvv2e));
  }
  double xn[3], wn[3], dx[3];
  for (int d = 0; d < 3; ++d) {
    const double vh = vnow[3 * a + d] + k * f[3 * a + d];
    const double xh = xin[3 * a + d] + hdt * vh;
    wn[d] = fix ? 0.0 : (p.gamma > 0.0 ? p.c1 * vh + sig * xi[d] : vh);
    xn[d] = fix ? xin[3 * a + d] : xh + hdt * wn[d];
    dx[d] = xn[d] - xhold[3 * a + d];
  }
  double c[3];                               // the row is x'_a + c . A
  for (int d = 0; d < 3; ++d) c[d] = g.pbc[d] ? -floor(cell_frac(g, dx, d) + 0.5) : 0.0;
  if (r < natoms) {
    double u2 = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double u = dx[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
      u2 += u * u;
      xout[3 * r + d] = xn[d]; wout[3 * r + d] = wn[d];
    }
    const float q = (float)u2 * 1.000001f;   // rounded up: the criterion must not miss
    disp[r] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
  } else {
    for (int d = 0; d < 3; ++d) c[d] += (double)img[3 * (r - natoms) + d];
  }
  for (int d = 0; d < 3; ++d) x[3 * r + d] = xn[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
}
void md_begin(Model &m, int natoms, const double *x_host, const double *v_host, const double *mass_host, const int *fixed_host, size_t thermo_rows, size_t frame_rows,
              hipStream_t s) {
  const size_t n = (size_t)std::max(natoms, 1);
  for (int k = 0; k < 2; ++k) { m.q_x[k].reserve(n * 3 * sizeof(double)); m.q_v[k].reserve(n * 3 * sizeof(double)); }
  m.q_vnow.reserve(n * 3 * sizeof(double));
  m.q_mass.reserve(n * sizeof(double));
  m.q_part.reserve(n * 3 * sizeof(double));
  m.q_fbits.reserve(n * sizeof(int));
  m.q_mstate.reserve(sizeof(MdState));
  m.q_thermo.reserve(std::max<size_t>(thermo_rows, 1) * 8 * sizeof(double));
  m.q_frames.reserve(std::max<size_t>(frame_rows * n * 3, 1) * sizeof(double));
  m.q_fixed.release();                       // no mask: the kernels take a null pointer
  if (natoms > 0) {
    copy_h2d(m.q_x[0].p, x_host, (size_t)natoms * 3 * sizeof(double));
    copy_h2d(m.q_v[0].p, v_host, (size_t)natoms * 3 * sizeof(double));
    copy_h2d(m.q_mass.p, mass_host, (size_t)natoms * sizeof(double));
    if (fixed_host) {
      m.q_fixed.reserve(n * sizeof(int));
      copy_h2d(m.q_fixed.p, fixed_host, (size_t)natoms * sizeof(int));
    }
  }
  AHIP_CHECK(hipMemsetAsync(m.q_thermo.p, 0, std::max<size_t>(thermo_rows, 1) * 8 * sizeof(double), s));
  MdState st{};
  st.status = MD_RUNNING;
  copy_h2d(m.q_mstate.p, &st, sizeof(st));
}
void md_step(Model &m, int in, const MdPar &p, bool move, hipStream_t s) {
  const Model::CellHold &h = m.hold;
  const int natoms = h.natoms, nrows = h.natoms + h.nghost;
  if (natoms == 0) return;
  const CellGeom g = cell_geometry("ahip_md_cell", h.cell, h.pbc, 0.0);
  MdState *st = m.q_mstate.as<MdState>();
  const double *f = m.c_f.as<double>(), *mass = m.q_mass.as<double>();
  const int *fixed = m.q_fixed.as<int>();
  hipLaunchKernelGGL(k_md_gather, dim3((unsigned)((natoms + 255) / 256)), dim3(256), 0, s, natoms, f, m.q_x[in].as<double>(), m.q_v[in].as<double>(), mass, fixed, st, p,
                     m.q_vnow.as<double>(), m.q_part.as<double>(), m.q_fbits.as<int>(), m.q_frames.as<double>());
  AHIP_CHECK(prim_sum_columns_f64(m.prim, m.q_part.as<double>(), natoms, 1, st->sums, s));
  AHIP_CHECK(prim_max_i32(m.q_fbits.as<int>(), natoms, &st->fbits, s));
  AHIP_CHECK(prim_max_i32(m.r_disp.as<int>(), natoms, &st->ubits, s));
  hipLaunchKernelGGL(k_md_decide, dim3(1), dim3(64), 0, s, st, p, m.c_engvir.as<double>(), m.q_thermo.as<double>());
  if (move)
    hipLaunchKernelGGL(k_md_move, dim3((unsigned)(((long long)nrows + 255) / 256)), dim3(256), 0, s, natoms, nrows, st, p, m.q_x[in].as<double>(), m.q_vnow.as<double>(), f,
                       mass, fixed, m.r_xhold.as<double>(), m.c_src.as<long long>(), m.r_img.as<int>(), g, m.q_x[in ^ 1].as<double>(), m.q_v[in ^ 1].as<double>(),
                       m.c_x.as<double>(), m.r_disp.as<int>());
  AHIP_CHECK(hipGetLastError());
}
MdState md_read(Model &m, hipStream_t s) {
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  MdState st;
  copy_d2h(&st, m.q_mstate.p, sizeof(st));
  return st;
}
void md_resume(Model &m, hipStream_t s) {
  const int running = MD_RUNNING;
  AHIP_CHECK(hipStreamSynchronize(s));
  copy_h2d(&m.q_mstate.as<MdState>()->status, &running, sizeof(int));
}
void md_noise(unsigned long long seed, unsigned long long step, int n, double *out_dev, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_md_noise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed, step, n, out_dev);
  AHIP_CHECK(hipGetLastError());
}

// ---- MD at constant pressure with its state on the device (ahip_npt_cell; the algorithm is stated in include/allegro_hip.h) ----
// The BAOAB of the MD above inside an isotropic stochastic cell rescaling.  Per configuration n: k_npt_gather (one thread per atom), the reductions, k_npt_decide
// (one thread, the only writer of the state: it also forms the rescaling factor, the next cell and its geometry, which the host has not seen), k_npt_move (one
// thread per row, in the cell of the state block).  Every kernel returns at once when the status is not RUNNING, x and w alternate between two buffers, and no
// kernel needs a barrier.
#define NPT_NOISE_ATOM 0xFFFFFFFFll      // the atom word of xi_V: natoms is an int, so no atom has it
// v_n, m |v_n|^2, the |F_i|^2 bits and the frame row of n, exactly as k_md_gather forms them
__global__ void k_npt_gather(int natoms, const double *f, const double *x, const double *w, const double *mass, const int *fixed, const NptState *st, MdPar p,
                             double *vnow, double *part, int *fbits, double *frames) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= natoms || st->status != MD_RUNNING) return;
  const int n = st->n;
  const bool fix = fixed && fixed[i];
  const double k = n > 0 ? p.hdtf / mass[i] : 0.0;
  double ff = 0.0, vv = 0.0;
  for (int d = 0; d < 3; ++d) {
    const double fd = f[3 * i + d], vd = fix ? 0.0 : w[3 * i + d] + k * fd;
    vnow[3 * i + d] = vd;
    vv += vd * vd;
    if (!fix) ff += fd * fd;
  }
  part[i] = mass[i] * vv;
  const float q = (float)ff;                 // non-negative floats order like their bit patterns (k_cell_refresh)
  fbits[i] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
  if (p.frame_every > 0 && n % p.frame_every == 0) {
    double *row = frames + ((size_t)(n / p.frame_every) * (size_t)natoms + (size_t)i) * 3;
    for (int d = 0; d < 3; ++d) row[d] = x[3 * i + d];
  }
}
__global__ void k_npt_decide(NptState *st, NptPar p, const double *engvir, double *thermo, double *fcells) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || st->status != MD_RUNNING) return;
  const double u2 = (double)bits_float(st->ubits), f2 = (double)bits_float(st->fbits);
  st->u2 = u2; st->fmax2 = f2;
  // 1, 2: the largest displacement and the reuse criterion of ahip_compute_cell_reuse, the current cell against the cell of the last rebuild
  if (st->ubits == 0x7fffffff) { st->status = MD_NONFINITE; return; }
  double sum_g = 0.0, sum_mg = 0.0;
  for (int d = 0; d < 3; ++d) {
    double q = 0.0;
    for (int k = 0; k < 3; ++k) { const double e = st->geom.h[3 * d + k] - st->hold_cell[3 * d + k]; q += e * e; }
    sum_g += sqrt(q);
    sum_mg += st->hold_images[d] * sqrt(q);
  }
  if (!(2.0 * sqrt(u2) + sum_mg <= p.md.skin) || !(sum_g <= st->hold_min_height)) { st->status = MD_NEED_REBUILD; return; }
  // 3
  const double V = fabs(det3(st->geom.h)), ke = 0.5 * p.md.mvv2e * st->sums[0];
  const double P = (2.0 * ke + engvir[1] + engvir[2] + engvir[3]) / (3.0 * V);
  if (st->fbits == 0x7fffffff || !isfinite(st->sums[0]) || !isfinite(engvir[0]) || !isfinite(V) || !(V > 0.0) || !isfinite(P)) { st->status = MD_NONFINITE; return; }
  st->V = V; st->P = P;
  // 4
  const int n = st->n;
  if (n % p.md.sample_every == 0) {
    double *row = thermo + 10 * (size_t)(n / p.md.sample_every);
    row[0] = engvir[0];
    row[1] = ke;
    for (int k = 0; k < 6; ++k) row[2 + k] = engvir[1 + k];
    row[8] = V; row[9] = P;
  }
  if (p.md.frame_every > 0 && n % p.md.frame_every == 0)
    for (int k = 0; k < 9; ++k) fcells[9 * (size_t)(n / p.md.frame_every) + k] = st->geom.h[k];
  // 5
  if (n == p.md.nsteps) { st->status = MD_DONE; return; }
  // 6: d(ln V), the factor of the lattice vectors, the next cell with its inverse
  double de = -p.beta_over_tau * (p.p0 - P) * p.md.dt;
  if (p.noise > 0.0) {
    double xi[3];
    md_xi(p.md.seed, NPT_NOISE_ATOM, p.md.step0 + (unsigned long long)n, xi);
    de += p.noise / sqrt(V) * xi[0];
  }
  const double mu = exp(de / 3.0);
  double An[9];
  for (int k = 0; k < 9; ++k) An[k] = mu * st->geom.h[k];
  const int pbc[3] = {1, 1, 1};
  CellGeom gn;
  // a rescaling that is not finite, or into a cell that is singular, is not made: the state stays that of the last valid step
  if (!isfinite(mu) || cell_geometry_try(An, pbc, 0.0, gn) != 0) { st->status = MD_NONFINITE; return; }
  st->mu = mu;
  st->geom = gn;
  st->n = n + 1;
}
// The move out of configuration n = st->n - 1 (the decision has counted it already): the BAOAB move of k_md_move on the row's source atom, then x'' = mu x',
// w'' = w' / mu (a fixed atom follows the cell: x'' = mu x, w'' = 0); the row as k_vcell_move writes it, the exact periodic image in the cell of the state block;
// atom rows also store x'', w'' and the displacement bits.  xin / vnow are never written by this launch.
__global__ void k_npt_move(int natoms, int nrows, const NptState *st, MdPar p, const double *xin, const double *vnow, const double *f, const double *mass,
                           const int *fixed, const double *xhold, const long long *src, const int *img, double *xout, double *wout, double *x, int *disp) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows || st->status != MD_RUNNING) return;
  const long long a = r < natoms ? r : src[r - natoms];
  const bool fix = fixed && fixed[a];
  const double ma = mass[a], k = p.hdtf / ma, hdt = 0.5 * p.dt, mu = st->mu;
  const CellGeom &g = st->geom;
  double xi[3] = {0.0, 0.0, 0.0}, sig = 0.0;
  if (p.gamma > 0.0 && !fix) {
    md_xi(p.seed, a, p.step0 + (unsigned long long)(st->n - 1), xi);
    sig = p.c2 * sqrt(p.kT / (ma * p.mvv2e));
  }
  double xn[3], wn[3], dx[3];
  for (int d = 0; d < 3; ++d) {
    const double vh = vnow[3 * a + d] + k * f[3 * a + d];
    const double xh = xin[3 * a + d] + hdt * vh;
    const double wd = p.gamma > 0.0 ? p.c1 * vh + sig * xi[d] : vh;
    wn[d] = fix ? 0.0 : wd / mu;
    xn[d] = mu * (fix ? xin[3 * a + d] : xh + hdt * wd);
    dx[d] = xn[d] - xhold[3 * a + d];
  }
  double c[3];                               // the row is x''_a + c . A'
  for (int d = 0; d < 3; ++d) c[d] = -floor(cell_frac(g, dx, d) + 0.5);
  if (r < natoms) {
    double u2 = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double u = dx[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
      u2 += u * u;
      xout[3 * r + d] = xn[d]; wout[3 * r + d] = wn[d];
    }
    const float q = (float)u2 * 1.000001f;   // rounded up: the criterion must not miss
    disp[r] = q >= 0.f && q <= 3.0e38f ? float_bits(q) : 0x7fffffff;
  } else {
    for (int d = 0; d < 3; ++d) c[d] += (double)img[3 * (r - natoms) + d];
  }
  for (int d = 0; d < 3; ++d) x[3 * r + d] = xn[d] + (c[0] * g.h[d] + c[1] * g.h[3 + d] + c[2] * g.h[6 + d]);
}
__global__ void k_npt_noise(unsigned long long seed, unsigned long long step, double *out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double xi[3];
  md_xi(seed, NPT_NOISE_ATOM, step, xi);
  out[0] = xi[0];
}
void npt_begin(Model &m, int natoms, const double *x_host, const double *v_host, const double *mass_host, const int *fixed_host, const double *cell, size_t thermo_rows,
               size_t frame_rows, hipStream_t s) {
  md_begin(m, natoms, x_host, v_host, mass_host, fixed_host, thermo_rows, frame_rows, s);      // x, w = v, the masses, the mask, the frames
  m.q_nstate.reserve(sizeof(NptState));
  m.q_nthermo.reserve(std::max<size_t>(thermo_rows, 1) * 10 * sizeof(double));
  m.q_fcells.reserve(std::max<size_t>(frame_rows, 1) * 9 * sizeof(double));
  AHIP_CHECK(hipMemsetAsync(m.q_nthermo.p, 0, std::max<size_t>(thermo_rows, 1) * 10 * sizeof(double), s));
  NptState st{};
  st.mu = 1.0;
  st.status = MD_RUNNING;
  const int pbc[3] = {1, 1, 1};
  st.geom = cell_geometry("ahip_npt_cell", cell, pbc, 0.0);
  copy_h2d(m.q_nstate.p, &st, sizeof(st));
}
void npt_step(Model &m, int in, const NptPar &p, bool move, hipStream_t s) {
  const int natoms = m.hold.natoms, nrows = m.hold.natoms + m.hold.nghost;
  if (natoms == 0) return;
  NptState *st = m.q_nstate.as<NptState>();
  const double *f = m.c_f.as<double>(), *mass = m.q_mass.as<double>();
  const int *fixed = m.q_fixed.as<int>();
  hipLaunchKernelGGL(k_npt_gather, dim3((unsigned)((natoms + 255) / 256)), dim3(256), 0, s, natoms, f, m.q_x[in].as<double>(), m.q_v[in].as<double>(), mass, fixed, st, p.md,
                     m.q_vnow.as<double>(), m.q_part.as<double>(), m.q_fbits.as<int>(), m.q_frames.as<double>());
  AHIP_CHECK(prim_sum_columns_f64(m.prim, m.q_part.as<double>(), natoms, 1, st->sums, s));
  AHIP_CHECK(prim_max_i32(m.q_fbits.as<int>(), natoms, &st->fbits, s));
  AHIP_CHECK(prim_max_i32(m.r_disp.as<int>(), natoms, &st->ubits, s));
  hipLaunchKernelGGL(k_npt_decide, dim3(1), dim3(64), 0, s, st, p, m.c_engvir.as<double>(), m.q_nthermo.as<double>(), m.q_fcells.as<double>());
  if (move)
    hipLaunchKernelGGL(k_npt_move, dim3((unsigned)(((long long)nrows + 255) / 256)), dim3(256), 0, s, natoms, nrows, st, p.md, m.q_x[in].as<double>(), m.q_vnow.as<double>(), f,
                       mass, fixed, m.r_xhold.as<double>(), m.c_src.as<long long>(), m.r_img.as<int>(), m.q_x[in ^ 1].as<double>(), m.q_v[in ^ 1].as<double>(),
                       m.c_x.as<double>(), m.r_disp.as<int>());
  AHIP_CHECK(hipGetLastError());
}
NptState npt_read(Model &m, hipStream_t s) {
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  NptState st;
  copy_d2h(&st, m.q_nstate.p, sizeof(st));
  return st;
}
// behind a rebuild in the cell st.geom.h: the hold the criterion is taken against from now on, status RUNNING.  The stream is idle (the caller has read st).
void npt_held(Model &m, NptState st, hipStream_t s) {
  AHIP_CHECK(hipStreamSynchronize(s));
  for (int k = 0; k < 9; ++k) st.hold_cell[k] = m.hold.cell[k];
  for (int d = 0; d < 3; ++d) st.hold_images[d] = m.hold.images[d];
  st.hold_min_height = m.hold.min_height;
  st.status = MD_RUNNING;
  copy_h2d(m.q_nstate.p, &st, sizeof(st));
}
void npt_resume(Model &m, hipStream_t s) {
  const int running = MD_RUNNING;
  AHIP_CHECK(hipStreamSynchronize(s));
  copy_h2d(&m.q_nstate.as<NptState>()->status, &running, sizeof(int));
}
void npt_noise(unsigned long long seed, unsigned long long step, double *out_dev, hipStream_t s) {
  hipLaunchKernelGGL(k_npt_noise, dim3(1), dim3(64), 0, s, seed, step, out_dev);
  AHIP_CHECK(hipGetLastError());
}

// ---- a batch of cells as ONE non-periodic cloud (ahip_compute_cells) ----
// Every structure keeps its own frame for the wrap and for its ghost images; only before the list build is every row (atom or ghost) translated by its
// structure's origin, chosen on the host so that rows of different structures are farther apart than the list cutoff.  Behind that the batch is one list of
// centres like any other.  The table has one entry per structure plus a closing one whose `first` is the number of atoms.
struct CellEntry {
  CellGeom g;
  double origin[3];     // added to the structure's rows for the list build and the evaluation
  int first;            // its first atom
  int pad;
};
// the single-cell kernels' row bodies with the geometry looked up per atom.  The wrap is out of place (the upload stays as it came); the model types travel along
__global__ void k_cells_wrap(int n, const double *xin, const int *mtin, const int *sidx, const CellEntry *tab, double *x, int *mt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double *xi = x + 3 * i;
  for (int d = 0; d < 3; ++d) xi[d] = xin[3 * i + d];
  mt[i] = mtin[i];
  cell_wrap_row(tab[sidx[i]].g, xi);
}
__global__ void k_cells_count(int n, const double *x, const int *sidx, const CellEntry *tab, int *cnt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cnt[i] = cell_count_row(tab[sidx[i]].g, x + 3 * i);
}
// over the scan of the WHOLE batch: ascending source atom groups the ghosts by structure; src is the atom's index in the batch
__global__ void k_cells_fill(int n, const double *x, const int *mtype, const int *sidx, const CellEntry *tab, const int *off, int capacity, double *xg, int *mtg,
                             long long *src, double *shift) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= capacity || k >= off[n]) return;
  const int a = cell_row_atom(off, n, k);
  if (!cell_fill_row(tab[sidx[a]].g, x + 3 * (long long)a, k - off[a], k, xg, shift)) return;
  mtg[k] = mtype[a];
  src[k] = a;
}
// rows (atoms, then ghosts) in the structures' own frames -> their places in the cloud
__global__ void k_cells_place(int natoms, int nall, const double *x, const int *sidx, const long long *src, const CellEntry *tab, double *xp) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nall) return;
  const long long a = r < natoms ? r : src[r - natoms];
  const double *o = tab[sidx[a]].origin;
  for (int d = 0; d < 3; ++d) xp[3 * r + d] = x[3 * r + d] + o[d];
}
// Energy, virial and ghost count of every structure: one workgroup per structure, float64, a fixed order (thread t takes the rows t, t + NT, ..., atoms before
// ghosts; then a tree over the threads).  The virial is the row sum  W = sum_rows x_row (x) F_row  over the structure's atoms and ghosts with the forces BEFORE the
// ghosts are folded home and positions in the structure's own frame: with F_i += g_e, F_j -= g_e per edge this is -sum_e r_e (x) g_e, whatever kernel wrote the forces.
// out[8 s ..]: energy, xx, yy, zz, xy, xz, yz, ghosts.
#ifdef AHIP_HOST_EMU
constexpr int CELLS_REDUCE_THREADS = 1;      // the emulation launches threads one after the other: a single thread does the whole structure
#else
constexpr int CELLS_REDUCE_THREADS = 256;
#endif
__device__ inline void cells_row_virial(const double *x, const double *f, double *w) {
  w[0] += x[0] * f[0]; w[1] += x[1] * f[1]; w[2] += x[2] * f[2];
  w[3] += 0.5 * (x[0] * f[1] + x[1] * f[0]); w[4] += 0.5 * (x[0] * f[2] + x[2] * f[0]); w[5] += 0.5 * (x[1] * f[2] + x[2] * f[1]);
}
__global__ void __launch_bounds__(CELLS_REDUCE_THREADS) k_cells_reduce(int nstruct, int natoms, const CellEntry *tab, const int *off, const double *x,
                                                                          const double *f, const double *eatom, double *out) {
  const int s = blockIdx.x, t = threadIdx.x;
  if (s >= nstruct) return;                                // (whole workgroups: the barriers below stay uniform)
  const int a0 = tab[s].first, a1 = tab[s + 1].first;
  const long long g0 = (long long)natoms + off[a0], g1 = (long long)natoms + off[a1];
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long r = a0 + t; r < a1; r += CELLS_REDUCE_THREADS) { acc[0] += eatom[r]; cells_row_virial(x + 3 * r, f + 3 * r, acc + 1); }
  for (long long r = g0 + t; r < g1; r += CELLS_REDUCE_THREADS) cells_row_virial(x + 3 * r, f + 3 * r, acc + 1);
#ifndef AHIP_HOST_EMU
  __shared__ double sh[7][CELLS_REDUCE_THREADS];
  for (int k = 0; k < 7; ++k) sh[k][t] = acc[k];
  __syncthreads();
  for (int w = CELLS_REDUCE_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) for (int k = 0; k < 7; ++k) sh[k][t] += sh[k][t + w];
    __syncthreads();
  }
  for (int k = 0; k < 7; ++k) acc[k] = sh[k][0];
#endif
  if (t == 0) {
    for (int k = 0; k < 7; ++k) out[8 * (long long)s + k] = acc[k];
    out[8 * (long long)s + 7] = (double)(off[a1] - off[a0]);
  }
}

// bins of the grid neigh_build derives from a bounding box (its rule, restated)
static long long neigh_grid_bins(const double *lo, const double *hi, double rc_list) {
  long long nbins = 1;
  for (int d = 0; d < 3; ++d) nbins *= std::min(1024, std::max(1, (int)std::floor((hi[d] - lo[d]) / rc_list)));
  return nbins;
}

size_t cells_plan(int nstruct, const int *first, const double *x, const double *cells, const int *pbc, double rc, std::vector<unsigned char> &table, double *lo,
                  double *hi) {
  std::vector<CellEntry> tab((size_t)nstruct + 1);
  std::vector<double> blo((size_t)nstruct * 3), ext((size_t)nstruct * 3);
  const int natoms = nstruct > 0 ? first[nstruct] : 0;
  double rows = (double)natoms, slot[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < nstruct; ++s) {
    const std::string who = "ahip_compute_cells: structure " + std::to_string(s);
    CellEntry &e = tab[(size_t)s];
    e.g = cell_geometry(who.c_str(), cells + 9 * (size_t)s, pbc + 3 * (size_t)s, rc);
    e.first = first[s]; e.pad = 0;
    const int n = first[s + 1] - first[s];
    rows += cell_most_images(e.g, n);
    if (!(rows <= 2147483647.0))
      throw ArgError(who + ": atoms and images of the batch exceed 2^31 - 1 rows up to here (the offsets are 32-bit); split the batch, or the cell is too thin for this cutoff");
    // the fractional range of its rows: [-m_d, 1 + m_d] on a periodic axis, what its atoms have on an open one (a molecule may lie outside its cell)
    // (open axes: measured on the WRAPPED position, through the kernel's own row body -- far outside the cell along a periodic axis the open-axis
    // component of the caller's position carries a rounding error that the wrapped row no longer has)
    double a[3], b[3];
    const bool open = !e.g.pbc[0] || !e.g.pbc[1] || !e.g.pbc[2];
    for (int d = 0; d < 3; ++d) {
      if (e.g.pbc[d]) { a[d] = -e.g.m[d]; b[d] = 1.0 + e.g.m[d]; }
      else { a[d] = n > 0 ? HUGE_VAL : 0.0; b[d] = n > 0 ? -HUGE_VAL : 0.0; }
    }
    for (int i = first[s]; open && i < first[s + 1]; ++i) {
      double xi[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
      cell_wrap_row(e.g, xi);
      for (int d = 0; d < 3; ++d) {
        if (e.g.pbc[d]) continue;
        const double v = cell_frac(e.g, xi, d);
        a[d] = std::min(a[d], v); b[d] = std::max(b[d], v);
      }
    }
    for (int d = 0; d < 3; ++d) if (!e.g.pbc[d]) { a[d] -= 1e-9; b[d] += 1e-9; }
    // ... and the Cartesian bounding box of that parallelepiped
    for (int k = 0; k < 3; ++k) {
      double l = 0.0, h = 0.0;
      for (int d = 0; d < 3; ++d) {
        const double p = a[d] * e.g.h[3 * d + k], q = b[d] * e.g.h[3 * d + k];
        l += std::min(p, q); h += std::max(p, q);
      }
      if (!std::isfinite(l) || !std::isfinite(h)) throw ArgError(who + ": a position is not finite");
      blo[3 * (size_t)s + k] = l; ext[3 * (size_t)s + k] = h - l;
      slot[k] = std::max(slot[k], h - l);
    }
  }
  // uniform slots of the largest extent plus the gap, on a near-cubic grid (the most slots along the thinnest slot dimension)
  int order[3] = {0, 1, 2}, cnt[3] = {1, 1, 1};
  for (int k = 0; k < 3; ++k) slot[k] += rc + 1e-6;
  std::sort(order, order + 3, [&](int p, int q) { return slot[p] < slot[q]; });
  if (nstruct > 0) {
    int n0 = (int)std::ceil(std::cbrt((double)nstruct));
    while ((long long)n0 * n0 * n0 < nstruct) ++n0;
    while (n0 > 1 && (long long)(n0 - 1) * (n0 - 1) * (n0 - 1) >= nstruct) --n0;
    int n1 = (int)std::ceil(std::sqrt((double)nstruct / n0));
    while ((long long)n0 * n1 * n1 < nstruct) ++n1;
    const int n2 = (int)(((long long)nstruct + (long long)n0 * n1 - 1) / ((long long)n0 * n1));
    cnt[order[0]] = n0; cnt[order[1]] = n1; cnt[order[2]] = n2;
  }
  for (int s = 0; s < nstruct; ++s) {
    const int i0 = s % cnt[order[0]], i1 = (s / cnt[order[0]]) % cnt[order[1]], i2 = s / (cnt[order[0]] * cnt[order[1]]);
    int idx[3];
    idx[order[0]] = i0; idx[order[1]] = i1; idx[order[2]] = i2;
    for (int k = 0; k < 3; ++k) tab[(size_t)s].origin[k] = idx[k] * slot[k] - blo[3 * (size_t)s + k];
  }
  CellEntry &end = tab[(size_t)nstruct];
  std::memset(&end, 0, sizeof(CellEntry));
  end.first = natoms;
  for (int k = 0; k < 3; ++k) { lo[k] = 0.0; hi[k] = cnt[k] * slot[k]; }
  if (neigh_grid_bins(lo, hi, rc) > (1LL << 26))
    throw ArgError("ahip_compute_cells: the structures' common slot (" + std::to_string(slot[0]) + " x " + std::to_string(slot[1]) + " x " + std::to_string(slot[2]) +
                   ", the largest extent of any) times " + std::to_string(nstruct) + " structures needs more than 2^26 neighbor bins: split the batch");
  table.resize(tab.size() * sizeof(CellEntry));
  std::memcpy(table.data(), tab.data(), table.size());
  return sizeof(CellEntry);
}
void cells_wrap(int natoms, const double *xin, const int *mtin, const int *sidx, const void *table, double *x, int *mt, hipStream_t s) {
  if (natoms <= 0) return;
  hipLaunchKernelGGL(k_cells_wrap, dim3((unsigned)((natoms + 255) / 256)), dim3(256), 0, s, natoms, xin, mtin, sidx, (const CellEntry *)table, x, mt);
  AHIP_CHECK(hipGetLastError());
}
int cells_count(Model &m, int natoms, const double *x, const int *sidx, const void *table, hipStream_t s) {
  if (natoms <= 0) return 0;
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  st.cnt.reserve(((size_t)natoms + 1) * sizeof(int));
  st.goff.reserve(((size_t)natoms + 2) * sizeof(int));
  hipLaunchKernelGGL(k_cells_count, dim3((unsigned)((natoms + 255) / 256)), dim3(256), 0, s, natoms, x, sidx, (const CellEntry *)table, st.cnt.as<int>());
  AHIP_CHECK(prim_exclusive_scan_i32(m.prim, st.cnt.as<int>(), st.goff.as<int>(), natoms, s));
  int tot = 0;
  AHIP_CHECK(hipMemcpyAsync(&tot, st.goff.as<int>() + natoms, sizeof(int), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  AHIP_CHECK(hipGetLastError());
  if (tot < 0) throw ArgError("ahip_compute_cells: more than 2^31 - 1 images");
  return tot;
}
void cells_fill(Model &m, int natoms, int nghost, const double *x, const int *mtype, const int *sidx, const void *table, double *xg, int *mtg, long long *src,
                double *shift, hipStream_t s) {
  if (natoms <= 0 || nghost <= 0) return;
  NbState &st = *(NbState *)m.nb_state;
  hipLaunchKernelGGL(k_cells_fill, dim3((unsigned)(((long long)nghost + 255) / 256)), dim3(256), 0, s, natoms, x, mtype, sidx, (const CellEntry *)table,
                     st.goff.as<int>(), nghost, xg, mtg, src, shift);
  AHIP_CHECK(hipGetLastError());
}
void cells_place(int natoms, int nall, const double *x, const int *sidx, const long long *src, const void *table, double *xp, hipStream_t s) {
  if (nall <= 0) return;
  hipLaunchKernelGGL(k_cells_place, dim3((unsigned)(((long long)nall + 255) / 256)), dim3(256), 0, s, natoms, nall, x, sidx, src, (const CellEntry *)table, xp);
  AHIP_CHECK(hipGetLastError());
}
void cells_reduce(Model &m, int nstruct, int natoms, const void *table, const double *x, const double *f, const double *eatom, double *out, hipStream_t s) {
  if (nstruct <= 0 || natoms <= 0) return;
  NbState &st = *(NbState *)m.nb_state;
  hipLaunchKernelGGL(k_cells_reduce, dim3((unsigned)nstruct), dim3(CELLS_REDUCE_THREADS), 0, s, nstruct, natoms, (const CellEntry *)table, st.goff.as<int>(), x, f, eatom, out);
  AHIP_CHECK(hipGetLastError());
}

void neigh_free(Model &m) {
  if (!m.nb_state) return;
  NbState *st = (NbState *)m.nb_state;
  for (DevBuf *b : {&st->bin_of, &st->bin_cnt, &st->bin_start, &st->bin_fill, &st->sorted, &st->cnt, &st->off, &st->nlj, &st->ilist, &st->box, &st->mapper, &st->inv_mass, &st->goff})
    b->release();
  delete st;
  m.nb_state = nullptr;
}

// Inverse masses by model type: up to 16 types travel by value in the kernel arguments (no upload, no table to keep), more in a small device table that is
// uploaded when its content changes (the masses of a run do not).
struct MassTab { double inv_mass[16]; };
struct MassByValue {
  MassTab t;
  __device__ __forceinline__ double operator()(int mt) const { return t.inv_mass[mt]; }
};
struct MassByTable {
  const double *inv_mass;
  __device__ __forceinline__ double operator()(int mt) const { return inv_mass[mt]; }
};

template <class Mass>
__global__ void k_nve(int mode, int n, double *x, double *v, const double *f, const int *mtype, Mass mass, double dt, double dtf) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3LL * n) return;
  long long i = t / 3;
  double dtfm = dtf * mass(mtype[i]);
  double vv = v[t] + dtfm * f[t];
  v[t] = vv;
  if (mode == 0) x[t] += dt * vv;
}

// first half step + the zero-fill of the force array the coming evaluation accumulates into (rows [0, nall): locals after their force has been
// used, ghosts outright): one launch instead of two in every step of the stand-alone driver
template <class Mass>
__global__ void k_nve_first(int n, int nall, double *x, double *v, double *f, const int *mtype, Mass mass, double dt, double dtf) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3LL * nall) return;
  if (t < 3LL * n) {
    double dtfm = dtf * mass(mtype[t / 3]);
    double vv = v[t] + dtfm * f[t];
    v[t] = vv;
    x[t] += dt * vv;
  }
  f[t] = 0.0;
}
static MassByValue mass_by_value(const double *mass_host, int ntypes) {
  MassByValue mv;
  for (int k = 0; k < 16; ++k) mv.t.inv_mass[k] = k < ntypes ? 1.0 / mass_host[k] : 0.0;
  return mv;
}
// the device table of a model with more than 16 types, current for mass_host (a change waits for the kernels of `s` that still read the old content)
static MassByTable mass_by_table(Model &m, const double *mass_host, int ntypes, hipStream_t s) {
  if (!m.nb_state) m.nb_state = new NbState();
  NbState &st = *(NbState *)m.nb_state;
  std::vector<double> inv((size_t)ntypes);
  for (int k = 0; k < ntypes; ++k) inv[(size_t)k] = 1.0 / mass_host[k];
  if (inv != st.inv_mass_host) {
    AHIP_CHECK(hipStreamSynchronize(s));
    st.inv_mass.reserve(inv.size() * sizeof(double));
    copy_h2d(st.inv_mass.p, inv.data(), inv.size() * sizeof(double));
    st.inv_mass_host = inv;
  }
  return MassByTable{st.inv_mass.as<double>()};
}
void nve_first_step(Model &m, int n, int nall, double *x, double *v, double *f, const int *mtype, const double *mass_host, int ntypes, double dt, double ftm2v,
                    hipStream_t s) {
  if (nall <= 0) return;
  const unsigned B = 256;
  const dim3 G((unsigned)((3LL * nall + B - 1) / B));
  if (ntypes <= 16) {
    const MassByValue mv = mass_by_value(mass_host, ntypes);
    hipLaunchKernelGGL(k_nve_first<MassByValue>, G, dim3(B), 0, s, n, nall, x, v, f, mtype, mv, dt, 0.5 * dt * ftm2v);
  } else {
    const MassByTable mt = mass_by_table(m, mass_host, ntypes, s);
    hipLaunchKernelGGL(k_nve_first<MassByTable>, G, dim3(B), 0, s, n, nall, x, v, f, mtype, mt, dt, 0.5 * dt * ftm2v);
  }
  AHIP_CHECK(hipGetLastError());
}

void nve_step(Model &m, int mode, int n, double *x, double *v, const double *f, const int *mtype, const double *mass_host,
              int ntypes, double dt, double ftm2v, hipStream_t s) {
  if (n <= 0) return;
  const unsigned B = 256;
  const dim3 G((unsigned)((3LL * n + B - 1) / B));
  if (ntypes <= 16) {
    const MassByValue mv = mass_by_value(mass_host, ntypes);
    hipLaunchKernelGGL(k_nve<MassByValue>, G, dim3(B), 0, s, mode, n, x, v, f, mtype, mv, dt, 0.5 * dt * ftm2v);
  } else {
    const MassByTable mt = mass_by_table(m, mass_host, ntypes, s);
    hipLaunchKernelGGL(k_nve<MassByTable>, G, dim3(B), 0, s, mode, n, x, v, f, mtype, mt, dt, 0.5 * dt * ftm2v);
  }
  AHIP_CHECK(hipGetLastError());
}

}  // namespace ahip
