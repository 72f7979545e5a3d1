// Saved-row maps of the wide fused kernels (fused_lx.hip: k_fused_lx, shape ShapeX; fused_lx2.hip: k_fused_lx2, shape ShapeP) as constexpr functions of the
// number of layers NL and the latent-MLP depth MD.  Host- and device-compilable, free of HIP: the kernels, the host driver that sizes the per-wave scratch
// and a stand-alone CPU test (tests/test_fused_lx_rows.py) read the same numbers.
//
// One row = one 16-feature register image of a wave (1 KiB).  Per wave:
//   d x0/dd 4 | w0 EW | per layer: omega EW | hidden layer 1..MD, HR rows each | u UR | V_in NV
// Hidden layers 1..MD-1 hold silu'(z); the last one holds silu'(z) on the f32 instances and the raw z on the f16x2 instances (which then leave the u rows unused).
// MD = 2 gives the maps the kernels have had since round 6.  UR (rows of the layer's output u, 64 scalars wide) defaults to HR: the two differ only on the MLP-width-128
// instances of k_fused_lx, whose hidden layers are 8 rows and whose u stays 4 (RowsXM), and on those of k_fused_lx2: 4 own rows per hidden layer, u 2 (RowsPM).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AHIP_ROWS_HD __host__ __device__
#else
#define AHIP_ROWS_HD
#endif

namespace ahip {

// EW: 16-feature tiles of an (l, u) weight vector held by the wave; HR: rows of one hidden layer held by the wave; NV: rows of its part of the edge tensor; UR: rows of u
template <int EW_, int HR_, int NV_, int UR_ = HR_> struct LxRows {
  static constexpr int EW = EW_, HR = HR_, NV = NV_, UR = UR_;
  static constexpr int R_DX0 = 0, R_W0 = 4, O_OM = 0;
  AHIP_ROWS_HD static constexpr int O_Z(int h) { return EW + HR * (h - 1); }              // hidden layer h = 1..MD (offsets inside a layer's block)
  AHIP_ROWS_HD static constexpr int O_U(int MD) { return EW + HR * MD; }
  AHIP_ROWS_HD static constexpr int O_VIN(int MD) { return EW + HR * MD + UR; }
  AHIP_ROWS_HD static constexpr int LSZ(int MD) { return EW + HR * MD + UR + NV; }
  AHIP_ROWS_HD static constexpr int R_LAYER(int kk, int MD) { return 4 + EW + kk * LSZ(MD); }
  AHIP_ROWS_HD static constexpr int R_TOTAL(int NL, int MD) { return 4 + EW + NL * LSZ(MD); }
};

// k_fused_lx: l_max = 2, 32 tensor features in one wave: (l, u) vectors of 3 x 2 tiles, 4 rows per hidden layer, 9 x 2 tensor rows
using RowsX = LxRows<6, 4, 18>;
// ... with 128-wide hidden layers (8 rows each; u 4 rows)
using RowsXM = LxRows<6, 8, 18, 4>;
// k_fused_lx2: l_max = 2, 64 tensor features over a wave pair: each wave holds 3 x 2 own tiles, 2 own rows per hidden layer, 9 x 2 own tensor rows
using RowsP = LxRows<6, 2, 18>;
// ... with 128-wide hidden layers (4 own rows each; u stays at 2 own rows): R_TOTAL(NL, MD) = 10 + NL (26 + 4 MD), 124 rows for 3 layers at depth 3 against 106
using RowsPM = LxRows<6, 4, 18, 2>;

}  // namespace ahip
