// Saved-row map of k_fused (fused.hip) as constexpr functions of the number of layers NL, the latent-MLP depth MD and the hidden tile count WT (16-feature tiles of
// one hidden layer: 4 = MLP width 64, 8 = MLP width 128, fused_shapes.h: FUSED_WF / FUSED_WF2).  Host- and device-compilable, free of HIP, like fused_lx_rows.h: the
// kernel, the host driver that sizes the per-wave scratch and a stand-alone CPU test (tests/test_fused_mlp_width_shapes.py) read the same numbers.
//
// One row = one 16-feature register image of a wave (1 KiB).  Per wave:
//   two-body rows 16 (d x0/dd 4 | second hidden layer 4 | u0 4 | w0 4; the middle two with fused_tb=mlp only) | per layer: omega 4 | hidden layer 1..MD, WT rows each | u 4 | V_in 8
// Hidden layers 1..MD-1 hold silu'(z); the last one holds silu'(z), or the raw z on the f16x2 instances (which then leave the u rows unused).
// WT = 4, MD = 2 gives the 24 rows per layer the kernel has had since round 3.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AHIP_FROWS_HD __host__ __device__
#else
#define AHIP_FROWS_HD
#endif

namespace ahip {

AHIP_FROWS_HD constexpr int R_Z1TB() { return 0; }
AHIP_FROWS_HD constexpr int R_Z2TB() { return 4; }
AHIP_FROWS_HD constexpr int R_U0() { return 8; }
AHIP_FROWS_HD constexpr int R_W0() { return 12; }
// offsets inside a layer's block: hidden layer h = 1..MD, u, V_in
AHIP_FROWS_HD constexpr int R_OZ(int h, int WT = 4) { return 4 + WT * (h - 1); }
AHIP_FROWS_HD constexpr int R_OU(int MD, int WT = 4) { return 4 + WT * MD; }
AHIP_FROWS_HD constexpr int R_OVIN(int MD, int WT = 4) { return 8 + WT * MD; }
AHIP_FROWS_HD constexpr int R_LSZ(int MD, int WT = 4) { return 16 + WT * MD; }
AHIP_FROWS_HD constexpr int R_LAYER(int kk, int MD = 2, int WT = 4) { return 16 + R_LSZ(MD, WT) * kk; }
AHIP_FROWS_HD constexpr int R_TOTAL(int NL, int MD = 2, int WT = 4) { return 16 + R_LSZ(MD, WT) * NL; }

}  // namespace ahip
