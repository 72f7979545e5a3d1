// Which fused kernel serves a model, at which shape, and why not: the shape rule of the fused side in one place.  Host-only and free of HIP and of the
// engine's Model (like arith_policy.h and fused_lx_rows.h): the gates of the kernel files (fused_model_supported, fusedlx_model_supported), the dispatch of
// the C-ABI (allegro_hip.hip: fused_family, run_model_once), the padding of engine.h (fused_host_model) and a stand-alone CPU test (tests/test_fused_shapes.py)
// read the same rules.
//
//   family    kernel        runs at                   serves
//   k_fused   k_fused       l_max 1, 32 features      l_max = 1, U <= 32
//   lx32      k_fused_lx    l_max 2, 32 features      l_max = 2, U <= 32
//   lx64      k_fused_lx2   l_max 2, 64 features      l_max = 2, 33 <= U <= 64;  l_max = 1, 33 <= U <= 64 (lifted: model_io.h, lift_host_model)
// all with S <= 64 scalars, MLP width <= 64 (k_fused and lx32 also 65..128, lx64 behind option lx64_mlp_width=auto: the width classes below), read-out width <= 64 (two width classes, below; narrower models run zero-padded: pad_host_model), 1..3 layers, <= 16 ACTIVE types.
//
// Width classes of the latent MLP (WF = the hidden width an instance runs at; the two-body MLP shares the model's mlp_width and is tabulated on the host):
//   WF = 64    mlp_width <= 64          every family, every instance below
//   WF = 128   65 <= mlp_width <= 128   k_fused and lx32 only, zero-padded to 128: f16x2 arithmetic (k_fused: with the tabulated two-body embedding), MLP depth 1..3,
//                                       read-out depth 1, plain and per-atom-virial variants, both tile shapes of k_fused, the 64-slot shape of k_fused_lx
//              the same                 lx64 behind option lx64_mlp_width=auto (the gates' trailing argument lx64_w128; default "64": refused): the same limits,
//                                       allow_tf32 = 0, the one tile shape of k_fused_lx2
// Width classes of the read-out MLP (RF = the width its hidden layers run at):
//   RF = 32    readout_width <= 32          every family, every instance above
//   RF = 64    33 <= readout_width <= 64    every family, zero-padded to 64: f16x2 arithmetic (k_fused: with the tabulated two-body embedding), MLP width <= 64 (WF = 64), MLP depth 1..3,
//                                           read-out depth 1, plain and per-atom-virial variants, both tile shapes of k_fused, the 64-slot shape of k_fused_lx, the one shape of k_fused_lx2
// S and the tensor features have one class each; lx64 (33..64 tensor features) runs its WF = 128 instances under option lx64_mlp_width=auto only; no instance combines WF = 128 with RF = 64.
//
// Active types: the model types the caller's type mapping can produce (engine.h: Model::active).  A fused evaluation runs on the model restricted to them
// (model_io.h: subset_host_model; compact slots 0 .. A - 1 in ascending model-type order, 4 bits each in the packed edge types), so the gates count A, not the
// model's T: a 20-type model mapped to three elements qualifies.  T <= 255 because the full -> compact table on the device holds bytes (0xFF = inactive).  The gates take
// A as a trailing argument; a caller that leaves it out gets A = T.
//
// Instances by (MD, RD) = (latent MLP depth, read-out depth): (2, 1) on every arithmetic the family has; every other pair of MD in 1..3, RD in 1..2 on the
// f16x2 arithmetic only (k_fused: with the tabulated two-body embedding).  Read-out depth 0 (a linear read-out) would need a different fold of the last
// layer's output linear into the read-out and has no instance.
//
// Tile shapes of the wide kernels (edge slots, centres per tile); a centre with more edges than the model's largest shape holds is "heavy":
//   lx32, lx64   4 waves (lx64: 4 wave pairs)   64 slots, 4 centres    every instance
//   lx32         8 waves                       128 slots, 8 centres    (MD, RD) = (2, 1) on f32 and f16x2, behind option wide_tile=auto (fused_has_wide_tile)
#pragma once
#include <string>

#include "arith_policy.h"
#include "model_io.h"

namespace ahip {

enum class FusedFamily { none, k_fused, lx32, lx64 };
inline const char *fused_family_name(FusedFamily f) {
  return f == FusedFamily::k_fused ? "k_fused" : f == FusedFamily::lx32 ? "lx32" : f == FusedFamily::lx64 ? "lx64" : "none";
}
inline bool fused_is_wide(FusedFamily f) { return f == FusedFamily::lx32 || f == FusedFamily::lx64; }

// the kernels' fixed widths: scalars, MLP width, read-out width (all families); tensor features and l_max per family
inline constexpr int FUSED_SF = 64, FUSED_WF = 64, FUSED_RF = 32;
inline constexpr int FUSED_WF2 = 128;       // the second hidden width of the latent MLP (k_fused, lx32; see the head of this file)
// the width class a model's latent MLP runs at
inline int fused_WF(const HostModel &h) { return h.mlp_width > FUSED_WF ? FUSED_WF2 : FUSED_WF; }
inline constexpr int FUSED_RF2 = 64;        // the second width of the read-out MLP (every family; see the head of this file)
// the width class a model's read-out MLP runs at
inline int fused_RF(const HostModel &h) { return h.readout_width > FUSED_RF ? FUSED_RF2 : FUSED_RF; }
inline int fused_UF(FusedFamily f) { return f == FusedFamily::lx64 ? 64 : 32; }
inline int fused_l_run(FusedFamily f) { return f == FusedFamily::k_fused ? 1 : 2; }

// The family whose SHAPE (l_max, tensor features) the model has, whatever its depths and the arithmetic: it decides the padded / lifted model, the tile
// shape and the heavy-centre threshold.  none: no fused kernel holds this l_max / this many tensor features.
inline FusedFamily fused_shape_class(const HostModel &h) {
  if (h.U < 1 || h.U > 64) return FusedFamily::none;
  if (h.l_max == 1) return h.U <= 32 ? FusedFamily::k_fused : FusedFamily::lx64;
  if (h.l_max == 2) return h.U <= 32 ? FusedFamily::lx32 : FusedFamily::lx64;
  return FusedFamily::none;
}
// S, MLP width, read-out width and tensor features within the fixed widths of k_fused (wide = false) or of the wide kernels
// (WF, RF: the width classes, FUSED_WF or FUSED_WF2, FUSED_RF or FUSED_RF2)
inline bool fused_widths_fit(const HostModel &h, bool wide, int WF = FUSED_WF, int RF = FUSED_RF) {
  return h.S >= 1 && h.S <= FUSED_SF && h.mlp_width >= 1 && h.mlp_width <= WF && h.readout_width >= 1 && h.readout_width <= RF && h.U >= 1 &&
         h.U <= (wide ? 64 : 32);
}
// the model is already at family f's shape: nothing to pad or lift
inline bool fused_shape_exact(const HostModel &h, FusedFamily f, int WF = FUSED_WF, int RF = FUSED_RF) {
  return h.S == FUSED_SF && h.mlp_width == WF && h.readout_width == RF && h.U == fused_UF(f) && h.l_max == fused_l_run(f);
}
// the model at family f's shape: lifted to the family's l_max where it is lower, then zero-padded
inline HostModel fused_shaped_model(const HostModel &h, FusedFamily f, int WF = FUSED_WF, int RF = FUSED_RF) {
  return pad_host_model(lift_host_model(h, fused_l_run(f)), FUSED_SF, fused_UF(f), WF, RF);
}

// a compiled instance of family f exists for this arithmetic (k_fused: and two-body mode) and these depths
// (WF: the width class of the latent MLP; the WF = 128 instances: k_fused and lx32 -- lx64 too where lx64_w128 says so (option lx64_mlp_width=auto) --, f16x2, read-out depth 1.  RF: the width class of the read-out MLP; the RF = 64
// instances: every family, f16x2, WF = 64, read-out depth 1)
inline bool fused_instance_exists(FusedFamily f, Arith ar, bool tb_table, int MD, int RD, int WF = FUSED_WF, int RF = FUSED_RF, bool lx64_w128 = false) {
  if (f == FusedFamily::none || MD < 1 || MD > 3 || RD < 1 || RD > 2) return false;
  if (RF == FUSED_RF2) return WF == FUSED_WF && ar == AR_F16X2 && RD == 1 && (fused_is_wide(f) || tb_table);
  if (RF != FUSED_RF) return false;
  if (WF == FUSED_WF2) return (f == FusedFamily::k_fused || f == FusedFamily::lx32 || (f == FusedFamily::lx64 && lx64_w128)) && ar == AR_F16X2 && RD == 1 && (fused_is_wide(f) || tb_table);
  if (WF != FUSED_WF) return false;
  if (MD == 2 && RD == 1) return fused_is_wide(f) ? (ar == AR_F32 || ar == AR_F16X2) : (ar != AR_F16X2 || tb_table);
  return ar == AR_F16X2 && (fused_is_wide(f) || tb_table);
}

// The second tile shape of k_fused_lx (8 waves, 128 edge slots: a centre with 65..128 edges stays on the fused kernel) exists for this family, arithmetic and
// these depths.  Option wide_tile=auto uses it where this says yes and is the 64-slot shape everywhere else.
// (the WF = 128 and the RF = 64 instances have the 64-slot shape only: wide_tile=auto is "64" for them)
inline bool fused_has_wide_tile(FusedFamily f, Arith ar, int MD, int RD, int WF = FUSED_WF, int RF = FUSED_RF) {
  return f == FusedFamily::lx32 && (ar == AR_F32 || ar == AR_F16X2) && MD == 2 && RD == 1 && WF == FUSED_WF && RF == FUSED_RF;
}
// edge slots and centres of a wide kernel's tile: the 4-wave shape of every instance, or the 8-wave shape of k_fused_lx (8 centres: 16 slots per centre as in the
// 4-wave shape -- lists that need it are dense, two 54-edge centres or one of 78 fill a tile -- and the environment rows of 8 centres leave its LDS at 153 392 B of 160 KB)
inline constexpr int lx_tile_slots(bool wide128) { return wide128 ? 128 : 64; }
inline constexpr int lx_tile_maxa(bool wide128) { return wide128 ? 8 : 4; }

// the refusals of the WF = 128 width class
inline constexpr const char *FUSED_WHY_W128_ARITH_NARROW =
    "MLP width 65..128 runs on the f16x2 arithmetic with the tabulated two-body embedding only (fused_arith=auto|f16x2, fused_tb=table, allow_tf32 = 0)";
inline constexpr const char *FUSED_WHY_W128_ARITH_WIDE = "MLP width 65..128 runs on the f16x2 arithmetic only on the wide fused kernels (fused_arith=auto|f16x2)";
inline constexpr const char *FUSED_WHY_W128_RD = "MLP width 65..128 runs with read-out depth 1 only on the fused kernels (read-out depth 2 has instances of MLP width <= 64 only)";
inline constexpr const char *FUSED_WHY_W128_LX64 =
    "MLP width 65..128 has no instance of the wide fused kernel for 33..64 tensor features (k_fused_lx2 holds MLP width 64; k_fused and k_fused_lx hold 128 with up to 32 tensor features)";
// ... behind option lx64_mlp_width=auto: a TF32-licensed model stays refused.  The first-evaluation self-check of fused_arith=auto does not run for such a model
// (allegro_hip.hip: run_model), and these f16x2-only instances have no float32 twin to be compared with or to fall back to but the layer-at-a-time kernels.
inline constexpr const char *FUSED_WHY_W128_LX64_TF32 =
    "MLP width 65..128 with 33..64 tensor features (option lx64_mlp_width=auto) runs on the f16x2 arithmetic for models with allow_tf32 = 0 only";

// the refusals of the RF = 64 width class of the read-out
inline constexpr const char *FUSED_WHY_R64_ARITH_NARROW =
    "read-out width 33..64 runs on the f16x2 arithmetic with the tabulated two-body embedding only (fused_arith=auto|f16x2, fused_tb=table, allow_tf32 = 0)";
inline constexpr const char *FUSED_WHY_R64_ARITH_WIDE = "read-out width 33..64 runs on the f16x2 arithmetic only on the wide fused kernels (fused_arith=auto|f16x2)";
inline constexpr const char *FUSED_WHY_R64_RD = "read-out width 33..64 runs with read-out depth 1 only on the fused kernels (read-out depth 2 has instances of read-out width <= 32 only)";
inline constexpr const char *FUSED_WHY_R64_W128 =
    "read-out width 33..64 has no fused instance with MLP width 65..128 (the instances of read-out width 64 hold MLP width 64; those of MLP width 128 hold read-out width 32)";

inline constexpr const char *FUSED_WHY_DEPTHS =
    "fused kernels need MLP depth 1..3 and read-out depth 1..2 (a linear read-out, depth 0, needs a different fold of the last layer and has no instance)";

// The type gate of every family.  n_active: the number of active types (see the head of this file), -1 = all of the model's.  The packed edge types hold two
// 4-bit slots, the full -> compact table on the device one byte per model type.
inline constexpr int FUSED_MAX_ACTIVE = 16, FUSED_MAX_TYPES = 255;
inline bool fused_types_fit(const HostModel &h, int n_active, std::string *why) {
  const int T = h.num_types, A = n_active < 0 ? T : n_active;
  if (A != T && T > FUSED_MAX_TYPES) {
    if (why) *why = "fused kernels on a subset of the types need a model of at most 255 types (byte table full -> compact type; this model has " + std::to_string(T) + ")";
    return false;
  }
  if (A > FUSED_MAX_ACTIVE) {
    if (why) *why = "fused kernels support at most 16 active model types (" + std::to_string(A) + " of the model's " + std::to_string(T) + " are mapped)";
    return false;
  }
  return true;
}

// k_fused's gate: `arith` is the arithmetic the model's options resolve to on k_fused (resolve_arith, wide = false)
inline bool fused_narrow_supported(const HostModel &h, Arith arith, bool tb_table, std::string *why, int n_active = -1) {
  auto no = [&](const char *msg) { if (why) *why = msg; return false; };
  if (h.l_max != 1) return no("fused kernels need l_max = 1");
  if (!fused_widths_fit(h, false, FUSED_WF2, FUSED_RF2))
    return no("fused kernels hold at most U=32, S=64, MLP width 128 (65..128: f16x2 instances, read-out depth 1), read-out width 64 (33..64: f16x2 instances, MLP width <= 64, read-out depth 1; narrower models run zero-padded)");
  if (h.mlp_depth < 1 || h.mlp_depth > 3 || h.readout_depth < 1 || h.readout_depth > 2) return no(FUSED_WHY_DEPTHS);
  if (fused_RF(h) == FUSED_RF2) {   // the wider read-out: f16x2 instances with the tabulated two-body embedding, MLP width <= 64, read-out depth 1 (template parameter RT of k_fused)
    if (fused_WF(h) == FUSED_WF2) return no(FUSED_WHY_R64_W128);
    if (arith != AR_F16X2) return no(FUSED_WHY_R64_ARITH_NARROW);
    if (h.readout_depth != 1) return no(FUSED_WHY_R64_RD);
  }
  if (fused_WF(h) == FUSED_WF2) {   // the wider hidden layers: f16x2 instances with the tabulated two-body embedding, read-out depth 1 (template parameter WT of k_fused)
    if (arith != AR_F16X2) return no(FUSED_WHY_W128_ARITH_NARROW);
    if (h.readout_depth != 1) return no(FUSED_WHY_W128_RD);
  }
  if (h.mlp_depth != 2) {           // depth 1 and 3 on the f16x2 instances with the tabulated two-body embedding
    if (arith != AR_F16X2) return no("MLP depth 1 / 3 runs on the f16x2 arithmetic with the tabulated two-body embedding only (fused_arith=auto|f16x2, fused_tb=table, allow_tf32 = 0)");
  }
  if (h.readout_depth == 2) {       // likewise (template parameter RD of k_fused)
    if (arith != AR_F16X2) return no("read-out depth 2 runs on the f16x2 arithmetic with the tabulated two-body embedding only (fused_arith=auto|f16x2, fused_tb=table, allow_tf32 = 0)");
  }
  // the radial basis only enters through the two-body embedding: tabulated (default) any number of Bessel functions will do, evaluated in the kernel
  // (fused_tb=mlp) its first linear is laid out for 8
  if (h.num_bessels < 1 || (!tb_table && h.num_bessels != 8)) return no("fused_tb=mlp needs 8 Bessel functions (the tabulated two-body embedding takes any number)");
  if (h.num_layers < 1 || h.num_layers > 3) return no("fused kernels need 1..3 layers");
  if (!fused_types_fit(h, n_active, why)) return false;
  return true;
}

// the wide kernels' gate: `arith` is what the options resolve to on them (resolve_arith, wide = true); lx64_w128: option lx64_mlp_width=auto (the WF = 128
// instances of k_fused_lx2; a caller that leaves it out gets the default of the option, "64")
inline bool fused_wide_supported(const HostModel &h, Arith arith, std::string *why, int n_active = -1, bool lx64_w128 = false) {
  auto no = [&](const char *msg) { if (why) *why = msg; return false; };
  if (h.l_max != 2 && !(h.l_max == 1 && h.U > 32)) return no("wide fused kernels are built for l_max = 2 (an l_max = 1 model runs on them lifted when it has 33..64 tensor features)");
  if (!fused_widths_fit(h, true, FUSED_WF2, FUSED_RF2))
    return no("wide fused kernels hold at most 64 tensor features, S=64, MLP width 128 (65..128: up to 32 tensor features, f16x2 instances, read-out depth 1), read-out width 64 (33..64: f16x2 instances, MLP width <= 64, read-out depth 1; narrower models run zero-padded)");
  if (h.mlp_depth < 1 || h.mlp_depth > 3 || h.readout_depth < 1 || h.readout_depth > 2) return no(FUSED_WHY_DEPTHS);
  if (fused_RF(h) == FUSED_RF2) {   // the wider read-out: both wide kernels (template parameter RT), f16x2, MLP width <= 64, read-out depth 1
    if (fused_WF(h) == FUSED_WF2) return no(FUSED_WHY_R64_W128);
    if (arith != AR_F16X2) return no(FUSED_WHY_R64_ARITH_WIDE);
    if (h.readout_depth != 1) return no(FUSED_WHY_R64_RD);
  }
  if (fused_WF(h) == FUSED_WF2) {   // the wider hidden layers: k_fused_lx (template parameter HT), k_fused_lx2 behind its option (template parameter WH), f16x2, read-out depth 1
    if (fused_shape_class(h) != FusedFamily::lx32) {
      if (!lx64_w128) return no(FUSED_WHY_W128_LX64);
      if (h.allow_tf32) return no(FUSED_WHY_W128_LX64_TF32);
    }
    if (arith != AR_F16X2) return no(FUSED_WHY_W128_ARITH_WIDE);
    if (h.readout_depth != 1) return no(FUSED_WHY_W128_RD);
  }
  if (h.mlp_depth != 2) {           // depth 1 and 3 on the f16x2 instances (template parameter MD of both wide kernels)
    if (arith != AR_F16X2) return no("MLP depth 1 / 3 runs on the f16x2 arithmetic only on the wide fused kernels (fused_arith=auto|f16x2)");
  }
  if (h.readout_depth == 2) {       // likewise (template parameter RD)
    if (arith != AR_F16X2) return no("read-out depth 2 runs on the f16x2 arithmetic only on the wide fused kernels (fused_arith=auto|f16x2)");
  }
  if (h.num_bessels < 1) return no("no radial basis");      // any number of Bessel functions: the two-body embedding is always tabulated here
  if (h.num_layers < 1 || h.num_layers > 3) return no("fused kernels need 1..3 layers");
  if (!fused_types_fit(h, n_active, why)) return false;
  return true;
}

// The decision for a model: the family that serves it (none: `why` holds the reasons of both gates), the shape it runs at and the arithmetic of its instance.
struct FusedDecision {
  FusedFamily family = FusedFamily::none;
  int l_run = 0, UF = 0;            // l_max and tensor features of the kernel (the model runs lifted / zero-padded to them)
  int WF = 0;                       // hidden width of the latent MLP the instance runs at: FUSED_WF or FUSED_WF2
  int RF = 0;                       // width of the read-out MLP the instance runs at: FUSED_RF or FUSED_RF2
  Arith arith = AR_F32;
  std::string why;
};
inline FusedDecision fused_decide(const HostModel &h, Arith arith_narrow, Arith arith_wide, bool tb_table, int n_active = -1, bool lx64_w128 = false) {
  FusedDecision d;
  std::string why1, why2;
  if (fused_narrow_supported(h, arith_narrow, tb_table, &why1, n_active)) { d.family = FusedFamily::k_fused; d.arith = arith_narrow; }
  else if (fused_wide_supported(h, arith_wide, &why2, n_active, lx64_w128)) { d.family = fused_shape_class(h); d.arith = arith_wide; }
  else { d.why = why1 + "; " + why2; return d; }
  d.l_run = fused_l_run(d.family); d.UF = fused_UF(d.family); d.WF = fused_WF(h); d.RF = fused_RF(h);
  return d;
}
// the same from an effective option (arith_effective) and the state of fused_arith=auto
inline FusedDecision fused_decide(const HostModel &h, ArithOpt opt, bool degraded, bool force_f32, bool tb_table, int n_active = -1, bool lx64_w128 = false) {
  return fused_decide(h, resolve_arith(opt, h.allow_tf32 != 0, degraded, force_f32, tb_table, false), resolve_arith(opt, h.allow_tf32 != 0, degraded, force_f32, tb_table, true), tb_table, n_active, lx64_w128);
}

}  // namespace ahip
