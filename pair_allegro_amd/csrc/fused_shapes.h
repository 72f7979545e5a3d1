// Which fused kernel serves a model, at which shape, and why not: the shape rule of the fused side in one place.  Host-only and free of HIP and of the
// engine's Model (like arith_policy.h and fused_lx_rows.h): the gates of the kernel files (fused_model_supported, fusedlx_model_supported), their instance
// dispatch, the dispatch of the C-ABI (allegro_hip.hip: fused_family, run_model_once), the padding of engine.h (fused_host_model) and stand-alone CPU tests
// (tests/test_fused_shapes.py, tests/test_fused_instance_table.py) read the same rules.
//
//   family    kernel        runs at                   serves
//   k_fused   k_fused       l_max 1, 32 features      l_max = 1, U <= 32
//   lx32      k_fused_lx    l_max 2, 32 features      l_max = 2, U <= 32
//   lx64      k_fused_lx2   l_max 2, 64 features      l_max = 2, 33 <= U <= 64;  l_max = 1, 33 <= U <= 64 (lifted: model_io.h, lift_host_model)
// all with S <= 64 scalars, 1..3 layers, <= 16 ACTIVE types.  WHICH INSTANCES ARE COMPILED, and into which object, is the table FUSED_INSTANCES below and nowhere else: the
// gates, the launch switches of the kernel files and the static_asserts of their dispatch lists read it, and csrc/Makefile has one line per (source, part) of it.
//
// Width classes: WF = the hidden width the latent MLP runs at (64, or 128 for 65 <= mlp_width <= 128; the two-body MLP shares the model's mlp_width and is tabulated on the host),
// RF = the width the read-out MLP's hidden layers run at (32, or 64 for 33 <= readout_width <= 64); a narrower model runs zero-padded (pad_host_model).  S and the tensor features have one class each.
//
// Active types: the model types the caller's type mapping can produce (engine.h: Model::active).  A fused evaluation runs on the model restricted to them
// (model_io.h: subset_host_model; compact slots 0 .. A - 1 in ascending model-type order, 4 bits each in the packed edge types), so the gates count A, not the
// model's T: a 20-type model mapped to three elements qualifies.  T <= 255 because the full -> compact table on the device holds bytes (0xFF = inactive).  The gates take
// A as a trailing argument; a caller that leaves it out gets A = T.
//
// Read-out depth 0 (a linear read-out) would need a different fold of the last layer's output linear into the read-out and has no instance.
//
// Tile shapes (the table's `tile`, in units of 16 edge slots: waves of k_fused and k_fused_lx, wave pairs of k_fused_lx2): 4 = 64 slots (k_fused: <= 6 centres, the wide
// kernels: 4), 8 = 128 slots (k_fused: <= 12 centres; k_fused_lx: 8, behind option wide_tile=auto: fused_has_wide_tile).  A centre with more edges than the model's
// largest shape holds is "heavy".
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>

#include "arith_policy.h"
#include "model_io.h"

namespace ahip {

// the engine's error types (here, not in engine.h, so that host-only code can throw them)
struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };
struct StateError : std::runtime_error { using std::runtime_error::runtime_error; };
struct UnsupportedError : std::runtime_error { using std::runtime_error::runtime_error; };

enum class FusedFamily { none, k_fused, lx32, lx64 };
inline const char *fused_family_name(FusedFamily f) {
  return f == FusedFamily::k_fused ? "k_fused" : f == FusedFamily::lx32 ? "lx32" : f == FusedFamily::lx64 ? "lx64" : "none";
}
inline constexpr bool fused_is_wide(FusedFamily f) { return f == FusedFamily::lx32 || f == FusedFamily::lx64; }

// the kernels' fixed widths: scalars, MLP width, read-out width (all families); tensor features and l_max per family
inline constexpr int FUSED_SF = 64, FUSED_WF = 64, FUSED_RF = 32;
inline constexpr int FUSED_WF2 = 128;       // the second hidden width of the latent MLP (see the head of this file)
// the width class a model's latent MLP runs at
inline int fused_WF(const HostModel &h) { return h.mlp_width > FUSED_WF ? FUSED_WF2 : FUSED_WF; }
inline constexpr int FUSED_RF2 = 64;        // the second width of the read-out MLP (see the head of this file)
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

// instrumentation variant of a fused kernel instance: plain, phase-profiled, or with the per-atom virial (output "atomic_virial"; no profiled twin)
enum { VAR_PLAIN = 0, VAR_PROF = 1, VAR_VA = 2 };
static inline int fused_variant(bool vatom, bool prof) { return vatom ? VAR_VA : prof ? VAR_PROF : VAR_PLAIN; }

// ---- the instance table ----
// One row per (object, arithmetic group): every kernel instance the library compiles is the product of a row's sets, and nothing else is compiled (the
// static_asserts of the kernel files' dispatch lists; tests/test_fused_instance_table.py compares the table with the symbols of every object).  Sets are bit masks
// over the values themselves (fi_bits).  The profiled variant is narrower than the product: latent MLP depth FUSED_PROF_MD only, and the layer counts of prof_nl.
struct FusedInstanceRow {
  FusedFamily family;
  const char *source; int part; const char *object;      // compiled from `source` with its part macro (AHIP_FUSED_PART, AHIP_LX_PART) = part into <object>.o (csrc/Makefile)
  unsigned ar;              // arithmetics (arith_policy.h: Arith)
  unsigned tb;              // two-body modes of k_fused: 1 = from the spline table, 0 = evaluated in the kernel (fused_tb=mlp); the wide kernels tabulate and take either
  unsigned md;              // latent MLP depths
  int RD, WF, RF;           // read-out depth, width classes
  unsigned tile, nl, var;   // tile shapes (the head of this file), layer counts, variants (VAR_*)
  unsigned prof_nl;         // layer counts of the profiled variant
  bool lx64_w128;           // behind option lx64_mlp_width=auto (the gates' trailing argument; default "64": refused)
};
inline constexpr int FUSED_PROF_MD = 2;
constexpr unsigned fi_bits(int a, int b = -1, int c = -1) { return (1u << a) | (b < 0 ? 0u : 1u << b) | (c < 0 ? 0u : 1u << c); }
constexpr bool fi_has(unsigned set, int v) { return v >= 0 && v < 32 && ((set >> v) & 1u); }
inline constexpr unsigned FI_F32 = fi_bits(AR_F32), FI_BF = fi_bits(AR_BF16X3, AR_TF32EQ), FI_H = fi_bits(AR_F16X2), FI_TABLE = fi_bits(1), FI_ANYTB = fi_bits(0, 1),
                          FI_D2 = fi_bits(2), FI_123 = fi_bits(1, 2, 3), FI_T4 = fi_bits(4), FI_T8 = fi_bits(8), FI_VARS = fi_bits(VAR_PLAIN, VAR_PROF, VAR_VA),
                          FI_NOPROF = fi_bits(VAR_PLAIN, VAR_VA), FI_NL3 = fi_bits(3);
inline constexpr FusedInstanceRow FUSED_INSTANCES[] = {
    // family             source          part object        arithmetic      two-body  MD      RD  WF   RF  tiles          layers  variants   profiled  option
    {FusedFamily::k_fused, "fused.hip",     0, "fused",       FI_F32,         FI_ANYTB, FI_D2,  1,  64,  32, FI_T4 | FI_T8, FI_123, FI_VARS,   FI_123,   false},
    {FusedFamily::k_fused, "fused.hip",     1, "fused_bf",    FI_BF,          FI_ANYTB, FI_D2,  1,  64,  32, FI_T4 | FI_T8, FI_123, FI_VARS,   FI_123,   false},
    {FusedFamily::k_fused, "fused.hip",     2, "fused_h",     FI_H,           FI_TABLE, FI_123, 1,  64,  32, FI_T4 | FI_T8, FI_123, FI_VARS,   FI_123,   false},
    {FusedFamily::k_fused, "fused.hip",     3, "fused_hr",    FI_H,           FI_TABLE, FI_123, 2,  64,  32, FI_T4 | FI_T8, FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::k_fused, "fused.hip",     4, "fused_hm",    FI_H,           FI_TABLE, FI_123, 1,  128, 32, FI_T4 | FI_T8, FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::k_fused, "fused.hip",     5, "fused_hq",    FI_H,           FI_TABLE, FI_123, 1,  64,  64, FI_T4 | FI_T8, FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx32,    "fused_lx.hip",  0, "fused_lx",    FI_F32,         FI_ANYTB, FI_D2,  1,  64,  32, FI_T4,         FI_123, FI_VARS,   FI_NL3,   false},
    {FusedFamily::lx32,    "fused_lx.hip",  0, "fused_lx",    FI_H,           FI_ANYTB, FI_123, 1,  64,  32, FI_T4,         FI_123, FI_VARS,   FI_NL3,   false},
    {FusedFamily::lx32,    "fused_lx.hip",  1, "fused_lx_r",  FI_H,           FI_ANYTB, FI_123, 2,  64,  32, FI_T4,         FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx32,    "fused_lx.hip",  2, "fused_lx_w",  FI_F32 | FI_H,  FI_ANYTB, FI_D2,  1,  64,  32, FI_T8,         FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx32,    "fused_lx.hip",  3, "fused_lx_m",  FI_H,           FI_ANYTB, FI_123, 1,  128, 32, FI_T4,         FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx32,    "fused_lx.hip",  4, "fused_lx_q",  FI_H,           FI_ANYTB, FI_123, 1,  64,  64, FI_T4,         FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx64,    "fused_lx2.hip", 0, "fused_lx2",   FI_F32,         FI_ANYTB, FI_D2,  1,  64,  32, FI_T4,         FI_123, FI_VARS,   FI_NL3,   false},
    {FusedFamily::lx64,    "fused_lx2.hip", 0, "fused_lx2",   FI_H,           FI_ANYTB, FI_123, 1,  64,  32, FI_T4,         FI_123, FI_VARS,   FI_NL3,   false},
    {FusedFamily::lx64,    "fused_lx2.hip", 1, "fused_lx2_r", FI_H,           FI_ANYTB, FI_123, 2,  64,  32, FI_T4,         FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx64,    "fused_lx2.hip", 2, "fused_lx2_q", FI_H,           FI_ANYTB, FI_123, 1,  64,  64, FI_T4,         FI_123, FI_NOPROF, 0,        false},
    {FusedFamily::lx64,    "fused_lx2.hip", 3, "fused_lx2_m", FI_H,           FI_ANYTB, FI_123, 1,  128, 32, FI_T4,         FI_123, FI_NOPROF, 0,        true},
};

// What a lookup asks for.  tile, NL and var may stay open (0, 0, -1: any).
struct FusedInstanceKey {
  FusedFamily f; int ar; bool tb_table;
  int MD, RD, WF = FUSED_WF, RF = FUSED_RF;
  bool lx64_w128 = false;
  int tile = 0, NL = 0, var = -1;
};
// The first row that holds the key, nullptr when none does.  `fields` narrows the comparison of arithmetic (with the two-body mode), depths and width classes to some of
// them: "has the family any row of this width class on this arithmetic" is how the gates find the field to blame.
enum : unsigned { FQ_AR = 1, FQ_MD = 2, FQ_RD = 4, FQ_WF = 8, FQ_RF = 16, FQ_ALL = 31 };
constexpr const FusedInstanceRow *fused_find_instance(const FusedInstanceKey &k, unsigned fields = FQ_ALL) {
  for (const FusedInstanceRow &r : FUSED_INSTANCES) {
    if (r.family != k.f || (r.lx64_w128 && !k.lx64_w128)) continue;
    if ((fields & FQ_AR) && !(fi_has(r.ar, k.ar) && fi_has(r.tb, k.tb_table))) continue;
    if (((fields & FQ_MD) && !fi_has(r.md, k.MD)) || ((fields & FQ_RD) && r.RD != k.RD) || ((fields & FQ_WF) && r.WF != k.WF) || ((fields & FQ_RF) && r.RF != k.RF)) continue;
    if ((k.tile && !fi_has(r.tile, k.tile)) || (k.NL && !fi_has(r.nl, k.NL)) || (k.var >= 0 && !fi_has(r.var, k.var))) continue;
    if (k.var == VAR_PROF && (k.MD != FUSED_PROF_MD || (k.NL && !fi_has(r.prof_nl, k.NL)))) continue;
    return &r;
  }
  return nullptr;
}
// the fully named instance is in the table and lives in this part of its source file (the static_asserts of the dispatch lists)
constexpr bool fused_part_holds(int part, const FusedInstanceKey &k) { return k.tile && k.NL && k.var >= 0 && fused_find_instance(k) && fused_find_instance(k)->part == part; }
// the row of a prepared model's instance; a model the gates should have kept away is an error, never another instance
inline const FusedInstanceRow &fused_require_instance(const FusedInstanceKey &k) {
  if (const FusedInstanceRow *r = fused_find_instance(k)) return *r;
  throw UnsupportedError(std::string("no compiled fused kernel instance: family ") + fused_family_name(k.f) + ", arithmetic " + fused_path_name((Arith)k.ar) + ", two-body " +
                         (k.tb_table ? "table" : "mlp") + ", MLP depth " + std::to_string(k.MD) + ", read-out depth " + std::to_string(k.RD) + ", MLP width " + std::to_string(k.WF) +
                         ", read-out width " + std::to_string(k.RF) + ", tile of " + std::to_string(16 * k.tile) + " slots (0: any)");
}

// a compiled instance of family f exists for this arithmetic (k_fused: and two-body mode), these depths and width classes (lx64_w128: option lx64_mlp_width=auto)
inline bool fused_instance_exists(FusedFamily f, Arith ar, bool tb_table, int MD, int RD, int WF = FUSED_WF, int RF = FUSED_RF, bool lx64_w128 = false) {
  return fused_find_instance({f, ar, tb_table, MD, RD, WF, RF, lx64_w128}) != nullptr;
}

// The second tile shape of k_fused_lx (8 waves, 128 edge slots: a centre with 65..128 edges stays on the fused kernel) exists for this family, arithmetic and
// these depths.  Option wide_tile=auto uses it where this says yes and is the 64-slot shape everywhere else.
inline bool fused_has_wide_tile(FusedFamily f, Arith ar, int MD, int RD, int WF = FUSED_WF, int RF = FUSED_RF) {
  return fused_is_wide(f) && fused_find_instance({f, ar, true, MD, RD, WF, RF, true, 8}) != nullptr;
}
// edge slots and centres of a wide kernel's tile: the 4-wave shape of every instance, or the 8-wave shape of k_fused_lx (8 centres: 16 slots per centre as in the
// 4-wave shape -- lists that need it are dense, two 54-edge centres or one of 78 fill a tile -- and the environment rows of 8 centres leave its LDS at 153 392 B of 160 KB)
inline constexpr int lx_tile_slots(bool wide128) { return wide128 ? 128 : 64; }
inline constexpr int lx_tile_maxa(bool wide128) { return wide128 ? 8 : 4; }

// ---- instance dispatch (host side) ----
// dispatch<Choices<4, 8>, Choices<1, 2, 3>>(f, nw, nl) calls f(std::integral_constant<int, NW>{}, std::integral_constant<int, NL>{}): every run-time value
// becomes the template argument equal to it, so a kernel instance exists exactly for what the choice lists name.  A value that is in none of its choices is a
// StateError: nothing runs on another instance.
template <int... Vs> struct Choices {};
template <class... Sets> struct Dispatch;
template <> struct Dispatch<> {
  template <class F, class... C> static void run(F &f, const int *, C... c) { f(c...); }
};
template <class... Rest> struct Dispatch<Choices<>, Rest...> {
  template <class F, class... C> static void run(F &, const int *v, C...) { throw StateError("instance dispatch: " + std::to_string(*v) + " is none of the compiled choices"); }
};
template <int V, int... Vs, class... Rest> struct Dispatch<Choices<V, Vs...>, Rest...> {
  template <class F, class... C> static void run(F &f, const int *v, C... c) {
    if (*v == V) Dispatch<Rest...>::run(f, v + 1, c..., std::integral_constant<int, V>{});
    else Dispatch<Choices<Vs...>, Rest...>::run(f, v, c...);
  }
};
template <class... Sets, class F, class... I> static void dispatch(F &&f, I... v) {
  static_assert(sizeof...(Sets) == sizeof...(I), "one run-time value per choice list");
  const int vals[] = {(int)v...};
  Dispatch<Sets...>::run(f, vals);
}
using Variants = Choices<VAR_VA, VAR_PROF, VAR_PLAIN>;

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
inline constexpr const char *FUSED_WHY_NO_INSTANCE = "no fused kernel instance for this arithmetic and two-body mode (the f16x2 instances take the tabulated two-body embedding)";

// Why family f has no instance for the model's depths, width classes and this arithmetic; nullptr when it has one.  Accept or refuse is the table's word; the text names the
// first field that no row of the family holds together with the ones before it, in the gates' order of precedence.
inline const char *fused_class_refusal(FusedFamily f, const HostModel &h, Arith arith, bool tb_table, bool lx64_w128) {
  const bool wide = fused_is_wide(f);
  const FusedInstanceKey k{f, arith, tb_table, h.mlp_depth, h.readout_depth, fused_WF(h), fused_RF(h), lx64_w128};
  auto holds = [&](unsigned fields) { return fused_find_instance(k, fields) != nullptr; };
  if (!holds(FQ_MD) || !holds(FQ_RD)) return FUSED_WHY_DEPTHS;
  if (k.RF == FUSED_RF2) {
    if (!holds(FQ_RF | FQ_WF)) return FUSED_WHY_R64_W128;
    if (!holds(FQ_RF | FQ_WF | FQ_AR)) return wide ? FUSED_WHY_R64_ARITH_WIDE : FUSED_WHY_R64_ARITH_NARROW;
    if (!holds(FQ_RF | FQ_WF | FQ_AR | FQ_RD)) return FUSED_WHY_R64_RD;
  }
  if (k.WF == FUSED_WF2) {
    if (!holds(FQ_WF)) return FUSED_WHY_W128_LX64;
    if (fused_find_instance(k, FQ_WF)->lx64_w128 && h.allow_tf32) return FUSED_WHY_W128_LX64_TF32;      // (behind the option: f16x2 with no float32 twin)
    if (!holds(FQ_WF | FQ_AR)) return wide ? FUSED_WHY_W128_ARITH_WIDE : FUSED_WHY_W128_ARITH_NARROW;
    if (!holds(FQ_WF | FQ_AR | FQ_RD)) return FUSED_WHY_W128_RD;
  }
  if (!holds(FQ_WF | FQ_RF | FQ_AR)) return FUSED_WHY_NO_INSTANCE;
  if (!holds(FQ_WF | FQ_RF | FQ_AR | FQ_MD))
    return wide ? "MLP depth 1 / 3 runs on the f16x2 arithmetic only on the wide fused kernels (fused_arith=auto|f16x2)"
                : "MLP depth 1 / 3 runs on the f16x2 arithmetic with the tabulated two-body embedding only (fused_arith=auto|f16x2, fused_tb=table, allow_tf32 = 0)";
  if (!holds(FQ_WF | FQ_RF | FQ_AR | FQ_RD))
    return wide ? "read-out depth 2 runs on the f16x2 arithmetic only on the wide fused kernels (fused_arith=auto|f16x2)"
                : "read-out depth 2 runs on the f16x2 arithmetic with the tabulated two-body embedding only (fused_arith=auto|f16x2, fused_tb=table, allow_tf32 = 0)";
  return holds(FQ_ALL) ? nullptr : FUSED_WHY_NO_INSTANCE;
}

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
  if (const char *msg = fused_class_refusal(FusedFamily::k_fused, h, arith, tb_table, false)) return no(msg);
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
  if (const char *msg = fused_class_refusal(fused_shape_class(h), h, arith, true, lx64_w128)) return no(msg);
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
