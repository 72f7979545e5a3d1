// Which arithmetic the fused kernels' linears run, decided in one place: option fused_arith (and the environment overrides of the A/B tools), the model
// file's allow_tf32, the sticky fall-back of fused_arith=auto, the two-body mode of k_fused.  Host-only and free of HIP: the C-ABI (allegro_hip.hip), the
// prepare steps of the kernel files and a stand-alone CPU test (tests/host_emu/arith_policy_main.cpp) read the same rules.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

namespace ahip {

// Arithmetic of a fused kernel's linears.  The values are the kernels' `int AR` template arguments and the entries of their dispatch<Choices<...>> lists:
//   AR_F32     f32-input MFMA, exact fmaf chains
//   AR_BF16X3  three-term bf16 split, float32-equivalent (k_fused only)
//   AR_TF32EQ  two-term bf16 split, what a model file licenses with allow_tf32 = 1 (k_fused only)
//   AR_F16X2   two float16 terms per operand, float32-equivalent (fused_h.h)
enum Arith : int { AR_F32 = 0, AR_BF16X3 = 1, AR_TF32EQ = 2, AR_F16X2 = 3 };

// "fused_f32" | "fused_bf16x3" | "fused_tf32eq" | "fused_f16x2": what ahip_last_path reports after a fused evaluation
inline const char *fused_path_name(Arith a) {
  return a == AR_TF32EQ ? "fused_tf32eq" : a == AR_F16X2 ? "fused_f16x2" : a == AR_BF16X3 ? "fused_bf16x3" : "fused_f32";
}

// An enumerated option keeps its words as one '|'-separated list beside its enum, in the order of the enumerators (the list is also the tail of the
// option's error text).  Position of `word` in such a list, -1 when it is not one of them:
inline int word_index(const char *list, const std::string &word) {
  int i = 0;
  for (const char *p = list; *p; ++i) {
    const char *e = std::strchr(p, '|');
    const size_t n = e ? (size_t)(e - p) : std::strlen(p);
    if (word.size() == n && word.compare(0, n, p, n) == 0) return i;
    p += n + (e ? 1 : 0);
  }
  return -1;
}
// the i-th word of such a list
inline std::string word_at(const char *list, int i) {
  const char *p = list;
  for (; i > 0 && p; --i) { p = std::strchr(p, '|'); if (p) ++p; }
  if (!p) return "";
  const char *e = std::strchr(p, '|');
  return e ? std::string(p, e) : std::string(p);
}

// option fused_arith
enum class ArithOpt { Auto, F32, F16x2, Bf16x3, Tf32eq };
inline constexpr const char *ARITH_OPT_WORDS = "auto|f32|f16x2|bf16x3|tf32eq";
inline std::string arith_opt_name(ArithOpt o) { return word_at(ARITH_OPT_WORDS, (int)o); }
inline bool parse_arith_opt(const std::string &word, ArithOpt &o) {
  const int i = word_index(ARITH_OPT_WORDS, word);
  if (i >= 0) o = (ArithOpt)i;
  return i >= 0;
}
// a word of the environment override AHIP_FUSED_ARITH: the option's words and "b3" (= bf16x3); anything else runs as f32
inline ArithOpt arith_opt_of_override(const std::string &word) {
  ArithOpt o = ArithOpt::F32;
  if (word == "b3") return ArithOpt::Bf16x3;
  (void)parse_arith_opt(word, o);
  return o;
}
// option fused_arith as it applies (the environment variable of the A/B tools wins)
inline ArithOpt arith_effective(ArithOpt opt) {
  const char *ar = std::getenv("AHIP_FUSED_ARITH");
  return ar ? arith_opt_of_override(ar) : opt;
}

// option fused_tb: two-body embedding of k_fused from the spline table or evaluated in the kernel as an MLP; AHIP_FUSED_TB overrides it
enum class FusedTb { Table, Mlp };
inline constexpr const char *FUSED_TB_WORDS = "table|mlp";
inline bool fused_tb_is_table(FusedTb opt) {
  const char *tb = std::getenv("AHIP_FUSED_TB");
  return tb ? std::strcmp(tb, "mlp") != 0 : opt != FusedTb::Mlp;
}

// fused_arith=auto must never be less robust than the reference's float32: a model the f16x2 split cannot carry -- a weight beyond float16's range, a linear
// whose weights sit in float16's subnormals, an activation that overflows, a first evaluation that disagrees with the f32 instance -- runs on the f32-input
// MFMA instance for the rest of this model's life instead of failing.  Only an EXPLICIT fused_arith=f16x2 still reports those as errors.
struct ArithState {
  ArithOpt opt = ArithOpt::Auto;            // auto = f16x2; tf32eq iff the model file sets allow_tf32 (k_fused); f32 once auto has degraded
  bool degraded = false;                    // auto has fallen back to f32 (sticky)
  bool checked = false;                     // the first-evaluation self-check of auto's f16x2 against the f32 instance has run (allegro_hip.hip: run_model)
  bool force_f32 = false;                   // self-check only: auto resolves to f32 for this dispatch
  int check_attempts = 0;
  std::string note;                         // what auto decided and why, one line (ahip_arith_note)
  Arith last = AR_F32;                      // what the last fused evaluation used
};
// the effective option is auto and has not degraded yet: a float16 range finding switches the model to f32 instead of being an error
inline bool arith_may_degrade(const ArithState &a) { return arith_effective(a.opt) == ArithOpt::Auto && !a.degraded; }

// The arithmetic an EFFECTIVE option resolves to.  k_fused (wide = false) has every instance: auto is tf32eq iff the model file licenses it, else f16x2
// unless the model has degraded or the self-check is running its f32 pass; the f16x2 instances exist with the tabulated two-body embedding only.  The wide
// kernels (l_max = 2) have f16x2 and f32: the bf16 splits run as f32 there, allow_tf32 and fused_tb play no part.
inline Arith resolve_arith(ArithOpt opt, bool allow_tf32, bool degraded, bool force_f32, bool tb_table, bool wide) {
  const bool free_auto = opt == ArithOpt::Auto && !force_f32;
  const bool f16x2 = opt == ArithOpt::F16x2 || (free_auto && !degraded);
  if (wide) return f16x2 ? AR_F16X2 : AR_F32;
  if (opt == ArithOpt::Bf16x3) return AR_BF16X3;
  if (opt == ArithOpt::Tf32eq || (free_auto && allow_tf32)) return AR_TF32EQ;
  return f16x2 && tb_table ? AR_F16X2 : AR_F32;
}

}  // namespace ahip
