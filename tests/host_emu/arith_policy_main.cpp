// TEST INFRASTRUCTURE ONLY (tests/test_arith_policy.py): prints what arith_policy.h resolves for every combination of its inputs, one line each:
//   <effective option word> <allow_tf32> <degraded> <force_f32> <table|mlp> <k_fused|wide> <Arith value> <path name>
// then, per enumerator of option fused_arith, "name <enumerator value> <arith_opt_name of it>".
#include <cstdio>

#include "arith_policy.h"

int main() {
  using namespace ahip;
  const char *words[] = {"auto", "f32", "f16x2", "bf16x3", "tf32eq", "b3", "fp8"};
  for (const char *word : words)
    for (int allow = 0; allow < 2; ++allow)
      for (int degraded = 0; degraded < 2; ++degraded)
        for (int force = 0; force < 2; ++force)
          for (int table = 1; table >= 0; --table)
            for (int wide = 0; wide < 2; ++wide) {
              const Arith a = resolve_arith(arith_opt_of_override(word), allow != 0, degraded != 0, force != 0, table != 0, wide != 0);
              std::printf("%s %d %d %d %s %s %d %s\n", word, allow, degraded, force, table ? "table" : "mlp", wide ? "wide" : "k_fused", (int)a, fused_path_name(a));
            }
  for (ArithOpt o : {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq}) std::printf("name %d %s\n", (int)o, arith_opt_name(o).c_str());
  return 0;
}
