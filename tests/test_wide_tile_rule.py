"""The rule behind option wide_tile=auto on the CPU (csrc/fused_shapes.h: fused_has_wide_tile, lx_tile_slots, lx_tile_maxa): which (family, arithmetic, latent MLP
depth, read-out depth) has the 8-wave / 128-slot tile shape of k_fused_lx.  The header is host-compilable; a stand-alone program built with plain g++ prints the table."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pair_allegro_amd", "csrc")

RULE_MAIN = r"""
#include <cstdio>
#include "fused_shapes.h"
using namespace ahip;
int main() {
  const FusedFamily fams[] = {FusedFamily::none, FusedFamily::k_fused, FusedFamily::lx32, FusedFamily::lx64};
  const Arith ars[] = {AR_F32, AR_BF16X3, AR_TF32EQ, AR_F16X2};
  std::printf("{\"slots\": [%d, %d], \"maxa\": [%d, %d], \"rows\": [\n", lx_tile_slots(false), lx_tile_slots(true), lx_tile_maxa(false), lx_tile_maxa(true));
  bool first = true;
  for (FusedFamily f : fams)
    for (Arith ar : ars)
      for (int md = 0; md <= 4; ++md)
        for (int rd = 0; rd <= 3; ++rd) {
          std::printf("%s{\"family\": \"%s\", \"arith\": \"%s\", \"md\": %d, \"rd\": %d, \"wide\": %d, \"exists\": %d}", first ? "" : ",\n", fused_family_name(f),
                      fused_path_name(ar), md, rd, (int)fused_has_wide_tile(f, ar, md, rd), (int)fused_instance_exists(f, ar, true, md, rd));
          first = false;
        }
  std::printf("\n]}\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_tile_rule")
    src, exe = d / "rule_main.cpp", d / "rule_main"
    src.write_text(RULE_MAIN)
    # plain host compiler, no HIP include path: the header must stand on its own
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), os.path.join(CSRC, "model_io.cpp"), "-o", str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode())


def test_the_128_slot_shape_exists_exactly_for_lx32_f32_and_f16x2_at_depths_2_1(rule):
    rows = rule["rows"]
    assert len(rows) == 4 * 4 * 5 * 4
    for r in rows:
        want = r["family"] == "lx32" and r["arith"] in ("fused_f32", "fused_f16x2") and (r["md"], r["rd"]) == (2, 1)
        assert bool(r["wide"]) == want, r
    assert sum(r["wide"] for r in rows) == 2


def test_the_128_slot_shape_only_where_the_family_has_an_instance_at_all(rule):
    assert all(r["exists"] for r in rule["rows"] if r["wide"])


def test_tile_shapes(rule):
    assert rule["slots"] == [64, 128] and rule["maxa"] == [4, 8]
