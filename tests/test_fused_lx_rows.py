"""Saved-row maps of the wide fused kernels (csrc/fused_lx_rows.h) on the CPU: the header is host-compilable, so a small stand-alone program built here
with plain g++ prints the maps of both shapes (k_fused_lx: RowsX, k_fused_lx2: RowsP) for every layer count and latent-MLP depth the kernels are built for.

A wave's scratch is R_TOTAL rows; the kernels address it only through these functions, so rows that overlap (two saves clobbering each other) or fall
outside [0, R_TOTAL) (a store past the wave's scratch -- the buffer descriptor drops it, the backward pass then reads zeros) show here without a GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pair_allegro_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "fused_lx_rows.h"
using namespace ahip;
// the maps must be usable in constant expressions (the kernels take them as compile-time row offsets)
static_assert(RowsX::R_TOTAL(3, 2) > 0 && RowsP::R_LAYER(2, 3) > 0, "constexpr");
template <class R> static void dump(const char *name, bool last) {
  std::printf("\"%s\": {\"EW\": %d, \"HR\": %d, \"NV\": %d, \"maps\": [", name, R::EW, R::HR, R::NV);
  bool first = true;
  for (int NL = 1; NL <= 3; ++NL)
    for (int MD = 1; MD <= 3; ++MD) {
      std::printf("%s{\"NL\": %d, \"MD\": %d, \"R_DX0\": %d, \"R_W0\": %d, \"O_OM\": %d, \"O_U\": %d, \"O_VIN\": %d, \"LSZ\": %d, \"R_TOTAL\": %d, \"O_Z\": [",
                  first ? "" : ", ", NL, MD, R::R_DX0, R::R_W0, R::O_OM, R::O_U(MD), R::O_VIN(MD), R::LSZ(MD), R::R_TOTAL(NL, MD));
      for (int h = 1; h <= MD; ++h) std::printf("%s%d", h > 1 ? ", " : "", R::O_Z(h));
      std::printf("], \"R_LAYER\": [");
      for (int k = 0; k < NL; ++k) std::printf("%s%d", k ? ", " : "", R::R_LAYER(k, MD));
      std::printf("]}");
      first = false;
    }
  std::printf("]}%s\n", last ? "" : ",");
}
int main() {
  std::printf("{\n");
  dump<RowsX>("k_fused_lx", false);
  dump<RowsP>("k_fused_lx2", true);
  std::printf("}\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    d = tmp_path_factory.mktemp("lx_rows")
    src, exe = d / "rows_main.cpp", d / "rows_main"
    src.write_text(MAIN)
    # plain host compiler, no HIP include path: the header must stand on its own
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode())


def _ranges(shape, m):
    """Every named row range [lo, hi) of one wave's scratch: d x0/dd (4 rows), w0, and per layer omega, the hidden layers, u, V_in."""
    ew, hr, nv = shape["EW"], shape["HR"], shape["NV"]
    out = [("dx0", m["R_DX0"], m["R_DX0"] + 4), ("w0", m["R_W0"], m["R_W0"] + ew)]
    for k, rl in enumerate(m["R_LAYER"]):
        out.append((f"l{k}.omega", rl + m["O_OM"], rl + m["O_OM"] + ew))
        for h, oz in enumerate(m["O_Z"], start=1):
            out.append((f"l{k}.hidden{h}", rl + oz, rl + oz + hr))
        out.append((f"l{k}.u", rl + m["O_U"], rl + m["O_U"] + hr))
        out.append((f"l{k}.V_in", rl + m["O_VIN"], rl + m["O_VIN"] + nv))
    return out


@pytest.mark.parametrize("kernel", ["k_fused_lx", "k_fused_lx2"])
def test_row_ranges_are_disjoint_and_tile_the_scratch(maps, kernel):
    shape = maps[kernel]
    seen = set()
    for m in shape["maps"]:
        seen.add((m["NL"], m["MD"]))
        assert len(m["O_Z"]) == m["MD"] and len(m["R_LAYER"]) == m["NL"]
        owner = {}
        for name, lo, hi in _ranges(shape, m):
            assert 0 <= lo < hi <= m["R_TOTAL"], (kernel, m["NL"], m["MD"], name, lo, hi)
            for r in range(lo, hi):
                assert r not in owner, f"{kernel} NL={m['NL']} MD={m['MD']}: row {r} belongs to {owner[r]} and {name}"
                owner[r] = name
        assert sorted(owner) == list(range(m["R_TOTAL"])), f"{kernel} NL={m['NL']} MD={m['MD']}: rows without an owner"
        # consecutive layers are LSZ apart, and a deeper MLP only adds HR rows per hidden layer
        for a, b in zip(m["R_LAYER"], m["R_LAYER"][1:]):
            assert b - a == m["LSZ"]
        assert m["LSZ"] == shape["EW"] + shape["HR"] * (m["MD"] + 1) + shape["NV"]
    assert seen == {(nl, md) for nl in (1, 2, 3) for md in (1, 2, 3)}


@pytest.mark.parametrize("kernel,hr,lsz,total3", [("k_fused_lx", 4, 36, 118), ("k_fused_lx2", 2, 30, 100)])
def test_depth_2_maps_are_the_ones_the_kernels_had(maps, kernel, hr, lsz, total3):
    """MD = 2 reproduces the row indices of the kernels before the depth parameter existed: d x0/dd 0..3, w0 from 4, per layer omega | silu'(z1) | z2 | u | V_in."""
    shape = maps[kernel]
    ew = shape["EW"]
    assert (ew, shape["HR"], shape["NV"]) == (6, hr, 18)
    for m in shape["maps"]:
        if m["MD"] != 2:
            continue
        assert (m["R_DX0"], m["R_W0"], m["O_OM"]) == (0, 4, 0)
        assert m["O_Z"] == [ew, ew + hr] and m["O_U"] == ew + 2 * hr and m["O_VIN"] == ew + 3 * hr
        assert m["LSZ"] == lsz
        assert m["R_LAYER"] == [4 + ew + k * lsz for k in range(m["NL"])]
        assert m["R_TOTAL"] == 4 + ew + m["NL"] * lsz
        if m["NL"] == 3:
            assert m["R_TOTAL"] == total3
