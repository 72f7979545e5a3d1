"""The second width of the fused kernels' read-out MLP on the CPU (csrc/fused_shapes.h: FUSED_RF2 = 64, fused_RF; csrc/model_io.cpp: pad_host_model).

All of it is host-compilable, so small stand-alone programs built here with plain g++ exercise it without a GPU:
  * the decision table of fused_shapes.h over the read-out width (24, 32, 33, 64, 65) x MLP width (64, 128), l_max, tensor features, both depths and every arithmetic:
    family, width classes WF and RF, arithmetic, whether a compiled instance exists, and the refusal reasons, against the rule as the header's head comment states it,
    written independently here; for read-out widths <= 32 also every helper with its new trailing argument left out, so that no existing decision has moved;
  * `fused_shaped_model` of a model of read-out width 50 (padded to 64) and 24 (padded to 32): out.w0 and out.w1 hold the model's block and exact zeros around it.
The row maps (fused_rows.h, fused_lx_rows.h) do not know the read-out width: compiled here beside the shape header, their totals are asserted unchanged.

A model with 33 <= readout_width <= 64 had no fused instance before the width class existed (its family was "none"): those rows are the new ground.  (The weight-stream
builders live in HIP translation units and cannot be reached from a host-only program; the GPU tests cover them.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from pair_allegro_amd import model_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pair_allegro_amd", "csrc")
NAMES = ["Ag", "Cu", "O"]

TABLE_MAIN = r"""
#include <cstdio>
#include "fused_lx_rows.h"
#include "fused_rows.h"
#include "fused_shapes.h"
using namespace ahip;
static_assert(FUSED_RF == 32 && FUSED_RF2 == 64, "the two read-out widths");
static_assert(R_TOTAL(3) == 88 && RowsX::R_TOTAL(3, 2) == 118 && RowsP::R_TOTAL(3, 2) == 10 + 3 * (6 + 2 * 3 + 18), "the row maps do not know the read-out width");
int main() {
  const int Rs[] = {24, 32, 33, 64, 65}, Ws[] = {64, 128}, Us[] = {32, 64};
  const ArithOpt opts[] = {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq};
  std::printf("[\n");
  bool first = true;
  for (int R : Rs)
    for (int W : Ws)
      for (int l = 1; l <= 2; ++l)
        for (int U : Us)
          for (int rd = 0; rd <= 3; ++rd)
            for (int md = 0; md <= 4; ++md)
              for (ArithOpt o : opts)
                for (int degraded = 0; degraded <= 1; ++degraded)
                  for (int tb = 0; tb <= 1; ++tb)
                    for (int tf32 = 0; tf32 <= 1; ++tf32) {
                      HostModel h;
                      h.l_max = l; h.U = U; h.S = 64; h.mlp_width = W; h.readout_width = R; h.mlp_depth = md; h.readout_depth = rd;
                      h.num_bessels = 8; h.num_layers = 2; h.num_types = 3; h.allow_tf32 = tf32;
                      const FusedDecision d = fused_decide(h, o, degraded != 0, false, tb != 0);
                      const bool wide = fused_is_wide(fused_shape_class(h));
                      std::string why = d.why;
                      for (char &c : why) if (c == '"' || c == '\\') c = '\'';
                      // "old": the helpers called the way a caller from before the read-out width class calls them (no RF argument)
                      std::printf("%s{\"R\": %d, \"W\": %d, \"l_max\": %d, \"U\": %d, \"rd\": %d, \"md\": %d, \"opt\": \"%s\", \"degraded\": %d, \"tb\": %d, \"tf32\": %d, \"family\": \"%s\", "
                                  "\"WF\": %d, \"RF\": %d, \"arith\": \"%s\", \"exists\": %d, \"exists_old\": %d, \"wide_tile\": %d, \"wide_tile_old\": %d, \"fit\": %d, \"fit_old\": %d, "
                                  "\"exact\": %d, \"exact_old\": %d, \"why\": \"%s\"}",
                                  first ? "" : ",\n", R, W, l, U, rd, md, arith_opt_name(o).c_str(), degraded, tb, tf32, fused_family_name(d.family), d.WF, d.RF, fused_path_name(d.arith),
                                  (int)fused_instance_exists(d.family, d.arith, tb != 0, md, rd, d.WF, d.RF), (int)fused_instance_exists(d.family, d.arith, tb != 0, md, rd, d.WF),
                                  (int)fused_has_wide_tile(d.family, d.arith, md, rd, d.WF, d.RF), (int)fused_has_wide_tile(d.family, d.arith, md, rd, d.WF),
                                  (int)fused_widths_fit(h, wide, FUSED_WF2, fused_RF(h)), (int)fused_widths_fit(h, wide, FUSED_WF2),
                                  (int)fused_shape_exact(h, fused_shape_class(h), fused_WF(h), fused_RF(h)), (int)fused_shape_exact(h, fused_shape_class(h), fused_WF(h)), why.c_str());
                      first = false;
                    }
  std::printf("\n]\n");
  return 0;
}
"""

PAD_MAIN = r"""
#include <cstdio>
#include <string>
#include "fused_shapes.h"
#include "model_io.h"
using namespace ahip;
// usage: pad_main <model.ahip> <out dir>: every tensor of fused_shaped_model(model, its family, its width classes) as raw float64 in <out dir>/<name>.f64, the shapes in <out dir>/index.txt
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  try {
    const HostModel h = load_model_file(argv[1]);
    const FusedFamily fam = fused_shape_class(h);
    const int RF = fused_RF(h);
    if (RF != (h.readout_width > 32 ? 64 : 32)) return 3;
    const HostModel p = fused_shaped_model(h, fam, fused_WF(h), RF);
    if (!fused_shape_exact(p, fam, fused_WF(h), RF)) return 5;
    if (RF == FUSED_RF2 && fused_shape_exact(p, fam, fused_WF(h))) return 5;      // (without the argument: read-out width 32)
    const std::string dir = argv[2];
    FILE *idx = std::fopen((dir + "/index.txt").c_str(), "w");
    if (!idx) return 4;
    std::fprintf(idx, "l_max %d U %d S %d W %d R %d\n", p.l_max, p.U, p.S, p.mlp_width, p.readout_width);
    for (const auto &kv : p.tensors) {
      std::fprintf(idx, "%s", kv.first.c_str());
      for (int s : kv.second.shape) std::fprintf(idx, " %d", s);
      std::fprintf(idx, "\n");
      FILE *f = std::fopen((dir + "/" + kv.first + ".f64").c_str(), "wb");
      if (!f) return 4;
      if (std::fwrite(kv.second.data.data(), sizeof(double), kv.second.data.size(), f) != kv.second.data.size()) return 4;
      std::fclose(f);
    }
    std::fclose(idx);
  } catch (const std::exception &e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  return 0;
}
"""


def _build(d, name, text, sources=()):
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(text)
    # plain host compiler, no HIP include path: headers and model_io.cpp must stand on their own
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src)] + [os.path.join(CSRC, s) for s in sources] + ["-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("rshapes"), "table_main", TABLE_MAIN, ["model_io.cpp"])
    return json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())


@pytest.fixture(scope="module")
def pad_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("rpad"), "pad_main", PAD_MAIN, ["model_io.cpp"])


# ---------------------------------------------------------------------------- the decision table

NEW_REASONS = {
    "w128": "read-out width 33..64 has no fused instance with MLP width 65..128",
    "arith": "read-out width 33..64 runs on the f16x2 arithmetic",
    "arith_tb": "read-out width 33..64 runs on the f16x2 arithmetic with the tabulated two-body embedding only",
    "rd": "read-out width 33..64 runs with read-out depth 1 only",
    "width": "read-out width 64",
}


def _expected(r):
    """(family, WF, RF, arithmetic, the phrase the refusal must contain) by the rule as the head of fused_shapes.h states it, written independently of its code."""
    opt, l, U, md, rd, W, R, tb = r["opt"], r["l_max"], r["U"], r["md"], r["rd"], r["W"], r["R"], r["tb"]
    f16 = opt == "f16x2" or (opt == "auto" and not r["degraded"])
    if opt == "bf16x3":
        narrow = "fused_bf16x3"
    elif opt == "tf32eq" or (opt == "auto" and r["tf32"]):
        narrow = "fused_tf32eq"
    else:
        narrow = "fused_f16x2" if f16 and tb else "fused_f32"
    wide = "fused_f16x2" if f16 else "fused_f32"
    if l == 1 and U <= 32:
        fam, ar = "k_fused", narrow
    elif l == 2 and U <= 32:
        fam, ar = "lx32", wide
    else:
        fam, ar = "lx64", wide
    no = ("none", 0, 0, None)
    if R > 64:
        return no + (NEW_REASONS["width"],)
    if not (1 <= md <= 3 and 1 <= rd <= 2):
        return no + ("MLP depth 1..3 and read-out depth 1..2",)
    if R > 32:
        if W > 64:
            return no + (NEW_REASONS["w128"],)
        if ar != "fused_f16x2":
            return no + (NEW_REASONS["arith_tb"] if fam == "k_fused" else NEW_REASONS["arith"],)
        if rd != 1:
            return no + (NEW_REASONS["rd"],)
        return fam, 64, 64, ar, None
    if W > 64:
        if fam == "lx64":
            return no + ("MLP width 65..128 has no instance of the wide fused kernel for 33..64 tensor features",)
        if ar != "fused_f16x2":
            return no + ("MLP width 65..128 runs on the f16x2 arithmetic",)
        if rd != 1:
            return no + ("MLP width 65..128 runs with read-out depth 1 only",)
        return fam, 128, 32, ar, None
    if (md != 2 or rd != 1) and ar != "fused_f16x2":
        return no + ("runs on the f16x2 arithmetic",)
    return fam, 64, 32, ar, None


def test_decision_table_over_the_readout_width(table):
    assert len(table) == 5 * 2 * 2 * 2 * 4 * 5 * 5 * 2 * 2 * 2
    seen = set()
    for r in table:
        fam, WF, RF, ar, phrase = _expected(r)
        assert r["family"] == fam, r
        if fam != "none":
            assert (r["WF"], r["RF"], r["arith"], r["exists"], r["why"]) == (WF, RF, ar, 1, ""), r
            assert r["fit"] == 1, r
            if RF == 64:
                # the 128-slot tile of k_fused_lx has no instance of the new width; an instance of the other width class is not this model's
                assert r["wide_tile"] == 0 and r["exists_old"] == 1 and r["fit_old"] == 0 and r["exact_old"] == 0, r
                assert r["exact"] == (1 if (r["R"], r["U"], r["l_max"]) in ((64, 32, 1), (64, 32, 2), (64, 64, 2)) else 0), r
        else:
            assert r["why"] and r["exists"] == 0 and phrase in r["why"], (r, phrase)
            for key, text in NEW_REASONS.items():
                if phrase == text:
                    seen.add(key)
        if r["R"] <= 32:
            # no existing decision moved: the helpers answer what they answer without the new trailing argument, and the class is the old width
            assert r["RF"] == (32 if fam != "none" else 0), r
            assert (r["exists"], r["wide_tile"], r["fit"], r["exact"]) == (r["exists_old"], r["wide_tile_old"], r["fit_old"], r["exact_old"]), r
            for text in NEW_REASONS.values():
                assert text == NEW_REASONS["width"] or text not in r["why"], r
    assert seen == set(NEW_REASONS), seen            # every new refusal text was matched by some row

    def rows(**kw):
        out = [r for r in table if all(r[k] == v for k, v in kw.items())]
        assert out
        return out

    base = dict(W=64, rd=1, opt="auto", degraded=0, tb=1, tf32=0)
    for R in (33, 64):
        for md in (1, 2, 3):
            assert {(r["family"], r["WF"], r["RF"], r["arith"]) for r in rows(R=R, l_max=1, U=32, md=md, **base)} == {("k_fused", 64, 64, "fused_f16x2")}
            assert {(r["family"], r["WF"], r["RF"], r["arith"]) for r in rows(R=R, l_max=2, U=32, md=md, **base)} == {("lx32", 64, 64, "fused_f16x2")}
            for l in (1, 2):
                assert {(r["family"], r["WF"], r["RF"], r["arith"]) for r in rows(R=R, l_max=l, U=64, md=md, **base)} == {("lx64", 64, 64, "fused_f16x2")}
        # l_max = 2 rows: the narrow gate's half of the reason is "need l_max = 1", so the phrase below comes from the wide gate alone
        for U in (32, 64):
            for r in rows(R=R, l_max=2, U=U, md=2, **dict(base, rd=2)):
                assert r["family"] == "none" and NEW_REASONS["rd"] in r["why"], r
            for r in rows(R=R, l_max=2, U=U, md=2, **dict(base, W=128)):
                assert r["family"] == "none" and NEW_REASONS["w128"] in r["why"], r
            for kw in (dict(opt="f32"), dict(opt="bf16x3"), dict(opt="tf32eq"), dict(degraded=1)):
                for r in rows(R=R, l_max=2, U=U, md=2, **dict(base, **kw)):
                    assert r["family"] == "none" and NEW_REASONS["arith"] in r["why"], r
            # the wide kernels take no part in fused_tb / allow_tf32
            for kw in (dict(tb=0), dict(tf32=1)):
                assert {(r["family"] != "none", r["RF"]) for r in rows(R=R, l_max=2, U=U, md=2, **dict(base, **kw))} == {(True, 64)}
        for kw in (dict(tb=0), dict(tf32=1), dict(opt="f32"), dict(degraded=1)):
            for r in rows(R=R, l_max=1, U=32, md=2, **dict(base, **kw)):
                assert r["family"] == "none" and NEW_REASONS["arith_tb"] in r["why"], r
        for r in rows(R=R, l_max=1, U=32, md=2, **dict(base, rd=2)):
            assert r["family"] == "none" and NEW_REASONS["rd"] in r["why"], r
        for r in rows(R=R, l_max=1, U=32, md=2, **dict(base, W=128)):
            assert r["family"] == "none" and NEW_REASONS["w128"] in r["why"], r
    for r in rows(R=65):
        assert r["family"] == "none" and r["fit"] == 0 and "read-out width 64" in r["why"] and "MLP width 128" in r["why"], r
    # the 128-slot tile of k_fused_lx where it was, and nowhere in the new class
    assert {r["wide_tile"] for r in rows(R=32, l_max=2, U=32, md=2, **base)} == {1}
    assert {r["wide_tile"] for r in rows(R=24, l_max=2, U=32, md=2, **base)} == {1}
    assert {r["wide_tile"] for r in rows(R=33, l_max=2, U=32, md=2, **base)} == {0}
    assert {r["wide_tile"] for r in rows(R=64, l_max=2, U=32, md=2, **base)} == {0}


# ---------------------------------------------------------------------------- zero padding to read-out width 64

def _read_dump(d):
    lines = open(os.path.join(d, "index.txt")).read().splitlines()
    head = lines[0].split()
    meta = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    tensors = {}
    for ln in lines[1:]:
        name, *shape = ln.split()
        tensors[name] = np.fromfile(os.path.join(d, name + ".f64"), dtype=np.float64).reshape([int(s) for s in shape])
    return meta, tensors


@pytest.mark.parametrize("R,RF", [(50, 64), (33, 64), (64, 64), (24, 32), (32, 32)])
@pytest.mark.parametrize("l_max,U,UF", [(1, 16, 32), (2, 16, 32), (2, 40, 64)])
def test_shaped_model_pads_the_readout_to_its_width_class(pad_exe, tmp_path, R, RF, l_max, U, UF):
    """S 48, MLP width 40, read-out width R, 3 types, 2 layers on every family: fused_shaped_model pads out.w0 to [64][RF] and out.w1 to [RF][1], the model's block in
    place and exact zeros around it."""
    cfg = dict(model_file.DEFAULT_CFG, model_dtype="float64", type_names=NAMES, l_max=l_max, num_layers=2, num_scalar_features=48, num_tensor_features=U,
               mlp_width=40, mlp_depth=2, readout_depth=1, readout_width=R, avg_num_neighbors=30.0)
    w = model_file.init_weights(cfg)
    path = str(tmp_path / "m.ahip")
    model_file.save_ahip(path, cfg, w)
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([pad_exe, path, str(out)], check=True)
    meta, got = _read_dump(str(out))
    assert meta == {"l_max": l_max, "U": UF, "S": 64, "W": 64, "R": RF}
    w0, w1 = got["out.w0"], got["out.w1"]
    assert w0.shape == (64, RF) and w1.shape == (RF, 1)
    a0, a1 = np.asarray(w["out.w0"], dtype=np.float64), np.asarray(w["out.w1"], dtype=np.float64).reshape(R, 1)
    assert np.array_equal(w0[:48, :R], a0) and not w0[48:].any() and not w0[:, R:].any() and a0.any()
    assert np.array_equal(w1[:R], a1) and not w1[R:].any() and a1.any()
    assert set(got) == set(w)
