"""Option lx64_mlp_width=auto on the CPU: the trailing `lx64_w128` argument of the gates in csrc/fused_shapes.h (the MLP-width-128 instances of k_fused_lx2, the wide
kernel for 33..64 tensor features), the saved-row map RowsPM of csrc/fused_lx_rows.h, and the padded model those instances run on.

Host-compiled with plain g++ like tests/test_fused_mlp_width_shapes.py:
  * over a grid of shapes, depths, arithmetic options: the gates with `false` answer exactly what they answer without the argument (the default of the option is today's
    behaviour), and with `true` the decision differs only for 33..64 tensor features at MLP width 65..128;
  * with `true` those models get ("lx64", l_run 2, UF 64, WF 128, RF 32, f16x2); read-out depth 2, read-out width 64, fused_arith=f32, allow_tf32 = 1, MLP width 129 and more
    than 16 active types stay refused, each with its reason;
  * RowsPM against RowsP and the closed forms; the padded model of an (S 48, U 48, W 100, R 24) model."""
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
#include "fused_shapes.h"
using namespace ahip;
static bool same(const FusedDecision &a, const FusedDecision &b) {
  return a.family == b.family && a.l_run == b.l_run && a.UF == b.UF && a.WF == b.WF && a.RF == b.RF && a.arith == b.arith && a.why == b.why;
}
static void put(const char *key, const FusedDecision &d, int md, int rd, bool on) {
  std::string why = d.why;
  for (char &c : why) if (c == '"' || c == '\\') c = '\'';
  std::printf("\"%s\": {\"family\": \"%s\", \"l_run\": %d, \"UF\": %d, \"WF\": %d, \"RF\": %d, \"arith\": \"%s\", \"exists\": %d, \"why\": \"%s\"}", key, fused_family_name(d.family), d.l_run, d.UF,
              d.WF, d.RF, fused_path_name(d.arith), (int)fused_instance_exists(d.family, d.arith, true, md, rd, d.WF, d.RF, on), why.c_str());
}
int main() {
  const int Us[] = {16, 32, 33, 48, 64}, Ws[] = {40, 64, 65, 100, 128, 129}, Rs[] = {24, 32, 64};
  const ArithOpt opts[] = {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq};
  std::printf("[\n");
  bool first = true;
  for (int l = 1; l <= 2; ++l)
    for (int U : Us)
      for (int W : Ws)
        for (int R : Rs)
          for (int md = 1; md <= 3; ++md)
            for (int rd = 1; rd <= 2; ++rd)
              for (ArithOpt o : opts)
                for (int tf32 = 0; tf32 <= 1; ++tf32)
                  for (int degraded = 0; degraded <= 1; ++degraded) {
                    HostModel h;
                    h.l_max = l; h.U = U; h.S = 64; h.mlp_width = W; h.readout_width = R; h.mlp_depth = md; h.readout_depth = rd;
                    h.num_bessels = 8; h.num_layers = 2; h.num_types = 3; h.allow_tf32 = tf32;
                    const FusedDecision a = fused_decide(h, o, degraded != 0, false, true), b = fused_decide(h, o, degraded != 0, false, true, -1, false),
                                        c = fused_decide(h, o, degraded != 0, false, true, -1, true);
                    // the overload on resolved arithmetics, and the wide gate itself
                    const Arith an = resolve_arith(o, tf32 != 0, degraded != 0, false, true, false), aw = resolve_arith(o, tf32 != 0, degraded != 0, false, true, true);
                    const FusedDecision a2 = fused_decide(h, an, aw, true), b2 = fused_decide(h, an, aw, true, -1, false), c2 = fused_decide(h, an, aw, true, -1, true);
                    std::string w1, w2;
                    const bool g1 = fused_wide_supported(h, aw, &w1), g2 = fused_wide_supported(h, aw, &w2, -1, false);
                    const bool same_false = same(a, b) && same(a2, b2) && same(a, a2) && same(c, c2) && g1 == g2 && w1 == w2 &&
                                            fused_instance_exists(a.family, a.arith, true, md, rd, a.WF, a.RF) == fused_instance_exists(a.family, a.arith, true, md, rd, a.WF, a.RF, false);
                    std::printf("%s{\"l_max\": %d, \"U\": %d, \"W\": %d, \"R\": %d, \"md\": %d, \"rd\": %d, \"opt\": \"%s\", \"tf32\": %d, \"degraded\": %d, \"same_false\": %d, \"same_true\": %d, ",
                                first ? "" : ",\n", l, U, W, R, md, rd, arith_opt_name(o).c_str(), tf32, degraded, (int)same_false, (int)same(a, c));
                    put("off", a, md, rd, false);
                    std::printf(", ");
                    put("on", c, md, rd, true);
                    std::printf("}");
                    first = false;
                  }
  // more than 16 active types, with the option
  {
    HostModel h;
    h.l_max = 2; h.U = 64; h.S = 64; h.mlp_width = 128; h.readout_width = 32; h.mlp_depth = 2; h.readout_depth = 1;
    h.num_bessels = 8; h.num_layers = 2; h.num_types = 20; h.allow_tf32 = 0;
    const FusedDecision many = fused_decide(h, ArithOpt::Auto, false, false, true, 17, true), few = fused_decide(h, ArithOpt::Auto, false, false, true, 3, true);
    std::printf(",\n{\"types\": 1, ");
    put("many", many, 2, 1, true);
    std::printf(", ");
    put("few", few, 2, 1, true);
    std::printf("}");
  }
  std::printf("\n]\n");
  return 0;
}
"""

ROWS_MAIN = r"""
#include <cstdio>
#include "fused_lx_rows.h"
using namespace ahip;
static_assert(RowsPM::R_TOTAL(3, 3) == 124 && RowsPM::R_TOTAL(3, 2) == 112 && RowsP::R_TOTAL(3, 3) == 106, "constexpr");
template <class R> static void dump(const char *name, bool last) {
  std::printf("\"%s\": {\"EW\": %d, \"HR\": %d, \"UR\": %d, \"NV\": %d, \"maps\": [", name, R::EW, R::HR, R::UR, R::NV);
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
  dump<RowsP>("RowsP", false);
  dump<LxRows<6, 2, 18>>("LxRows_6_2_18", false);
  dump<RowsPM>("RowsPM", true);
  std::printf("}\n");
  return 0;
}
"""

PAD_MAIN = r"""
#include <cstdio>
#include <string>
#include "fused_shapes.h"
#include "model_io.h"
using namespace ahip;
// usage: pad_main <model.ahip> <out dir>: every tensor of fused_shaped_model(model, lx64, 128, 32) as raw float64 in <out dir>/<name>.f64, the shapes in <out dir>/index.txt
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  try {
    const HostModel h = load_model_file(argv[1]);
    if (fused_shape_class(h) != FusedFamily::lx64 || fused_WF(h) != FUSED_WF2 || fused_RF(h) != FUSED_RF) return 3;
    const HostModel p = fused_shaped_model(h, FusedFamily::lx64, 128, 32);
    if (!fused_shape_exact(p, FusedFamily::lx64, FUSED_WF2, FUSED_RF) || fused_shape_exact(p, FusedFamily::lx64)) return 5;
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
    exe = _build(tmp_path_factory.mktemp("lx64w"), "table_main", TABLE_MAIN, ["model_io.cpp"])
    return json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("lx64rows"), "rows_main", ROWS_MAIN)
    return json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())


@pytest.fixture(scope="module")
def pad_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("lx64pad"), "pad_main", PAD_MAIN, ["model_io.cpp"])


def _grid(table):
    return [r for r in table if "types" not in r]


def _rows(table, **kw):
    out = [r for r in _grid(table) if all(r[k] == v for k, v in kw.items())]
    assert out, kw
    return out


# ---------------------------------------------------------------------------- the gates

def test_false_is_the_answer_without_the_argument_and_true_differs_only_in_the_hole(table):
    grid = _grid(table)
    assert len(grid) == 2 * 5 * 6 * 3 * 3 * 2 * 5 * 2 * 2
    differ = 0
    for r in grid:
        assert r["same_false"] == 1, r
        in_hole = 33 <= r["U"] <= 64 and 65 <= r["W"] <= 128
        if not in_hole:
            assert r["same_true"] == 1 and r["on"] == r["off"], r
        else:
            # without the option: refused, by the reason the existing tests pin -- or, for read-out width 64, by the reason that comes before it
            assert r["off"]["family"] == "none", r
            assert "33..64 tensor features" in r["off"]["why"] or (r["R"] == 64 and "read-out width 33..64 has no fused instance with MLP width 65..128" in r["off"]["why"]), r
            differ += r["same_true"] == 0
    assert differ > 0
    # the models the option is for change family; everything else in the hole changes its reason at most
    for r in grid:
        if r["same_true"] == 0 and r["on"]["family"] != "none":
            assert r["on"]["family"] == "lx64" and r["on"]["WF"] == 128, r


def test_with_the_option_the_hole_runs_on_lx64_at_width_128(table):
    for l in (1, 2):
        for U in (33, 48, 64):
            for W in (65, 100, 128):
                for md in (1, 2, 3):
                    for R in (24, 32):
                        for r in _rows(table, l_max=l, U=U, W=W, R=R, md=md, rd=1, opt="auto", tf32=0, degraded=0):
                            on = r["on"]
                            assert (on["family"], on["l_run"], on["UF"], on["WF"], on["RF"], on["arith"], on["exists"], on["why"]) == ("lx64", 2, 64, 128, 32, "fused_f16x2", 1, ""), r
                            assert r["off"]["exists"] == 0
                        for r in _rows(table, l_max=l, U=U, W=W, R=R, md=md, rd=1, opt="f16x2", tf32=0, degraded=0):
                            assert (r["on"]["family"], r["on"]["WF"], r["on"]["arith"]) == ("lx64", 128, "fused_f16x2"), r
    # MLP width <= 64 and the other two families: the option changes nothing (covered row by row above; here the families by name)
    for r in _rows(table, W=128, U=32, l_max=2, R=32, md=2, rd=1, opt="auto", tf32=0, degraded=0):
        assert r["on"] == r["off"] and r["on"]["family"] == "lx32"
    for r in _rows(table, W=64, U=64, l_max=2, R=32, md=2, rd=1, opt="auto", tf32=0, degraded=0):
        assert r["on"] == r["off"] and (r["on"]["family"], r["on"]["WF"]) == ("lx64", 64)


def test_refusals_with_the_option(table):
    base = dict(l_max=2, U=64, W=128, R=32, md=2, rd=1, opt="auto", tf32=0, degraded=0)

    def refused(phrase, **kw):
        for l in (1, 2):
            for U in (33, 48, 64):
                for r in _rows(table, **dict(base, l_max=l, U=U, **kw)):
                    assert r["on"]["family"] == "none" and r["on"]["exists"] == 0 and phrase in r["on"]["why"], (r, phrase)

    refused("MLP width 65..128 runs with read-out depth 1 only", rd=2)
    refused("read-out width 33..64 has no fused instance with MLP width 65..128", R=64)
    refused("MLP width 65..128 runs on the f16x2 arithmetic only on the wide fused kernels", opt="f32")
    refused("MLP width 65..128 runs on the f16x2 arithmetic only on the wide fused kernels", degraded=1)
    refused("MLP width 65..128 runs on the f16x2 arithmetic only on the wide fused kernels", opt="bf16x3")
    # allow_tf32 = 1: fused_arith=auto resolves to f16x2 on the wide kernels whatever the model licenses, and its self-check does not run for a licensed model; the
    # f16x2-only instances behind the option stay closed to it, under auto and under an explicit f16x2
    refused("(option lx64_mlp_width=auto) runs on the f16x2 arithmetic for models with allow_tf32 = 0 only", tf32=1)
    refused("(option lx64_mlp_width=auto) runs on the f16x2 arithmetic for models with allow_tf32 = 0 only", tf32=1, opt="f16x2")
    refused("MLP width 128", W=129)
    (t,) = [r for r in table if "types" in r]
    assert t["many"]["family"] == "none" and "at most 16 active model types (17 of the model's 20 are mapped)" in t["many"]["why"], t
    assert (t["few"]["family"], t["few"]["WF"], t["few"]["arith"]) == ("lx64", 128, "fused_f16x2"), t


# ---------------------------------------------------------------------------- the row map

def test_rows_pm(maps):
    assert maps["LxRows_6_2_18"] == maps["RowsP"]
    p, pm = maps["RowsP"], maps["RowsPM"]
    assert (p["EW"], p["HR"], p["UR"], p["NV"]) == (6, 2, 2, 18) and (pm["EW"], pm["HR"], pm["UR"], pm["NV"]) == (6, 4, 2, 18)
    for a, b in zip(p["maps"], pm["maps"]):
        nl, md = b["NL"], b["MD"]
        assert (a["NL"], a["MD"]) == (nl, md)
        assert b["O_Z"] == [6 + 4 * (h - 1) for h in range(1, md + 1)] and b["O_U"] == 6 + 4 * md and b["O_VIN"] == 8 + 4 * md
        assert b["R_TOTAL"] == 10 + nl * (26 + 4 * md) and b["LSZ"] == a["LSZ"] + 2 * md and b["R_TOTAL"] == a["R_TOTAL"] + 2 * md * nl
        assert (b["R_DX0"], b["R_W0"], b["O_OM"]) == (a["R_DX0"], a["R_W0"], a["O_OM"]) == (0, 4, 0)
        # every named range disjoint, inside the scratch, together tiling it
        owner = {}
        ranges = [("dx0", 0, 4), ("w0", 4, 10)]
        for k, rl in enumerate(b["R_LAYER"]):
            ranges.append((f"l{k}.omega", rl, rl + 6))
            ranges += [(f"l{k}.hidden{h}", rl + oz, rl + oz + 4) for h, oz in enumerate(b["O_Z"], start=1)]
            ranges += [(f"l{k}.u", rl + b["O_U"], rl + b["O_U"] + 2), (f"l{k}.V_in", rl + b["O_VIN"], rl + b["O_VIN"] + 18)]
        for name, lo, hi in ranges:
            for r in range(lo, hi):
                assert r not in owner, (nl, md, r, owner.get(r), name)
                owner[r] = name
        assert sorted(owner) == list(range(b["R_TOTAL"]))
    tot = {(m["NL"], m["MD"]): m["R_TOTAL"] for m in pm["maps"]}
    assert tot[(3, 3)] == 124 and tot[(3, 2)] == 112
    assert {(m["NL"], m["MD"]): m["R_TOTAL"] for m in p["maps"]}[(3, 3)] == 106


# ---------------------------------------------------------------------------- the padded model

def _read_dump(d):
    lines = open(os.path.join(d, "index.txt")).read().splitlines()
    head = lines[0].split()
    meta = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    tensors = {}
    for ln in lines[1:]:
        name, *shape = ln.split()
        tensors[name] = np.fromfile(os.path.join(d, name + ".f64"), dtype=np.float64).reshape([int(s) for s in shape])
    return meta, tensors


@pytest.mark.parametrize("l_max,md", [(2, 2), (2, 3), (1, 1)])
def test_padded_model_of_a_narrow_lx64_model(pad_exe, tmp_path, l_max, md):
    """(S 48, U 48, W 100, R 24), l_max 2 or 1 (lifted): fused_shaped_model(h, lx64, 128, 32) is (l_max 2, U 64, S 64, W 128, R 32), holds the model's weights where
    they belong and exactly zero everywhere else."""
    S, U, W, R, SF, UF, WF, RF = 48, 48, 100, 24, 64, 64, 128, 32
    cfg = dict(model_file.DEFAULT_CFG, model_dtype="float64", type_names=NAMES, l_max=l_max, num_layers=2, num_scalar_features=S, num_tensor_features=U, mlp_width=W,
               mlp_depth=md, readout_depth=1, readout_width=R, avg_num_neighbors=30.0)
    w = model_file.init_weights(cfg)
    path = str(tmp_path / "m.ahip")
    model_file.save_ahip(path, cfg, w)
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([pad_exe, path, str(out)], check=True)
    meta, got = _read_dump(str(out))
    assert meta == {"l_max": 2, "U": UF, "S": SF, "W": WF, "R": RF}
    nl0 = l_max + 1
    checked = 0
    for name, a in w.items():
        a = np.asarray(a, dtype=np.float64)
        g = got[name]
        head, leaf = name.rsplit(".", 1) if "." in name else ("", name)
        mask = np.zeros(g.shape, dtype=bool)
        if head == "tb" or head.endswith(".lat"):
            k = int(leaf[1:])
            lat = head != "tb"
            rows = np.concatenate([np.arange(S), SF + np.arange(U)]) if lat and k == 0 else np.arange(a.shape[0])
            assert g.shape == ((SF + UF if lat else a.shape[0]) if k == 0 else WF, SF if k == md else WF), (name, g.shape)
            mask[np.ix_(rows, np.arange(a.shape[1]))] = True
            assert np.array_equal(g[np.ix_(rows, np.arange(a.shape[1]))], a), name
            if k < md:
                assert not g[:, W:].any()
            if k > 0:
                assert not g[W:].any()
        elif head == "out":
            k = int(leaf[1:])
            assert g.shape == (SF if k == 0 else RF, 1 if k == 1 else RF), (name, g.shape)
            mask[: a.shape[0], : a.shape[1]] = True
            assert np.array_equal(g[: a.shape[0], : a.shape[1]], a), name
        elif name == "emb.w" or leaf == "env":
            # (l, u) columns: l U + u -> l UF + u; a lifted model gains an l = 2 block of zeros
            g3 = g.reshape(SF, 3, UF)
            assert np.array_equal(g3[:S, :nl0, :U], a.reshape(S, nl0, U)), name
            m3 = mask.reshape(SF, 3, UF)
            m3[:S, :nl0, :U] = True
        else:
            continue       # tensor-product path weights, channel mixing, per-type tables: laid out by lift_host_model / pad_host_model, covered by tests/test_fused_shapes.py
        assert not g[~mask].any(), name
        assert g[mask].any(), name
        checked += 1
    assert checked == 1 + 2 + (md + 1) * 3 + 2
