"""The second hidden width of the fused kernels' latent MLP on the CPU (csrc/fused_shapes.h: FUSED_WF2 = 128; csrc/model_io.cpp: pad_host_model; csrc/fused_rows.h and
csrc/fused_lx_rows.h: the saved-row maps of k_fused at WT = 8 and of k_fused_lx at 8 hidden rows).

All of it is host-compilable, so small stand-alone programs built here with plain g++ exercise it without a GPU:
  * the decision table of fused_shapes.h over the MLP width (64, 65, 96, 128, 129), l_max, tensor features, both depths and every arithmetic: family, width class WF,
    arithmetic, whether a compiled instance exists, and the refusal reasons, against the rule as the header's head comment states it, written independently here;
  * `pad_host_model(model, 64, UF, 128, 32)` for MLP width 72 and 128, dumped tensor by tensor and compared for exact equality with the mapping written in numpy;
  * the row maps: every named row range of a wave's scratch is disjoint from the others, inside [0, R_TOTAL), and together they tile it (R_TOTAL = last row + 1).

A model with 65 <= mlp_width <= 128 had no fused instance before the width class existed (its family was "none"): those rows are the new ground."""
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
int main() {
  const int Ws[] = {64, 65, 96, 128, 129}, Us[] = {32, 64};
  const ArithOpt opts[] = {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq};
  std::printf("[\n");
  bool first = true;
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
                    h.l_max = l; h.U = U; h.S = 64; h.mlp_width = W; h.readout_width = 32; h.mlp_depth = md; h.readout_depth = rd;
                    h.num_bessels = 8; h.num_layers = 2; h.num_types = 3; h.allow_tf32 = tf32;
                    const FusedDecision d = fused_decide(h, o, degraded != 0, false, tb != 0);
                    std::string why = d.why;
                    for (char &c : why) if (c == '"' || c == '\\') c = '\'';
                    std::printf("%s{\"W\": %d, \"l_max\": %d, \"U\": %d, \"rd\": %d, \"md\": %d, \"opt\": \"%s\", \"degraded\": %d, \"tb\": %d, \"tf32\": %d, \"family\": \"%s\", \"WF\": %d, "
                                "\"arith\": \"%s\", \"exists\": %d, \"exists64\": %d, \"wide_tile\": %d, \"why\": \"%s\"}",
                                first ? "" : ",\n", W, l, U, rd, md, arith_opt_name(o).c_str(), degraded, tb, tf32, fused_family_name(d.family), d.WF, fused_path_name(d.arith),
                                (int)fused_instance_exists(d.family, d.arith, tb != 0, md, rd, d.WF), (int)fused_instance_exists(d.family, d.arith, tb != 0, md, rd),
                                (int)fused_has_wide_tile(d.family, d.arith, md, rd, d.WF), why.c_str());
                    first = false;
                  }
  std::printf("\n]\n");
  return 0;
}
"""

PAD_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "fused_shapes.h"
#include "model_io.h"
using namespace ahip;
// usage: pad_main <model.ahip> <UF> <out dir>: every tensor of pad(model, 64, UF, 128, 32) as raw float64 in <out dir>/<name>.f64, the shapes in <out dir>/index.txt
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  try {
    const HostModel h = load_model_file(argv[1]);
    const int UF = std::atoi(argv[2]);
    const HostModel p = pad_host_model(h, 64, UF, 128, 32);
    // the same through the header's own composition, at the width class the header picks for this model
    const FusedFamily fam = fused_shape_class(h);
    if (fused_UF(fam) != UF || fused_l_run(fam) != h.l_max || fused_WF(h) != FUSED_WF2 || FUSED_WF2 != 128) return 3;
    const HostModel q = fused_shaped_model(h, fam, fused_WF(h));
    if (q.mlp_width != p.mlp_width || q.U != p.U || q.tensors.size() != p.tensors.size()) return 3;
    for (const auto &kv : p.tensors)
      if (q.get(kv.first).data != kv.second.data || q.get(kv.first).shape != kv.second.shape) return 3;
    if (fused_shape_exact(q, fam) || !fused_shape_exact(q, fam, FUSED_WF2)) return 5;
    const std::string dir = argv[3];
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

ROWS_MAIN = r"""
#include <cstdio>
#include "fused_lx_rows.h"
#include "fused_rows.h"
using namespace ahip;
static_assert(RowsXM::R_TOTAL(3, 3) > 0 && R_TOTAL(3, 3, 8) > 0 && R_LAYER(1) == 40 && R_TOTAL(3) == 88, "constexpr; the defaults are MD = 2, WT = 4");
template <class R> static void dump_lx(const char *name) {
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
  std::printf("]},\n");
}
static void dump_k_fused(int WT, bool last) {
  std::printf("\"k_fused_wt%d\": {\"WT\": %d, \"maps\": [", WT, WT);
  bool first = true;
  for (int NL = 1; NL <= 3; ++NL)
    for (int MD = 1; MD <= 3; ++MD) {
      std::printf("%s{\"NL\": %d, \"MD\": %d, \"R_Z1TB\": %d, \"R_Z2TB\": %d, \"R_U0\": %d, \"R_W0\": %d, \"O_U\": %d, \"O_VIN\": %d, \"LSZ\": %d, \"R_TOTAL\": %d, \"O_Z\": [",
                  first ? "" : ", ", NL, MD, R_Z1TB(), R_Z2TB(), R_U0(), R_W0(), R_OU(MD, WT), R_OVIN(MD, WT), R_LSZ(MD, WT), R_TOTAL(NL, MD, WT));
      for (int h = 1; h <= MD; ++h) std::printf("%s%d", h > 1 ? ", " : "", R_OZ(h, WT));
      std::printf("], \"R_LAYER\": [");
      for (int k = 0; k < NL; ++k) std::printf("%s%d", k ? ", " : "", R_LAYER(k, MD, WT));
      std::printf("]}");
      first = false;
    }
  std::printf("]}%s\n", last ? "" : ",");
}
int main() {
  std::printf("{\n");
  dump_lx<RowsX>("k_fused_lx");
  dump_lx<RowsXM>("k_fused_lx_m");
  dump_k_fused(4, false);
  dump_k_fused(8, true);
  std::printf("}\n");
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
    exe = _build(tmp_path_factory.mktemp("wshapes"), "table_main", TABLE_MAIN, ["model_io.cpp"])
    return json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())


@pytest.fixture(scope="module")
def pad_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("wpad"), "pad_main", PAD_MAIN, ["model_io.cpp"])


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("wrows"), "rows_main", ROWS_MAIN)
    return json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())


# ---------------------------------------------------------------------------- the decision table

def _expected(r):
    """(family, WF, arithmetic, the phrase the refusal must contain) by the rule as the head of fused_shapes.h states it, written independently of its code."""
    opt, l, U, md, rd, W, tb = r["opt"], r["l_max"], r["U"], r["md"], r["rd"], r["W"], r["tb"]
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
    no = ("none", 0, None)
    if W > 128:
        return no + ("MLP width 128",)
    if not (1 <= md <= 3 and 1 <= rd <= 2):
        return no + ("MLP depth 1..3 and read-out depth 1..2",)
    if W > 64:
        if fam == "lx64":
            return no + ("MLP width 65..128 has no instance of the wide fused kernel for 33..64 tensor features",)
        if ar != "fused_f16x2":
            return no + ("MLP width 65..128 runs on the f16x2 arithmetic",)
        if rd != 1:
            return no + ("MLP width 65..128 runs with read-out depth 1 only",)
        return fam, 128, ar, None
    if (md != 2 or rd != 1) and ar != "fused_f16x2":
        return no + ("runs on the f16x2 arithmetic",)
    return fam, 64, ar, None


def test_decision_table_over_the_mlp_width(table):
    assert len(table) == 5 * 2 * 2 * 4 * 5 * 5 * 2 * 2 * 2
    for r in table:
        fam, WF, ar, phrase = _expected(r)
        assert r["family"] == fam, r
        if fam != "none":
            assert (r["WF"], r["arith"], r["exists"], r["why"]) == (WF, ar, 1, ""), r
            # an instance of the other width class is not this model's: the 5-argument form asks about MLP width <= 64
            if WF == 128:
                assert r["wide_tile"] == 0, r
                assert r["exists64"] == 1, r
        else:
            assert r["why"] and r["exists"] == 0 and phrase in r["why"], (r, phrase)

    def rows(**kw):
        out = [r for r in table if all(r[k] == v for k, v in kw.items())]
        assert out
        return out

    base = dict(rd=1, opt="auto", degraded=0, tb=1, tf32=0)
    for W in (65, 96, 128):
        for md in (1, 2, 3):
            assert {(r["family"], r["WF"], r["arith"]) for r in rows(W=W, l_max=1, U=32, md=md, **base)} == {("k_fused", 128, "fused_f16x2")}
            assert {(r["family"], r["WF"], r["arith"]) for r in rows(W=W, l_max=2, U=32, md=md, **base)} == {("lx32", 128, "fused_f16x2")}
        # 33..64 tensor features, read-out depth 2, every arithmetic but f16x2, fused_tb=mlp, allow_tf32: refused, each with its own reason
        for l in (1, 2):
            for r in rows(W=W, l_max=l, U=64, md=2, **base):
                assert r["family"] == "none" and "33..64 tensor features" in r["why"], r
            for r in rows(W=W, l_max=l, U=32, md=2, **dict(base, rd=2)):
                assert r["family"] == "none" and "MLP width 65..128 runs with read-out depth 1 only" in r["why"], r
            for kw in (dict(opt="f32"), dict(opt="bf16x3"), dict(opt="tf32eq"), dict(degraded=1)):
                for r in rows(W=W, l_max=l, U=32, md=2, **dict(base, **kw)):
                    assert r["family"] == "none" and "MLP width 65..128 runs on the f16x2 arithmetic" in r["why"], r
        for kw in (dict(tb=0), dict(tf32=1)):
            for r in rows(W=W, l_max=1, U=32, md=2, **dict(base, **kw)):
                assert r["family"] == "none" and "MLP width 65..128 runs on the f16x2 arithmetic with the tabulated two-body embedding only" in r["why"], r
        # the wide kernels take no part in fused_tb / allow_tf32
        for kw in (dict(tb=0), dict(tf32=1)):
            assert {(r["family"], r["WF"]) for r in rows(W=W, l_max=2, U=32, md=2, **dict(base, **kw))} == {("lx32", 128)}
    for r in rows(W=129):
        assert r["family"] == "none" and "MLP width 128" in r["why"], r
    # nothing changes at MLP width 64: class 64, and the 128-slot tile of k_fused_lx where it was
    for r in rows(W=64):
        assert r["WF"] in (0, 64) and (r["family"] == "none") == (r["WF"] == 0), r
    assert {r["wide_tile"] for r in rows(W=64, l_max=2, U=32, md=2, **base)} == {1}
    assert {r["wide_tile"] for r in rows(W=128, l_max=2, U=32, md=2, **base)} == {0}


# ---------------------------------------------------------------------------- zero padding to hidden width 128

def pad_np(cfg, w, SF, UF, WF, RF):
    """Zero padding to the widths of a fused kernel, tensor by tensor from its NAME: the (l, u) columns move from l U + u to l UF + u, the scalars of the latent MLP's
    input behind SF, every hidden dimension of the two-body and latent MLPs goes from W to WF, of the read-out from R to RF."""
    S, U = cfg["num_scalar_features"], cfg["num_tensor_features"]
    nl, dep, rdep = cfg["l_max"] + 1, cfg["mlp_depth"], cfg["readout_depth"]

    def grow(a, r1, c1, rows=None):
        b = np.zeros((r1, c1))
        if rows is None:
            rows = np.arange(a.shape[0])
        b[rows, : a.shape[1]] = a
        return b

    out = {}
    for name, a in w.items():
        a = np.asarray(a, dtype=np.float64)
        head, leaf = name.rsplit(".", 1) if "." in name else ("", name)
        if name == "emb.w" or leaf == "env":
            b = np.zeros((SF, nl, UF)); b[:S, :, :U] = a.reshape(S, nl, U); b = b.reshape(SF, nl * UF)
        elif leaf == "tp":
            b = grow(a, a.shape[0], UF)
        elif leaf == "mix":
            b = np.zeros((nl, UF, UF)); b[:, :U, :U] = a
        elif head == "tb" or head.endswith(".lat"):
            k = int(leaf[1:])
            lat = head != "tb"
            r1 = (SF + UF if lat else a.shape[0]) if k == 0 else WF
            c1 = SF if k == dep else WF
            rows = np.concatenate([np.arange(S), SF + np.arange(U)]) if lat and k == 0 else None
            b = grow(a, r1, c1, rows)
        elif head == "out":
            k = int(leaf[1:])
            b = grow(a, SF if k == 0 else RF, 1 if k == rdep else RF)
        else:
            b = a.copy()
        out[name] = b
    return out


def _read_dump(d):
    lines = open(os.path.join(d, "index.txt")).read().splitlines()
    head = lines[0].split()
    meta = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    tensors = {}
    for ln in lines[1:]:
        name, *shape = ln.split()
        tensors[name] = np.fromfile(os.path.join(d, name + ".f64"), dtype=np.float64).reshape([int(s) for s in shape])
    return meta, tensors


@pytest.mark.parametrize("W", [72, 128])
@pytest.mark.parametrize("l_max,md,rd", [(1, 2, 1), (2, 3, 1), (1, 1, 2)])
def test_pad_to_hidden_width_128_is_the_numpy_mapping(pad_exe, tmp_path, W, l_max, md, rd):
    """S 48, U 16, read-out width 24 (W = 72) or the kernel's own S 64, U 32, read-out 32 (W = 128), 3 types, 3 layers: every tensor of pad(model, 64, 32, 128, 32)
    equals the numpy mapping exactly, and columns / rows W .. 127 of every hidden dimension are zero."""
    narrow = W == 72
    cfg = dict(model_file.DEFAULT_CFG, model_dtype="float64", type_names=NAMES, l_max=l_max, num_layers=3, num_scalar_features=48 if narrow else 64,
               num_tensor_features=16 if narrow else 32, mlp_width=W, mlp_depth=md, readout_depth=rd, readout_width=24 if narrow else 32, avg_num_neighbors=30.0)
    w = model_file.init_weights(cfg)
    path = str(tmp_path / "m.ahip")
    model_file.save_ahip(path, cfg, w)
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([pad_exe, path, "32", str(out)], check=True)
    meta, got = _read_dump(str(out))
    assert meta == {"l_max": l_max, "U": 32, "S": 64, "W": 128, "R": 32}
    want = pad_np(cfg, w, 64, 32, 128, 32)
    assert set(got) == set(want)
    for name in sorted(want):
        assert got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), name
    S, U = cfg["num_scalar_features"], cfg["num_tensor_features"]
    for pre in ["tb"] + [f"l{k}.lat" for k in (1, 2, 3)]:
        a0 = got[f"{pre}.w0"]
        assert a0.shape[1] == 128 and not a0[:, W:].any() and a0[:, :W].any()
        if pre != "tb":        # [x (64), scalars (32)] -> 128: the model's scalar rows S .. S + U - 1 sit behind the 64 latent rows
            assert a0.shape[0] == 96 and np.array_equal(a0[64: 64 + U, :W], np.asarray(w[f"{pre}.w0"])[S:]) and not a0[S:64].any() and not a0[64 + U:].any()
        for k in range(1, md):
            a = got[f"{pre}.w{k}"]
            assert a.shape == (128, 128) and not a[W:].any() and not a[:, W:].any()
        al = got[f"{pre}.w{md}"]
        assert al.shape == (128, 64) and not al[W:].any() and np.array_equal(al[:W, :S], np.asarray(w[f"{pre}.w{md}"]))


# ---------------------------------------------------------------------------- saved-row maps

def _ranges_lx(shape, m):
    ew, hr, ur, nv = shape["EW"], shape["HR"], shape["UR"], shape["NV"]
    out = [("dx0", m["R_DX0"], m["R_DX0"] + 4), ("w0", m["R_W0"], m["R_W0"] + ew)]
    for k, rl in enumerate(m["R_LAYER"]):
        out.append((f"l{k}.omega", rl + m["O_OM"], rl + m["O_OM"] + ew))
        for h, oz in enumerate(m["O_Z"], start=1):
            out.append((f"l{k}.hidden{h}", rl + oz, rl + oz + hr))
        out.append((f"l{k}.u", rl + m["O_U"], rl + m["O_U"] + ur))
        out.append((f"l{k}.V_in", rl + m["O_VIN"], rl + m["O_VIN"] + nv))
    return out


def _ranges_k_fused(shape, m):
    wt = shape["WT"]
    out = [("dx0", m["R_Z1TB"], m["R_Z1TB"] + 4), ("z2tb", m["R_Z2TB"], m["R_Z2TB"] + 4), ("u0", m["R_U0"], m["R_U0"] + 4), ("w0", m["R_W0"], m["R_W0"] + 4)]
    for k, rl in enumerate(m["R_LAYER"]):
        out.append((f"l{k}.omega", rl, rl + 4))
        for h, oz in enumerate(m["O_Z"], start=1):
            out.append((f"l{k}.hidden{h}", rl + oz, rl + oz + wt))
        out.append((f"l{k}.u", rl + m["O_U"], rl + m["O_U"] + 4))
        out.append((f"l{k}.V_in", rl + m["O_VIN"], rl + m["O_VIN"] + 8))
    return out


@pytest.mark.parametrize("kernel", ["k_fused_lx", "k_fused_lx_m", "k_fused_wt4", "k_fused_wt8"])
def test_row_ranges_are_disjoint_and_tile_the_scratch(maps, kernel):
    shape = maps[kernel]
    ranges = _ranges_lx if kernel.startswith("k_fused_lx") else _ranges_k_fused
    seen = set()
    for m in shape["maps"]:
        seen.add((m["NL"], m["MD"]))
        assert len(m["O_Z"]) == m["MD"] and len(m["R_LAYER"]) == m["NL"]
        owner = {}
        for name, lo, hi in ranges(shape, m):
            assert 0 <= lo < hi <= m["R_TOTAL"], (kernel, m["NL"], m["MD"], name, lo, hi)
            for r in range(lo, hi):
                assert r not in owner, f"{kernel} NL={m['NL']} MD={m['MD']}: row {r} belongs to {owner[r]} and {name}"
                owner[r] = name
        assert sorted(owner) == list(range(m["R_TOTAL"])), f"{kernel} NL={m['NL']} MD={m['MD']}: rows without an owner"
        assert m["R_TOTAL"] == max(owner) + 1
        for a, b in zip(m["R_LAYER"], m["R_LAYER"][1:]):
            assert b - a == m["LSZ"]
    assert seen == {(nl, md) for nl in (1, 2, 3) for md in (1, 2, 3)}


def test_row_maps_at_hidden_width_64_are_the_ones_the_kernels_had(maps):
    """WT = 4 / 4 hidden rows reproduce the indices of the kernels before the width parameter existed; 8 rows per hidden layer add exactly 4 MD rows per layer."""
    for m in maps["k_fused_wt4"]["maps"]:
        md, nl = m["MD"], m["NL"]
        assert (m["R_Z1TB"], m["R_Z2TB"], m["R_U0"], m["R_W0"]) == (0, 4, 8, 12)
        assert m["O_Z"] == [4 * h for h in range(1, md + 1)] and m["O_U"] == 4 + 4 * md and m["O_VIN"] == 8 + 4 * md and m["LSZ"] == 16 + 4 * md
        assert m["R_LAYER"] == [16 + (16 + 4 * md) * k for k in range(nl)] and m["R_TOTAL"] == 16 + (16 + 4 * md) * nl
    for a, b in zip(maps["k_fused_wt4"]["maps"], maps["k_fused_wt8"]["maps"]):
        assert (a["NL"], a["MD"]) == (b["NL"], b["MD"])
        assert b["LSZ"] == a["LSZ"] + 4 * a["MD"] and b["R_TOTAL"] == a["R_TOTAL"] + 4 * a["MD"] * a["NL"]
        assert b["O_Z"] == [4 + 8 * (h - 1) for h in range(1, b["MD"] + 1)]
    x, xm = maps["k_fused_lx"], maps["k_fused_lx_m"]
    assert (x["EW"], x["HR"], x["UR"], x["NV"]) == (6, 4, 4, 18) and (xm["EW"], xm["HR"], xm["UR"], xm["NV"]) == (6, 8, 4, 18)
    for a, b in zip(x["maps"], xm["maps"]):
        assert a["LSZ"] == 6 + 4 * (a["MD"] + 1) + 18 and a["O_VIN"] == 6 + 4 * (a["MD"] + 1)
        assert b["LSZ"] == a["LSZ"] + 4 * a["MD"] and b["R_TOTAL"] == a["R_TOTAL"] + 4 * a["MD"] * a["NL"]
    assert [m["R_TOTAL"] for m in x["maps"] if (m["NL"], m["MD"]) == (3, 2)] == [118]
