"""Active types on the CPU: a model of more than 16 types runs its fused side on the slice at the types the simulation uses (csrc/model_io.cpp: subset_host_model,
csrc/fused_shapes.h: the gates count active types, include/allegro_hip.h: ahip_set_active_types / ahip_get_active_types).

  * subset_host_model, built into a stand-alone g++ program, against model_file.subset_types (numpy) for exact equality, its order against pad_host_model /
    lift_host_model, and the lists it must refuse;
  * the premise: the float64 oracle of a 20-type model on atoms of three of its types equals the oracle of the 3-type slice with difference 0.0;
  * the shape rule with an active count: T = 20 with 3, 16 and 17 active types, T = 300, and the count left out (today's answer for every row of the table of
    tests/test_fused_shapes.py);
  * the C entry points on the emulation library: round trip, error cases, the automatic set of a 20-type model, and the NVE helpers with a 20-entry mass table."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import util
from pair_allegro_amd import capi, lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pair_allegro_amd", "csrc")
NAMES20 = ["H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar", "Cu", "Ag"]
ACTIVE = [7, 18, 19]
PAIR_NAMES = ["Ag", "Cu", "O"]

SUBSET_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>
#include "fused_shapes.h"
#include "model_io.h"
using namespace ahip;
static bool same(const HostModel &a, const HostModel &b) {
  if (a.num_types != b.num_types || a.type_names != b.type_names || a.type_names_joined != b.type_names_joined || a.per_edge_type_cutoff != b.per_edge_type_cutoff ||
      a.l_max != b.l_max || a.U != b.U || a.S != b.S || a.mlp_width != b.mlp_width || a.readout_width != b.readout_width || a.tensors.size() != b.tensors.size()) return false;
  for (const auto &kv : a.tensors)
    if (b.get(kv.first).shape != kv.second.shape || b.get(kv.first).data != kv.second.data) return false;
  return true;
}
// usage: subset_main dump <model.ahip> <out dir> t0 t1 ...   every tensor of subset_host_model(model, {t...}) as raw float64, shapes and metadata in index.txt
//        subset_main order <model.ahip> t0 t1 ...            subset then pad / lift against pad / lift then subset: exit 0 when equal
//        subset_main throws <model.ahip> t0 t1 ...           exit 0 when subset_host_model refuses the list with std::runtime_error
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  try {
    const HostModel h = load_model_file(argv[2]);
    std::vector<int> act;
    for (int k = mode == "dump" ? 4 : 3; k < argc; ++k) act.push_back(std::atoi(argv[k]));
    if (mode == "throws") {
      try { (void)subset_host_model(h, act); } catch (const std::runtime_error &) { return 0; }
      return 3;
    }
    const HostModel p = subset_host_model(h, act);
    if (mode == "order") {
      if (!same(pad_host_model(p, 64, 32, 64, 32), subset_host_model(pad_host_model(h, 64, 32, 64, 32), act))) return 3;
      if (!same(lift_host_model(p, 2), subset_host_model(lift_host_model(h, 2), act))) return 4;
      if (!same(fused_shaped_model(p, FusedFamily::lx64), subset_host_model(fused_shaped_model(h, FusedFamily::lx64), act))) return 5;
      return 0;
    }
    const std::string dir = argv[3];
    FILE *idx = std::fopen((dir + "/index.txt").c_str(), "w");
    if (!idx) return 4;
    std::fprintf(idx, "num_types %d\ntype_names %s\ncutoffs", p.num_types, p.type_names_joined.c_str());
    for (double v : p.per_edge_type_cutoff) std::fprintf(idx, " %.17g", v);
    std::fprintf(idx, "\nnames_vector");
    for (const std::string &s : p.type_names) std::fprintf(idx, " %s", s.c_str());
    std::fprintf(idx, "\nshape l_max %d U %d S %d W %d R %d B %d layers %d\n", p.l_max, p.U, p.S, p.mlp_width, p.readout_width, p.num_bessels, p.num_layers);
    for (const auto &kv : p.tensors) {
      std::fprintf(idx, "tensor %s", kv.first.c_str());
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

# rows: (T, A or -1 for "left out"); and the whole table of tests/test_fused_shapes.py with the count left out, given as -1 and given as T: three equal answers
SHAPES_MAIN = r"""
#include <cstdio>
#include "fused_shapes.h"
using namespace ahip;
static HostModel shape(int l, int U, int T) {
  HostModel h;
  h.l_max = l; h.U = U; h.S = 64; h.mlp_width = 64; h.readout_width = 32; h.mlp_depth = 2; h.readout_depth = 1;
  h.num_bessels = 8; h.num_layers = 2; h.num_types = T;
  return h;
}
int main() {
  const int rows[][2] = {{20, 3}, {20, 16}, {20, 17}, {20, -1}, {20, 20}, {300, 3}, {300, -1}, {255, 16}, {16, -1}, {16, 16}, {3, 2}};
  std::printf("{\"rows\": [\n");
  bool first = true;
  for (const auto &r : rows)
    for (int l = 1; l <= 2; ++l)
      for (int U : {32, 64}) {
        const HostModel h = shape(l, U, r[0]);
        const FusedDecision d = r[1] == -1 ? fused_decide(h, ArithOpt::Auto, false, false, true) : fused_decide(h, ArithOpt::Auto, false, false, true, r[1]);
        std::string why = d.why;
        for (char &c : why) if (c == '"' || c == '\\') c = '\'';
        std::printf("%s{\"T\": %d, \"A\": %d, \"l_max\": %d, \"U\": %d, \"family\": \"%s\", \"why\": \"%s\"}", first ? "" : ",\n", r[0], r[1], l, U, fused_family_name(d.family), why.c_str());
        first = false;
      }
  // the table of tests/test_fused_shapes.py: the count left out == -1 == the model's own
  const int Us[] = {16, 32, 33, 64, 65};
  const ArithOpt opts[] = {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq};
  int n = 0, bad = 0;
  for (int l = 0; l <= 3; ++l)
    for (int U : Us)
      for (int rd = 0; rd <= 3; ++rd)
        for (int md = 0; md <= 4; ++md)
          for (ArithOpt o : opts)
            for (int degraded = 0; degraded <= 1; ++degraded)
              for (int T : {3, 16, 17}) {
                HostModel h = shape(l, U, T);
                h.mlp_depth = md; h.readout_depth = rd;
                const FusedDecision a = fused_decide(h, o, degraded != 0, false, true), b = fused_decide(h, o, degraded != 0, false, true, -1),
                                    c = fused_decide(h, o, degraded != 0, false, true, T);
                ++n;
                if (a.family != b.family || a.family != c.family || a.why != b.why || a.why != c.why || a.arith != b.arith || a.arith != c.arith) ++bad;
                std::string w1, w2;
                const bool s1 = fused_narrow_supported(h, a.arith, true, &w1), s2 = fused_narrow_supported(h, a.arith, true, &w2, T);
                const bool x1 = fused_wide_supported(h, a.arith, &w1), x2 = fused_wide_supported(h, a.arith, &w2, T);
                if (s1 != s2 || x1 != x2 || w1 != w2) ++bad;
              }
  std::printf("\n], \"table_rows\": %d, \"table_mismatches\": %d}\n", n, bad);
  return 0;
}
"""


def _build(d, name, text, sources=()):
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(text)
    # plain host compiler, no HIP include path: header and model_io.cpp must stand on their own
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src)] + [os.path.join(CSRC, s) for s in sources] + ["-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def subset_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("subset"), "subset_main", SUBSET_MAIN, ["model_io.cpp"])


def _cutoffs20(r_max):
    """a different cutoff for every ordered type pair, all within r_max"""
    T = len(NAMES20)
    return (r_max - 0.002 * np.arange(T * T, dtype=np.float64)).reshape(T, T).tolist()


def _small20(**over):
    return dict(dict(model_file.DEFAULT_CFG, model_dtype="float64", type_names=list(NAMES20), l_max=1, num_layers=2, num_scalar_features=48, num_tensor_features=16,
                     mlp_width=40, readout_width=24, avg_num_neighbors=30.0), **over)


def _read_dump(d):
    meta, tensors = {}, {}
    for line in open(os.path.join(d, "index.txt")):
        tok = line.split()
        if tok[0] == "tensor":
            shape = tuple(int(t) for t in tok[2:])
            tensors[tok[1]] = np.fromfile(os.path.join(d, tok[1] + ".f64"), dtype=np.float64).reshape(shape)
        else:
            meta[tok[0]] = tok[1:]
    return meta, tensors


@pytest.mark.parametrize("cutoffs", [False, True])
def test_subset_host_model_equals_numpy_slice(subset_exe, tmp_path, cutoffs):
    cfg = _small20(per_edge_type_cutoff=_cutoffs20(5.0) if cutoffs else None)
    w = model_file.init_weights(cfg)
    path = str(tmp_path / "m20.ahip")
    model_file.save_ahip(path, cfg, w)
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([subset_exe, "dump", path, str(out)] + [str(t) for t in ACTIVE], check=True)
    meta, tensors = _read_dump(str(out))
    # names in any order and repeated: the slice keeps model order
    cfg3, w3 = model_file.subset_types(cfg, w, ["Cu", "O", "Ag", "O"])
    assert cfg3["type_names"] == ["O", "Cu", "Ag"] == meta["type_names"] == meta["names_vector"]
    assert int(meta["num_types"][0]) == 3
    if cutoffs:
        pc = np.asarray(cfg["per_edge_type_cutoff"])
        assert cfg3["per_edge_type_cutoff"] == [[pc[a, b] for b in ACTIVE] for a in ACTIVE]
        assert [float(v) for v in meta["cutoffs"]] == list(np.asarray(cfg3["per_edge_type_cutoff"]).reshape(-1))
    else:
        assert cfg3["per_edge_type_cutoff"] is None and meta["cutoffs"] == []
    assert set(tensors) == set(w3) == {n for n, _ in model_file.tensor_shapes(cfg3)}
    for name, shape in model_file.tensor_shapes(cfg3):
        assert tensors[name].shape == tuple(shape) == w3[name].shape, name
        assert (tensors[name] == w3[name]).all(), name                          # exact: rows are copied, nothing is computed
    # the rows themselves, spelled out once more: centre one-hots, neighbour one-hots, Bessel rows
    T, B = 20, cfg["num_bessels"]
    assert (w3["tb.w0"] == w["tb.w0"][ACTIVE + [T + t for t in ACTIVE] + list(range(2 * T, 2 * T + B))]).all()
    # every tensor without a type axis is the model's own
    for name in w:
        if name not in ("tb.w0", "scale", "shift"):
            assert (w3[name] == w[name]).all()
    # a slice is a model file like any other
    p3 = str(tmp_path / "m3.ahip")
    model_file.save_ahip(p3, cfg3, w3)
    cfg3b, w3b = model_file.load(p3)
    assert cfg3b["type_names"] == cfg3["type_names"] and all((w3b[k] == w3[k]).all() for k in w3)


def test_subset_commutes_with_padding_and_lifting(subset_exe, tmp_path):
    cfg = _small20(per_edge_type_cutoff=_cutoffs20(5.0))
    path = str(tmp_path / "m20.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    subprocess.run([subset_exe, "order", path] + [str(t) for t in ACTIVE], check=True)
    subprocess.run([subset_exe, "order", path] + [str(t) for t in range(20)], check=True)      # the identity slice


@pytest.mark.parametrize("active", [[18, 7, 19], [7, 7, 18], [7, 18, 20], [-1, 7], []])
def test_subset_host_model_refuses(subset_exe, tmp_path, active):
    cfg = _small20()
    path = str(tmp_path / "m20.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    subprocess.run([subset_exe, "throws", path] + [str(t) for t in active], check=True)


def test_subset_types_refuses_unknown_names():
    cfg = _small20()
    with pytest.raises(ValueError):
        model_file.subset_types(cfg, model_file.init_weights(cfg), ["Cu", "Pd"])


@pytest.mark.parametrize("kind", ["S", "L32"])
def test_oracle_of_the_slice_is_the_oracle_of_the_model(kind):
    """The premise of the feature, in float64: atoms of three of a model's twenty types see exactly the 3-type model sliced out of it."""
    g = util.load_golden("Cu2AgO4_r5")
    nb = float(g["nedges"]) / len(g["pos"])
    base = dict(type_names=list(NAMES20), avg_num_neighbors=nb, r_max=5.0, num_layers=2, model_dtype="float64")
    cfg = model_file.model_S(**base) if kind == "S" else model_file.model_L(**dict(base, num_tensor_features=32))
    w = model_file.init_weights(cfg)
    cfg3, w3 = model_file.subset_types(cfg, w, PAIR_NAMES)
    types = np.array([PAIR_NAMES.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    full = util.oracle_run(cfg, w, g["cell"], g["pos"], types, PAIR_NAMES)
    part = util.oracle_run(cfg3, w3, g["cell"], g["pos"], types, PAIR_NAMES)
    assert np.abs(full["forces"]).max() > 1e-3
    assert np.abs(full["forces"] - part["forces"]).max() == 0.0
    assert np.abs(full["eatom"] - part["eatom"]).max() == 0.0
    assert np.abs(np.asarray(full["virial"]) - np.asarray(part["virial"])).max() == 0.0
    assert float(full["pe"]) - float(part["pe"]) == 0.0


def test_shape_rule_counts_active_types(tmp_path):
    exe = _build(tmp_path, "shapes_main", SHAPES_MAIN, ["model_io.cpp"])
    out = json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())
    assert out["table_rows"] > 1000 and out["table_mismatches"] == 0
    served = {(1, 32): "k_fused", (1, 64): "lx64", (2, 32): "lx32", (2, 64): "lx64"}
    for r in out["rows"]:
        T, A, fam, why = r["T"], r["A"], r["family"], r["why"]
        key = (r["l_max"], r["U"])
        n = T if A == -1 else A
        if T > 255 and A not in (-1, T):
            assert fam == "none" and "at most 255 types" in why and str(T) in why, r
        elif n > 16:
            assert fam == "none", r
            assert f"at most 16 active model types ({n} of the model's {T} are mapped)" in why, r
        else:
            assert fam == served[key] and why == "", r


# ---------------------------------------------------------------------------------------------- emulation library
def _emu_pair(emu_lib, path, names):
    pair = PairAllegro(me=0, nprocs=1, lib=emu_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", path] + list(names), ntypes=len(names))
    pair.init_style()
    return pair


def _evaluate(pair, cfg, g, names):
    types = np.array([list(names).index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    rs = lmp_like.build_rank_system(g["cell"], g["pos"], types, cfg["r_max"] + 1.0)
    atom = atom_from_rank_system(rs, len(names))
    pair.compute(atom, list_from_rank_system(rs))
    return atom.f.copy(), float(pair.eng_vdwl)


@pytest.mark.parametrize("dtype,path_name", [("float64", "generic_f64"), ("float32", "generic_f32")])
def test_emulation_reports_the_mappers_set_for_a_20_type_model(emu_lib, tmp_path, dtype, path_name):
    g = util.load_golden("Cu2AgO4_r5")
    cfg = _small20(model_dtype=dtype)
    path = str(tmp_path / "m20.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    pair = _emu_pair(emu_lib, path, ["O", "Ag", "Cu", "O"])          # four LAMMPS types, two of them one model type, not in model order
    m = pair.model
    assert m.get_active_types() == []                                # nothing evaluated yet
    f_auto, e_auto = _evaluate(pair, cfg, g, ["O", "Ag", "Cu", "O"])
    assert m.last_path == path_name
    assert m.get_active_types() == ACTIVE
    # an explicit set wins over the mapper's; the layer-at-a-time kernels see full types either way
    m.set_active_types([19, 3, 7, 18, 7])
    f_set, e_set = _evaluate(pair, cfg, g, ["O", "Ag", "Cu", "O"])
    assert m.get_active_types() == [3, 7, 18, 19]
    assert (f_set == f_auto).all() and e_set == e_auto
    m.set_active_types([])                                           # back to automatic
    _evaluate(pair, cfg, g, ["O", "Ag", "Cu", "O"])
    assert m.get_active_types() == ACTIVE
    m.close()


def test_emulation_small_model_has_no_subset_unless_set(emu_lib, tmp_path):
    g = util.load_golden("Cu2AgO4_r5")
    cfg = dict(_small20(), type_names=["Ag", "Cu", "O"])
    path = str(tmp_path / "m3.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    pair = _emu_pair(emu_lib, path, PAIR_NAMES)
    m = pair.model
    _evaluate(pair, cfg, g, PAIR_NAMES)
    assert m.get_active_types() == []                                # at most 16 types: the mapper does not make a subset
    m.set_active_types([2, 0, 1, 1])
    _evaluate(pair, cfg, g, PAIR_NAMES)
    assert m.get_active_types() == [0, 1, 2]
    for bad in ([3], [-1], [0, 1, 99]):
        with pytest.raises(capi.AhipError) as e:
            m.set_active_types(bad)
        assert e.value.code == capi.AHIP_ERR_ARG and "outside the model's 3 types" in e.value.msg
    assert m.get_active_types() == [0, 1, 2]                         # a refused call changes nothing
    n = C.c_int(-1)
    assert emu_lib.lib.ahip_get_active_types(m.h, C.byref(n), None) == 0 and n.value == 3      # the count alone
    assert emu_lib.lib.ahip_get_active_types(m.h, None, None) == capi.AHIP_ERR_ARG
    assert emu_lib.lib.ahip_set_active_types(m.h, 2, None) == capi.AHIP_ERR_ARG
    assert emu_lib.lib.ahip_set_active_types(m.h, -1, None) == capi.AHIP_ERR_ARG
    assert emu_lib.lib.ahip_set_active_types(None, 0, None) == capi.AHIP_ERR_ARG
    m.close()


def test_emulation_nve_with_a_20_type_mass_table(emu_lib, tmp_path):
    """ahip_nve_dev / ahip_nve_first_dev take any number of model types (the emulation's device pointers are host pointers): against velocity Verlet in numpy."""
    cfg = _small20()
    path = str(tmp_path / "m20.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    m = capi.Model(path, 0, emu_lib)
    rng = np.random.RandomState(5)
    n, nall, dt, ftm2v = 37, 45, 0.002, 1.0 / 1.0364269e-4
    mass = 1.0 + np.arange(20, dtype=np.float64) * 3.7
    mt = (np.arange(nall) * 7 % 20).astype(np.int32)
    assert mt[:n].max() > 15
    for mode in (0, 1, "first"):
        x, v, f = rng.normal(size=(nall, 3)), rng.normal(size=(nall, 3)), rng.normal(size=(nall, 3))
        x0, v0, f0 = x.copy(), v.copy(), f.copy()
        if mode == "first":
            m.nve_first_dev(n, nall, x.ctypes.data, v.ctypes.data, f.ctypes.data, mt.ctypes.data, mass, dt, ftm2v)
        else:
            m.nve_dev(mode, n, x.ctypes.data, v.ctypes.data, f.ctypes.data, mt.ctypes.data, mass, dt, ftm2v)
        vv = v0[:n] + ((0.5 * dt * ftm2v) * (1.0 / mass[mt[:n]]))[:, None] * f0[:n]
        np.testing.assert_allclose(v[:n], vv, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(x[:n], x0[:n] + dt * vv if mode != 1 else x0[:n], rtol=1e-13, atol=1e-13)
        assert (v[n:] == v0[n:]).all() and (x[n:] == x0[n:]).all()
        assert (f == 0).all() if mode == "first" else (f == f0).all()
        mass = mass * 1.5                                            # a changed table is uploaded again
    m.close()
