"""The shape rule of the fused kernels on the CPU (csrc/fused_shapes.h, csrc/model_io.cpp: lift_host_model).

Both are host-compilable, so small stand-alone programs built here with plain g++ exercise them without a GPU:
  * `lift_host_model(h, 2)` followed by `pad_host_model(.., 64, 64, 64, 32)` -- what k_fused_lx2 runs for an l_max = 1 model with 33..64 tensor features -- is dumped
    tensor by tensor and compared, for exact equality, with the same mapping written in numpy from cg.tp_paths;
  * the numpy-lifted model, saved as an ordinary l_max = 2 file, is evaluated by the emulated float64 layer-at-a-time kernels beside the original: the same forces, energies
    and virial to 1e-12 of their scale (the bar of test_emu_parity.py: test_zero_padded_model_is_the_same_model);
  * the decision table of fused_shapes.h (family, shape the kernel runs at, refusal reason) over l_max, tensor features, both depths and every arithmetic."""
import json
import os
import subprocess

import numpy as np
import pytest

import util
from pair_allegro_amd import cg, lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pair_allegro_amd", "csrc")
NAMES = ["Ag", "Cu", "O"]

LIFT_MAIN = r"""
#include <cstdio>
#include <string>
#include "fused_shapes.h"
#include "model_io.h"
using namespace ahip;
// usage: lift_main <model.ahip> <out dir>: every tensor of pad(lift(model, 2), 64, 64, 64, 32) as raw float64 in <out dir>/<name>.f64, the shapes in <out dir>/index.txt
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  try {
    const HostModel h = load_model_file(argv[1]);
    const HostModel l = lift_host_model(h, 2);
    const HostModel p = pad_host_model(l, 64, 64, 64, 32);
    // the same through the header's own composition
    const HostModel q = fused_shaped_model(h, FusedFamily::lx64);
    if (q.l_max != p.l_max || q.U != p.U || q.tensors.size() != p.tensors.size()) return 3;
    for (const auto &kv : p.tensors)
      if (q.get(kv.first).data != kv.second.data || q.get(kv.first).shape != kv.second.shape) return 3;
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

TABLE_MAIN = r"""
#include <cstdio>
#include "fused_shapes.h"
using namespace ahip;
int main() {
  const int Us[] = {16, 32, 33, 64, 65};
  const ArithOpt opts[] = {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq};
  std::printf("[\n");
  bool first = true;
  for (int l = 0; l <= 3; ++l)
    for (int U : Us)
      for (int rd = 0; rd <= 3; ++rd)
        for (int md = 0; md <= 4; ++md)
          for (ArithOpt o : opts)
            for (int degraded = 0; degraded <= 1; ++degraded) {
              HostModel h;
              h.l_max = l; h.U = U; h.S = 64; h.mlp_width = 64; h.readout_width = 32; h.mlp_depth = md; h.readout_depth = rd;
              h.num_bessels = 8; h.num_layers = 2; h.num_types = 3;
              const FusedDecision d = fused_decide(h, o, degraded != 0, false, true);
              std::string why = d.why;
              for (char &c : why) if (c == '"' || c == '\\') c = '\'';
              std::printf("%s{\"l_max\": %d, \"U\": %d, \"rd\": %d, \"md\": %d, \"opt\": \"%s\", \"degraded\": %d, \"family\": \"%s\", \"l_run\": %d, \"UF\": %d, \"arith\": \"%s\", \"exists\": %d, \"why\": \"%s\"}",
                          first ? "" : ",\n", l, U, rd, md, arith_opt_name(o).c_str(), degraded, fused_family_name(d.family), d.l_run, d.UF, fused_path_name(d.arith),
                          (int)fused_instance_exists(d.family, d.arith, true, md, rd), why.c_str());
              first = false;
            }
  std::printf("\n]\n");
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
def lift_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("lift"), "lift_main", LIFT_MAIN, ["model_io.cpp"])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("shapes"), "table_main", TABLE_MAIN, ["model_io.cpp"])
    return json.loads(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode())


def _cfg(nl, U=40, **over):
    return dict(model_file.DEFAULT_CFG, model_dtype="float64", type_names=NAMES, l_max=1, num_layers=nl, num_scalar_features=48, num_tensor_features=U,
                mlp_width=40, readout_width=24, avg_num_neighbors=30.0, **over)


def lift_np(cfg, w, LF):
    """The model as an l_max = LF model: zero (l, u) columns, tp rows by (l1, l2, l3), zero mixing blocks."""
    L, U, NL = cfg["l_max"], cfg["num_tensor_features"], cfg["num_layers"]
    c2 = dict(cfg, l_max=LF)
    w2 = {k: np.array(v, dtype=np.float64) for k, v in w.items()}

    def widen(a):
        out = np.zeros((a.shape[0], U * (LF + 1)))
        out[:, : U * (L + 1)] = a
        return out

    w2["emb.w"] = widen(w2["emb.w"])
    for k in range(1, NL + 1):
        w2[f"l{k}.env"] = widen(w2[f"l{k}.env"])
        src, dst = cg.tp_paths(L, scalar_only=k == NL), cg.tp_paths(LF, scalar_only=k == NL)
        tp = np.zeros((len(dst), U))
        for p, path in enumerate(src):
            tp[dst.index(path)] = w2[f"l{k}.tp"][p]
        w2[f"l{k}.tp"] = tp
        if k < NL:
            mix = np.zeros((LF + 1, U, U))
            mix[: L + 1] = w2[f"l{k}.mix"]
            w2[f"l{k}.mix"] = mix
    return c2, w2


def pad_np(cfg, w, SF, UF, WF, RF):
    """Zero padding to the widths of a fused kernel; the (l, u) columns move from l U + u to l UF + u, the scalars of the latent MLP's input behind SF."""
    S, U, W, R = cfg["num_scalar_features"], cfg["num_tensor_features"], cfg["mlp_width"], cfg["readout_width"]
    nl = cfg["l_max"] + 1
    out = {}
    for name, a in w.items():
        a = np.asarray(a, dtype=np.float64)
        leaf = name.split(".")[-1]
        if name == "emb.w" or leaf == "env":
            b = np.zeros((SF, nl, UF)); b[:S, :, :U] = a.reshape(S, nl, U); b = b.reshape(SF, nl * UF)
        elif leaf == "tp":
            b = np.zeros((a.shape[0], UF)); b[:, :U] = a
        elif leaf == "mix":
            b = np.zeros((nl, UF, UF)); b[:, :U, :U] = a
        elif a.ndim == 2:
            r1 = {S: SF, W: WF, R: RF, S + U: SF + UF}.get(a.shape[0], a.shape[0]) if not name.startswith("tb.w0") else a.shape[0]
            c1 = {S: SF, W: WF, R: RF}.get(a.shape[1], a.shape[1])
            b = np.zeros((r1, c1))
            if a.shape[0] == S + U and ".lat.w0" in name:
                b[:S, : a.shape[1]] = a[:S]; b[SF: SF + U, : a.shape[1]] = a[S:]
            else:
                b[: a.shape[0], : a.shape[1]] = a
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


@pytest.mark.parametrize("nl", [1, 2, 3])
def test_lift_and_pad_is_the_numpy_mapping(lift_exe, tmp_path, nl):
    """l_max = 1, U = 40, 3 types, `nl` layers: every tensor of pad(lift(model, 2), 64, 64, 64, 32) equals the numpy mapping exactly; every `tp` row of a path with an
    l = 2 leg is zero; column l * 64 + u of emb.w / env holds the source's l * 40 + u."""
    cfg = _cfg(nl)
    assert len({cfg["num_scalar_features"], cfg["mlp_width"], cfg["readout_width"], cfg["num_scalar_features"] + 40, 2 * 3 + cfg["num_bessels"]}) == 5     # pad_np tells the dimensions apart by size
    w = model_file.init_weights(cfg)
    path = str(tmp_path / "m.ahip")
    model_file.save_ahip(path, cfg, w)
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([lift_exe, path, str(out)], check=True)
    meta, got = _read_dump(str(out))
    assert meta == {"l_max": 2, "U": 64, "S": 64, "W": 64, "R": 32}
    c2, w2 = lift_np(cfg, w, 2)
    want = pad_np(c2, w2, 64, 64, 64, 32)
    assert set(got) == set(want)
    for name in sorted(want):
        assert got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), name
    for k in range(1, nl + 1):
        paths = cg.tp_paths(2, scalar_only=k == nl)
        tp = got[f"l{k}.tp"]
        assert tp.shape == (len(paths), 64)
        src = cg.tp_paths(1, scalar_only=k == nl)
        for p, path3 in enumerate(paths):
            if 2 in path3:
                assert not tp[p].any(), (k, path3)
            else:
                assert np.array_equal(tp[p, :40], w[f"l{k}.tp"][src.index(path3)]) and not tp[p, 40:].any()
        for name in ["emb.w", f"l{k}.env"]:
            a = got[name]
            for l in range(3):
                blk = a[:48, l * 64: l * 64 + 40]
                if l < 2:
                    assert np.array_equal(blk, np.asarray(w[name])[:, l * 40: l * 40 + 40]), (name, l)
                else:
                    assert not a[:, l * 64:].any(), name
                assert not a[:, l * 64 + 40: (l + 1) * 64].any() and not a[48:].any()
        if k < nl:
            assert not got[f"l{k}.mix"][2].any()


@pytest.mark.parametrize("nl", [1, 2, 3])
def test_lifted_model_is_the_same_model(emu_lib, model_dir, nl):
    """The numpy-lifted model saved as an l_max = 2 file against the original on the emulated float64 layer-at-a-time kernels, Cu2AgO4."""
    g = util.load_golden("Cu2AgO4_r5")
    cfg = _cfg(nl)
    w = model_file.init_weights(cfg)
    c2, w2 = lift_np(cfg, w, 2)
    assert [(n, tuple(w2[n].shape)) for n, _ in model_file.tensor_shapes(c2)] == model_file.tensor_shapes(c2)
    types = np.array([NAMES.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    rs = lmp_like.build_rank_system(g["cell"], g["pos"], types, cfg["r_max"] + 1.0)
    out = []
    for tag, c, ww in (("l1", cfg, w), ("l2", c2, w2)):
        path = f"{model_dir}/lift_{tag}_nl{nl}.ahip"
        model_file.save_ahip(path, c, ww)
        pair = PairAllegro(lib=emu_lib, quiet=True)
        pair.settings([])
        pair.coeff(["*", "*", path] + NAMES, ntypes=3)
        atom = atom_from_rank_system(rs, 3)
        pair.compute(atom, list_from_rank_system(rs))
        assert pair.model.last_path == "generic_f64"
        out.append((atom.f.copy(), pair.eatom[: rs.nlocal].copy(), pair.eng_vdwl, np.array(pair.virial)))
        pair.model.close()
    (f0, e0, pe0, v0), (f1, e1, pe1, v1) = out
    assert np.abs(f0).max() > 1e-3
    np.testing.assert_allclose(f1, f0, rtol=0, atol=1e-12 * max(1.0, np.abs(f0).max()))
    np.testing.assert_allclose(e1, e0, rtol=0, atol=1e-12 * max(1.0, np.abs(e0).max()))
    np.testing.assert_allclose(pe1, pe0, rtol=0, atol=1e-12 * max(1.0, abs(pe0)))
    np.testing.assert_allclose(v1, v0, rtol=0, atol=1e-12 * max(1.0, np.abs(v0).max()))


def _expected(r):
    """The rule as the documentation states it (fused_shapes.h header comment), written independently of the header's code."""
    opt, l, U, md, rd = r["opt"], r["l_max"], r["U"], r["md"], r["rd"]
    f16 = opt == "f16x2" or (opt == "auto" and not r["degraded"])
    narrow = "fused_bf16x3" if opt == "bf16x3" else "fused_tf32eq" if opt == "tf32eq" else "fused_f16x2" if f16 else "fused_f32"
    wide = "fused_f16x2" if f16 else "fused_f32"
    if l == 1 and U <= 32:
        fam, ar, l_run, UF = "k_fused", narrow, 1, 32
    elif l == 2 and U <= 32:
        fam, ar, l_run, UF = "lx32", wide, 2, 32
    elif l in (1, 2) and U <= 64:
        fam, ar, l_run, UF = "lx64", wide, 2, 64
    else:
        return "none", 0, 0, None
    if not (1 <= md <= 3 and 1 <= rd <= 2):
        return "none", 0, 0, None
    if (md != 2 or rd != 1) and ar != "fused_f16x2":
        return "none", 0, 0, None
    return fam, l_run, UF, ar


def test_decision_table(table):
    assert len(table) == 4 * 5 * 4 * 5 * 5 * 2
    for r in table:
        fam, l_run, UF, ar = _expected(r)
        assert (r["family"], r["l_run"], r["UF"]) == (fam, l_run, UF), r
        if fam != "none":
            assert r["arith"] == ar and r["exists"] == 1 and r["why"] == "", r
        else:
            assert r["why"] and r["exists"] == 0, r

    def rows(**kw):
        out = [r for r in table if all(r[k] == v for k, v in kw.items())]
        assert out
        return out

    base = dict(md=2, rd=1, opt="auto", degraded=0)
    assert {r["family"] for r in rows(l_max=1, U=32, **base)} == {"k_fused"}
    assert {r["family"] for r in rows(l_max=1, U=16, **base)} == {"k_fused"}
    for U in (33, 64):
        for l in (1, 2):
            assert {(r["family"], r["l_run"], r["UF"]) for r in rows(l_max=l, U=U, **base)} == {("lx64", 2, 64)}
    assert {r["family"] for r in rows(l_max=2, U=32, **base)} == {"lx32"}
    assert {r["family"] for r in rows(U=65)} == {"none"}
    assert {r["family"] for r in rows(l_max=0)} == {"none"} and {r["family"] for r in rows(l_max=3)} == {"none"}
    # read-out depth 2: f16x2 only, with the reason that says so; a model on f32 by its options or by a degraded auto
    for l, U in ((1, 32), (2, 32), (2, 64), (1, 64)):
        for kw in (dict(opt="f32", degraded=0), dict(opt="auto", degraded=1), dict(opt="bf16x3", degraded=0)):
            for r in rows(l_max=l, U=U, rd=2, md=2, **kw):
                assert r["family"] == "none" and "read-out depth 2 runs on the f16x2 arithmetic" in r["why"], r
        for md in (1, 2, 3):
            for opt in ("auto", "f16x2"):
                assert {r["family"] for r in rows(l_max=l, U=U, rd=2, md=md, opt=opt, degraded=0)} <= {"k_fused", "lx32", "lx64"}
    for rd in (0, 3):
        for r in rows(rd=rd, l_max=1, U=32) + rows(rd=rd, l_max=2, U=64):
            assert r["family"] == "none" and "read-out depth 1..2" in r["why"], r
    # the refusal texts of MLP depth 1 / 3 are the ones the GPU tests match
    for r in rows(l_max=2, U=64, md=3, rd=1, opt="f32", degraded=0):
        assert "MLP depth 1 / 3 runs on the f16x2 arithmetic only on the wide fused kernels" in r["why"]
    for r in rows(l_max=1, U=32, md=3, rd=1, opt="f32", degraded=0):
        assert "MLP depth 1 / 3 runs on the f16x2 arithmetic with the tabulated two-body embedding only" in r["why"]
