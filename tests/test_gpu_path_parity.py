"""Path-difference parity on the MI355X (tests/path_parity.py): every tensor-product path of every layer, on every fused kernel and
arithmetic, and on the layer-at-a-time kernels; per-edge gradients of k_fused; degenerate per-type energy scales on the f16x2 arithmetic."""
import ctypes as C

import numpy as np
import pytest

import path_parity as pp
import util
from pair_allegro_amd import lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

pytestmark = pytest.mark.gpu

ARITHS = ("f32", "f16x2", "bf16x3")
WIDE_ARITHS = ("f32", "f16x2")                   # k_fused_lx / k_fused_lx2 have no bf16 instances (fused_arith=bf16x3 runs fused_f32 there)
_cases = {}


def _cu2ago4(model_dir, name, **over):
    """Cu2AgO4: 3 types, triclinic, ragged degrees, several centres per tile."""
    if name not in _cases:
        g = util.load_golden("Cu2AgO4_r5")
        cfg = dict(over, type_names=["Ag", "Cu", "O"], avg_num_neighbors=float(g["nedges"]) / len(g["pos"]))
        cfg = model_file.model_L(**cfg) if cfg.get("l_max", 1) == 2 else model_file.model_S(**cfg)
        _cases[name] = pp.PathCase(model_dir, name, cfg, g["cell"], g["pos"], g["symbols"])
    return _cases[name]


def _cupd_oh(model_dir, name, **over):
    """The 256-atom CuPd box relabelled O/H (test_model_L_layers_and_widths): degrees above 32, i.e. the multi-wave / wave-pair splits."""
    if name not in _cases:
        g = util.load_golden("CuPd-cubic-big_r5")
        symbols = ["O" if s == "Cu" else "H" for s in g["symbols"]]
        nb = float(len(util.glue.brute_force_edges(g["cell"], g["pos"], 5.0)[0])) / len(g["pos"])
        cfg = dict(over, type_names=["H", "O"], avg_num_neighbors=nb)
        cfg = model_file.model_L(**cfg) if cfg.get("l_max", 1) == 2 else model_file.model_S(**cfg)
        _cases[name] = pp.PathCase(model_dir, name, cfg, g["cell"], g["pos"], symbols)
    return _cases[name]


# kernel -> (model overrides); k_fused: model S (l_max 1); k_fused_lx: U = 32; k_fused_lx2: U = 64 (l_max 2, 3 layers)
KERNELS = {
    "k_fused_nl2": dict(num_layers=2),
    "k_fused_nl3": dict(num_layers=3),
    "k_fused_lx": dict(l_max=2, num_tensor_features=32),
    "k_fused_lx2": dict(l_max=2, num_tensor_features=64),
}


def _run_paths(lib, case, selection, arith):
    worst = 0.0
    for k, p, lll in selection:
        worst = max(worst, case.check(lib, k, p, "float32", f"fused_{arith}", options={"path": "fused", "fused_arith": arith}))
    return worst


def _instances(kernels):
    return [(k, a) for k in kernels for a in (ARITHS if k.startswith("k_fused_nl") else WIDE_ARITHS)]


@pytest.mark.parametrize("kernel,arith", _instances(KERNELS))
def test_every_path_on_the_fused_kernels(hip_lib, model_dir, kernel, arith):
    case = _cu2ago4(model_dir, f"paths_{kernel}", **KERNELS[kernel])
    worst = _run_paths(hip_lib, case, pp.paths(case.cfg), arith)
    print(f"\n{kernel} {arith} Cu2AgO4 all {len(pp.paths(case.cfg))} paths: worst error / bar {worst:.3f}")


def _one_path_per_l3_and_the_last_layer(cfg):
    every = pp.paths(cfg)
    first = [next(e for e in every if e[0] == 1 and e[2][2] == l3) for l3 in range(cfg["l_max"] + 1)]
    return first + [e for e in every if e[0] == cfg["num_layers"]][-1:]


@pytest.mark.parametrize("kernel,arith", _instances(["k_fused_nl2", "k_fused_lx", "k_fused_lx2"]))
def test_paths_with_degrees_above_32(hip_lib, model_dir, kernel, arith):
    case = _cupd_oh(model_dir, f"paths_big_{kernel}", **KERNELS[kernel])
    worst = _run_paths(hip_lib, case, _one_path_per_l3_and_the_last_layer(case.cfg), arith)
    print(f"\n{kernel} {arith} CuPd-256 O/H: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_every_path_on_the_layer_kernels_l_max_3(hip_lib, model_dir, dtype):
    """l_max = 3, 2 layers (34 + 4 paths), widths off every fused shape (S 48, U 16, MLP 40, read-out 24): the layer-at-a-time kernels."""
    if "l3" not in _cases:
        g = util.load_golden("Cu2AgO4_r5")
        cfg = dict(model_file.DEFAULT_CFG, type_names=["Ag", "Cu", "O"], l_max=3, num_layers=2, num_scalar_features=48, num_tensor_features=16,
                   mlp_width=40, readout_width=24, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]))
        _cases["l3"] = pp.PathCase(model_dir, "paths_l3", cfg, g["cell"], g["pos"], g["symbols"])
    case = _cases["l3"]
    worst = 0.0
    for k, p, lll in pp.paths(case.cfg):
        worst = max(worst, case.check(hip_lib, k, p, dtype, "generic_f32" if dtype == "float32" else "generic_f64", options={"path": "generic"}))
    print(f"\nlayer kernels l_max 3 {dtype}: worst error / bar {worst:.3f}")


def test_every_path_on_the_layer_kernels_odd_widths_l_max_2(hip_lib, model_dir):
    """l_max = 2, 2 layers, S 30 / U 6 / MLP 37 / read-out 10: no width is a multiple of 4, so the GEMM takes its scalar-load instances and the sub-block views
    V + lm U are not 16-byte aligned; the unrolled tensor product and the row reductions run with an odd U.  Per path, not only in the sum."""
    if "odd_l2" not in _cases:
        g = util.load_golden("Cu2AgO4_r5")
        cfg = dict(model_file.DEFAULT_CFG, type_names=["Ag", "Cu", "O"], l_max=2, num_layers=2, num_scalar_features=30, num_tensor_features=6,
                   mlp_width=37, readout_width=10, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]))
        _cases["odd_l2"] = pp.PathCase(model_dir, "paths_odd_l2", cfg, g["cell"], g["pos"], g["symbols"])
    case = _cases["odd_l2"]
    worst = 0.0
    for k, p, lll in pp.paths(case.cfg):
        worst = max(worst, case.check(hip_lib, k, p, "float32", "generic_f32", options={"path": "generic"}))
    print(f"\nlayer kernels l_max 2 odd widths: worst error / bar {worst:.3f} ({len(pp.paths(case.cfg))} paths)")


# ---- per-edge gradients of k_fused (AHIP_FUSED_DBG=1: the kernel dumps {g[3], dd, dfc, dY[3]} per edge) --------------------------------
@pytest.mark.parametrize("arith", ["f32", "f16x2"])
@pytest.mark.parametrize("tag", ["Si64_r5", "Cu2AgO4_r5"])
def test_per_edge_gradients_of_k_fused(hip_lib, model_dir, tag, arith, monkeypatch):
    """Errors of single edges can cancel in the force sum: the kernel's per-edge gradient dE/d(r_j - r_i) against the float64 oracle's
    autograd gradient, edge by edge, within 2e-5 of the largest one."""
    monkeypatch.setenv("AHIP_FUSED_DBG", "1")
    g = util.load_golden(tag)
    names = sorted(set(g["symbols"]))
    types = np.array([names.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    cfg = model_file.model_S(type_names=names, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]))
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/edge_grads_{tag}.ahip"
    model_file.save_ahip(path, cfg, w)
    rs = lmp_like.build_rank_system(g["cell"], g["pos"], types, cfg["r_max"] + 1.0)
    pair = PairAllegro(lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", path] + names, ntypes=len(names))
    pair.model.set_option("path", "fused")
    pair.model.set_option("fused_arith", arith)
    pair.init_style()
    pair.compute(atom_from_rank_system(rs, len(names)), list_from_rank_system(rs))
    assert pair.model.last_path == f"fused_{arith}"
    ei, _ = pair.model.get_edges()
    E = ei.shape[1]
    out = np.zeros((E, 8), dtype=np.float32)
    fn = hip_lib.lib.ahip_debug_fused_edges
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_longlong]
    assert fn(pair.model.h, out.ctypes.data_as(C.POINTER(C.c_float)), E) == 0
    pair.model.close()
    ref_ei, gref = pp.oracle_edge_gradients(cfg, w, rs, names)
    assert E == ref_ei.shape[1]
    order = {(int(i), int(j)): e for e, (i, j) in enumerate(ref_ei.T)}
    idx = np.array([order[(int(i), int(j))] for i, j in ei.T])
    err = np.abs(out[:, :3].astype(np.float64) - gref[idx]).max()
    scale = np.abs(gref).max()
    print(f"\n{tag} {arith}: per-edge max|g - g_ref| / max|g_ref| = {err / scale:.3e} ({E} edges)")
    assert err <= 2e-5 * scale, (err, scale)


# ---- degenerate per-type energy scales on the f16x2 arithmetic (the backward pass runs scaled by 2^-exponent of the centre type's scale) --
@pytest.mark.parametrize("scale", [0.0, -1.0, 1e-3, 1e3, 1e-39])
@pytest.mark.parametrize("kernel", ["k_fused_nl2", "k_fused_lx", "k_fused_lx2"])
def test_degenerate_species_scale_on_f16x2(hip_lib, model_dir, kernel, scale):
    """One species' energy scale 0, -1, 1e-3, 1e3 or the float32 subnormal 1e-39: explicit fused_arith=f16x2 stays fused without the range
    alarm (it raises), is finite, and matches the float64 oracle to the path-difference bar.  1e-39 gave the backward exponent -130, whose
    inverse 2^130 is inf: every edge of that species came out non-finite."""
    g = util.load_golden("Cu2AgO4_r5")
    names = ["Ag", "Cu", "O"]
    types = np.array([names.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    over = dict(KERNELS[kernel], type_names=names, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]))
    cfg = model_file.model_L(**over) if over.get("l_max", 1) == 2 else model_file.model_S(**over)
    w = model_file.init_weights(cfg)
    w["scale"] = np.array(w["scale"], dtype=np.float64)
    w["scale"][1] = scale                                              # Cu: the species with two atoms
    path = f"{model_dir}/scale_{kernel}_{scale:g}.ahip"
    model_file.save_ahip(path, cfg, w)
    ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, g["cell"], g["pos"], types, names)
    res = util.run_pair(hip_lib, path, g["cell"], g["pos"], types, names, options={"path": "fused", "fused_arith": "f16x2"})
    assert res["info"]["path"] == "fused_f16x2", res["info"]
    worst = 0.0
    for q in pp.QUANTITIES:
        assert np.isfinite(res[q]).all(), q
        err = np.abs(res[q] - ref[q]).max()
        allowed = pp.BAR["float32"] * np.abs(ref[q]).max() + pp.ROUNDING["float32"] * np.abs(ref[q]).max()
        worst = max(worst, err / allowed)
        assert err <= allowed, (q, err, allowed)
    print(f"\n{kernel} scale {scale:g}: worst error / bar {worst:.3f}")
