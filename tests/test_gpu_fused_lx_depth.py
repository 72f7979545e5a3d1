"""GPU tests of the latent-MLP-depth instances of the wide fused kernels (template parameter MD of k_fused_lx / k_fused_lx2, csrc/fused_lx.hip, csrc/fused_lx2.hip):
`allegro_mlp_hidden_layers_depth` 1 and 3 on l_max = 2 models (2 in /root/reference/tests/test_data/test_repro_allegro.yaml:94), f16x2 arithmetic only.

Geometries: the 7-atom triclinic Cu2AgO4 golden (3 types, ragged degrees, several centres per tile) and the 256-atom CuPd box relabelled O/H (degrees above 32: every
wave of k_fused_lx and both waves of every pair of k_fused_lx2 carry edges).  The float64 oracle runs once per model and is shared by the tests of this file.

Error bars of the force error against the float64 oracle (`_assert_bars`): below parity_cases.NORTH_STAR_DF, and below max(3 e_generic, 1e-5) with e_generic the error of
the layer-at-a-time float32 kernels on the same file -- the bar test_gpu_fused.py: test_fused_latent_mlp_depth_1_and_3 uses for k_fused.  Nobody had measured that
second bar on the wide kernels, so every case also measures the depth-2 instance of the same kernel (same widths, layer count and geometry): where that existing instance
itself exceeds max(3 e_generic, 1e-5), the bar for the new depth is twice the depth-2 instance's measured error instead.  Every figure is printed before it is asserted.
Measured on the MI355X (max|dF|, eV/A): the depth-2 instances 5.3e-7 .. 1.2e-6 on the eight (geometry, width, layers) shapes below, i.e. always inside max(3 e_generic, 1e-5), so
the fall-back bar is not in use; depth 1 5.8e-7 .. 2.2e-6, depth 3 3.7e-7 .. 1.8e-6, the layer-at-a-time float32 kernels 1.1e-6 .. 6.7e-6."""
import numpy as np
import pytest

import atomic_virial_ref as av
import parity_cases as pc
import util
from oracle import allegro_torch
from pair_allegro_amd import model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

pytestmark = pytest.mark.gpu

_geoms = {}
_runs = {}          # (geometry, frozen model overrides) -> the file, the float64 oracle, the default (fused) run and the layer-at-a-time run


def _geometry(tag):
    """cell, positions, symbols, model type names, average neighbour count at r_max = 5."""
    if tag not in _geoms:
        if tag == "Cu2AgO4":
            g = util.load_golden("Cu2AgO4_r5")
            _geoms[tag] = (g["cell"], g["pos"], g["symbols"], ["Cu", "Ag", "O"], float(g["nedges"]) / len(g["pos"]))
        else:
            g = util.load_golden("CuPd-cubic-big_r5")
            symbols = ["O" if s == "Cu" else "H" for s in g["symbols"]]
            nb = float(len(util.glue.brute_force_edges(g["cell"], g["pos"], 5.0)[0])) / len(g["pos"])
            _geoms[tag] = (g["cell"], g["pos"], symbols, ["O", "H"], nb)
    return _geoms[tag]


def _case(model_dir, name, cfg, cell, pos, symbols):
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/{name}.nequip.pth"
    allegro_torch.export_nequip_pth(path, cfg, w)
    names = sorted(set(symbols))
    types = np.array([names.index(s) + 1 for s in symbols], dtype=np.int32)
    ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, names)
    return path, types, names, ref


def _model(model_dir, tag, **over):
    """The model file of model_L(**over) on geometry `tag` and its float64 oracle result, built once."""
    key = (tag, tuple(sorted(over.items())))
    if key not in _runs:
        cell, pos, symbols, tn, nb = _geometry(tag)
        cfg = model_file.model_L(type_names=tn, avg_num_neighbors=nb, **over)
        name = "lxd_" + tag + "_" + "_".join(f"{k}{v}" for k, v in sorted(over.items()))
        path, types, names, ref = _case(model_dir, name, cfg, cell, pos, symbols)
        _runs[key] = dict(cfg=cfg, path=path, types=types, names=names, ref=ref, cell=cell, pos=pos)
    return _runs[key]


def _measure(hip_lib, model_dir, tag, **over):
    """Default options (the fused kernel) and path=generic on the same file, both against the float64 oracle; once per model."""
    c = _model(model_dir, tag, **over)
    if "fused" not in c:
        c["fused"] = util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"])
        c["generic"] = util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"], options={"path": "generic"})
        c["err"] = float(np.abs(c["fused"]["forces"] - c["ref"]["forces"]).max())
        c["egen"] = float(np.abs(c["generic"]["forces"] - c["ref"]["forces"]).max())
    return c


def _assert_bars(hip_lib, model_dir, tag, depth, **over):
    """The module docstring's bars for the depth-`depth` model; the depth-2 model of the same shape is measured beside it."""
    c = _measure(hip_lib, model_dir, tag, mlp_depth=depth, **over)
    d2 = _measure(hip_lib, model_dir, tag, mlp_depth=2, **over)
    what = f"{tag} {over} depth {depth}"
    print(f"{what}: max|dF| vs f64 oracle fused {c['err']:.3e}, layer-at-a-time f32 {c['egen']:.3e}; depth 2: fused {d2['err']:.3e}, layer-at-a-time f32 {d2['egen']:.3e}")
    assert c["fused"]["info"]["path"] == "fused_f16x2", c["fused"]["info"]
    assert c["generic"]["info"]["path"] == "generic_f32" and d2["fused"]["info"]["path"] == "fused_f16x2"
    util.assert_close_to(c["fused"], c["ref"], 5e-4, what=what)
    assert c["err"] < pc.NORTH_STAR_DF
    bar = max(3.0 * c["egen"], 1e-5)
    if d2["err"] >= max(3.0 * d2["egen"], 1e-5):          # the existing depth-2 instance misses that bar itself: twice its measured error instead
        bar = 2.0 * d2["err"]
    assert c["err"] < bar, (what, c["err"], bar)
    return c


@pytest.mark.parametrize("U", [32, 64])
@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("depth", [1, 3])
def test_every_depth_instance_ragged_tiles(hip_lib, model_dir, depth, nl, U):
    """Every new instance (depth 1 / 3 x 1..3 layers x both kernels) on Cu2AgO4: fused_f16x2 by default, within the bars of the module docstring.
    Measured on the MI355X (max|dF| in eV/A against the float64 oracle): see DESIGN 4.3, "Latent MLP depth 1 / 3 on the wide kernels"."""
    _assert_bars(hip_lib, model_dir, "Cu2AgO4", depth, num_layers=nl, num_tensor_features=U)


@pytest.mark.parametrize("U", [32, 64])
@pytest.mark.parametrize("depth", [1, 3])
def test_every_depth_instance_full_tiles(hip_lib, model_dir, depth, U):
    """Three layers on the 256-atom box: degrees above 32, so all four waves of k_fused_lx and both waves of every pair of k_fused_lx2 work on real edges."""
    c = _assert_bars(hip_lib, model_dir, "CuPd256", depth, num_layers=3, num_tensor_features=U)
    assert c["fused"]["info"]["max_degree"] > 32


def test_depth_3_without_f16x2_is_refused_or_falls_back(hip_lib, model_dir, monkeypatch):
    """Depth 1 / 3 exists on the f16x2 arithmetic only: fused_arith=f32 sends the model to the layer-at-a-time float32 kernels, path=fused then fails with the gate's
    reason; fused_arith=auto with its first-evaluation self-check on (whose float32 pass runs on the layer-at-a-time kernels) ends on f16x2 and says so."""
    monkeypatch.delenv("AHIP_NO_ARITH_SELFCHECK", raising=False)
    for U in (32, 64):
        c = _model(model_dir, "Cu2AgO4", mlp_depth=3, num_layers=3, num_tensor_features=U)
        args = (hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"])
        exact = util.run_pair(*args, options={"fused_arith": "f32"})
        assert exact["info"]["path"] == "generic_f32"
        util.assert_close_to(exact, c["ref"], 5e-4, what="depth 3, fused_arith=f32")
        with pytest.raises(Exception, match="fused path unavailable.*MLP depth 1 / 3 runs on the f16x2 arithmetic only on the wide fused kernels"):
            util.run_pair(*args, options={"path": "fused", "fused_arith": "f32"})
        auto = util.run_pair(*args, options={"fused_arith": "auto"})
        assert auto["info"]["path"] == "fused_f16x2"
        assert "f16x2 kept" in auto["info"]["arith_note"], auto["info"]["arith_note"]
        util.assert_close_to(auto, c["ref"], 5e-4, what="depth 3, fused_arith=auto")


def test_depth_3_narrow_model_zero_padded(hip_lib, model_dir):
    """A narrower l_max = 2 model (U 16, S 48, MLP width 40, read-out 24) with depth 3 runs on k_fused_lx zero-padded, like its depth-2 twin
    (test_gpu_fused_lx.py: test_narrower_l2_models_run_on_the_wide_kernels_zero_padded)."""
    _assert_bars(hip_lib, model_dir, "Cu2AgO4", 3, num_tensor_features=16, num_scalar_features=48, mlp_width=40, readout_width=24)


AV_NAMES = ["Ag", "Cu", "O"]


@pytest.mark.parametrize("U", [32, 64])
@pytest.mark.parametrize("depth", [1, 3])
def test_depth_instances_atomic_virial(hip_lib, model_dir, depth, U):
    """The VAR_VA twins of the new instances: output atomic_virial against the float64 oracle's W, bars of test_gpu_atomic_virial.py (2e-5 of max|W|; the symmetrised
    sum of W against the virial at 1e-6 of the row scale)."""
    g = util.load_golden("Cu2AgO4_r5")
    cfg = model_file.model_L(type_names=AV_NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), num_tensor_features=U, mlp_depth=depth)
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/lxd_av_U{U}_md{depth}.ahip"
    model_file.save_ahip(path, cfg, w)
    types = np.array([AV_NAMES.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    rs = av.rank_system(cfg, g["cell"], g["pos"], types)
    ref = av.oracle_w(cfg, w, rs, AV_NAMES)
    res = av.run(hip_lib, path, rs, AV_NAMES, options={"path": "fused", "fused_arith": "f16x2"})
    assert res["path"] == "fused_f16x2"
    assert res["W"].shape == ref.shape
    scale = np.abs(ref).max()
    err = np.abs(res["W"] - ref).max()
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    dv = np.abs(av.sym_sum(res["W"]) - res["virial"]).max()
    print(f"atomic_virial depth {depth} U {U}: max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)


LAUNCHES = 20


@pytest.mark.parametrize("U", [32, 64])
@pytest.mark.parametrize("depth", [1, 3])
def test_depth_instances_repeat_themselves(hip_lib, model_dir, depth, U):
    """The stores of the extra saved rows and the extra pair hand-overs: 20 evaluations of one model object on the 256-atom box (3 layers) -- per-atom energies bit for bit
    those of the first evaluation (their summation order is fixed), forces within 1e-9 of max|F| (float64 atomics in arrival order): the criterion of test_gpu_soak.py.
    20 launches, not 100: the box is small and the test stays within seconds."""
    c = _model(model_dir, "CuPd256", mlp_depth=depth, num_layers=3, num_tensor_features=U)
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"]] + list(c["names"]), ntypes=len(c["names"]))
    pair.init_style()
    rs = util.lmp_like.build_rank_system(c["cell"], c["pos"], c["types"], pair.init_one(1, 1) + 1.0)
    lst = list_from_rank_system(rs)
    first = None
    try:
        for it in range(LAUNCHES):
            atom = atom_from_rank_system(rs, len(c["names"]))
            pair.compute(atom, lst)
            assert pair.model.last_path == "fused_f16x2"
            cur = (atom.f.copy(), pair.eatom[: rs.nlocal].copy(), float(pair.eng_vdwl))
            if first is None:
                first = cur
                fscale = np.abs(first[0]).max()
                continue
            worst = np.abs(cur[0] - first[0]).max() / fscale
            ndiff = int((cur[1] != first[1]).sum())
            assert worst <= 1e-9, f"launch {it}: forces differ from the first launch by {worst:.3e} (relative to max|F|)"
            assert ndiff == 0, f"launch {it}: {ndiff} per-atom energies differ from the first launch"
            assert abs(cur[2] - first[2]) <= 1e-12 * abs(first[2])
    finally:
        pair.model.close()
    # the first launch is the one the parity tests above compare with the oracle; here only that it is sane
    forces = np.zeros((len(c["pos"]), 3))
    np.add.at(forces, rs.tag - 1, first[0])
    assert np.abs(forces - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF
