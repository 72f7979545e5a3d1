"""GPU tests of l_max = 1 models with 33..64 tensor features on k_fused_lx2 (csrc/fused_shapes.h: family lx64; csrc/model_io.cpp: lift_host_model).  k_fused holds 32
channels; the wave-pair kernel holds 64 and evaluates l = 0..2, and an l_max = 1 model is an l_max = 2 model whose l = 2 weights are zero, so the host lifts and zero-pads
the model and the kernel's device code is what it was.

Geometries and error bars: tests/fused_shape_cases.py (those of tests/test_gpu_fused_lx_depth.py; the instance measured beside each case is the l_max = 2, 64-feature
model of the same layer count on the same geometry).  Every figure is printed before it is asserted.  Measured on the MI355X (max|dF|, eV/A): U 33 / 48 / 64 x 1..3 layers on Cu2AgO4
4.3e-7 .. 1.3e-6 (layer-at-a-time float32 1.2e-6 .. 4.4e-6, the l_max = 2 twins 5.3e-7 .. 1.0e-6); 256-atom box 1.4e-6; float32 instance 9.7e-7."""
import numpy as np
import pytest

import atomic_virial_ref as av
import fused_shape_cases as fsc
import parity_cases as pc
import util
from pair_allegro_amd import lmp_like, model_file

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("U", [33, 48, 64])
@pytest.mark.parametrize("nl", [1, 2, 3])
def test_lmax1_wide_channels_ragged_tiles(hip_lib, model_dir, nl, U):
    """l_max = 1 with 33 / 48 / 64 tensor features, 1..3 layers, Cu2AgO4: fused_f16x2 by default, within the bars."""
    c = fsc.model(model_dir, "Cu2AgO4", "l1", num_layers=nl, num_tensor_features=U)
    twin = fsc.model(model_dir, "Cu2AgO4", "k_fused_lx2", num_layers=nl)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 l_max 1 U {U} {nl} layers")


def test_32_channels_stay_on_k_fused(hip_lib, model_dir):
    """U = 32 keeps k_fused and its packing, U = 33 takes the wide kernel's: 27 centres of 6 edges each fill a 64-slot tile as far as the kernel allows -- 6 centres per
    tile on k_fused (5 tiles), 4 on the wide kernels (7 tiles)."""
    for U, centres in ((32, 6), (33, 4)):
        c = fsc.model(model_dir, "sc27", "l1", num_tensor_features=U)
        pair, rs, f, e, pe = fsc.one_evaluation(hip_lib, c)
        try:
            assert pair.model.last_path == "fused_f16x2"
            assert pair.model.last_max_degree == 6
            used, total = pair.model.tile_occupancy()
        finally:
            pair.model.close()
        print(f"sc27 U {U}: {used} edges in {total // 64} tiles")
        assert used == 27 * 6 and total == 64 * -(-27 // centres), (U, used, total)
        forces = np.zeros((27, 3))
        np.add.at(forces, rs.tag - 1, f)
        assert np.abs(forces - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF


def test_lmax1_64_channels_full_tiles(hip_lib, model_dir):
    """The 256-atom box (degree 42: both waves of every pair carry edges), U = 64, 3 layers."""
    c = fsc.model(model_dir, "CuPd256", "l1", num_layers=3, num_tensor_features=64)
    twin = fsc.model(model_dir, "CuPd256", "k_fused_lx2", num_layers=3)
    fsc.assert_bars(hip_lib, c, twin, "CuPd256 l_max 1 U 64 3 layers")
    assert c["fused"]["info"]["max_degree"] > 32


def test_lmax1_48_channels_float32_instance(hip_lib, model_dir):
    """An MLP-depth-2, read-out-depth-1 model has the float32 instance of k_fused_lx2 as every model of that kernel does: fused_arith=f32 gives fused_f32."""
    c = fsc.measure(hip_lib, fsc.model(model_dir, "Cu2AgO4", "l1", num_layers=2, num_tensor_features=48))
    res = fsc.run(hip_lib, c, {"fused_arith": "f32"})
    err = float(np.abs(res["forces"] - c["ref"]["forces"]).max())
    print(f"l_max 1 U 48 fused_arith=f32: max|dF| vs f64 oracle {err:.3e}, layer-at-a-time f32 {c['egen']:.3e}")
    assert res["info"]["path"] == "fused_f32", res["info"]
    util.assert_close_to(res, c["ref"], 5e-4, what="l_max 1 U 48 fused_f32")
    assert err < pc.NORTH_STAR_DF and err < max(3.0 * c["egen"], 1e-5)


def test_lmax1_64_channels_dense_list_goes_layer_at_a_time(hip_lib, model_dir):
    """fcc Cu at r_max 6.1: every centre has 78 edges, above the wide kernels' 64-slot tile, so the whole list goes to the layer-at-a-time kernels (k_fused, which has
    8-wave tiles for such a list, does not hold 64 channels); path=fused is a clean error."""
    c = fsc.model(model_dir, "Cu108", "l1", num_tensor_features=64)
    res = fsc.run(hip_lib, c)
    assert res["info"]["path"] == "generic_f32" and res["info"]["max_degree"] > 64, res["info"]
    util.assert_close_to(res, c["ref"], 5e-4, what="l_max 1 U 64, 78 neighbours")
    assert np.abs(res["forces"] - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF
    with pytest.raises(Exception, match="fused path unavailable.*per tile of the wide fused kernel"):
        fsc.run(hip_lib, c, {"path": "fused"})


AV_NAMES = ["Ag", "Cu", "O"]


def test_lmax1_48_channels_with_readout_depth_2_and_mlp_depth_3(hip_lib, model_dir):
    """Both new shapes together: U = 48, read-out depth 2, MLP depth 3 -- and the per-atom virial of that instance (bars of test_gpu_atomic_virial.py)."""
    over = dict(num_layers=2, num_tensor_features=48, readout_depth=2, mlp_depth=3)
    c = fsc.model(model_dir, "Cu2AgO4", "l1", **over)
    twin = fsc.model(model_dir, "Cu2AgO4", "k_fused_lx2", num_layers=2)
    fsc.assert_bars(hip_lib, c, twin, "Cu2AgO4 l_max 1 U 48 read-out depth 2 MLP depth 3")
    g = util.load_golden("Cu2AgO4_r5")
    cfg = model_file.model_S(type_names=AV_NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), **over)
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/l1w_av.ahip"
    model_file.save_ahip(path, cfg, w)
    types = np.array([AV_NAMES.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    rs = av.rank_system(cfg, g["cell"], g["pos"], types)
    ref = av.oracle_w(cfg, w, rs, AV_NAMES)
    res = av.run(hip_lib, path, rs, AV_NAMES, options={"path": "fused", "fused_arith": "f16x2"})
    assert res["path"] == "fused_f16x2"
    scale = np.abs(ref).max()
    err = np.abs(res["W"] - ref).max()
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    dv = np.abs(av.sym_sum(res["W"]) - res["virial"]).max()
    print(f"atomic_virial l_max 1 U 48 RD 2 MD 3: max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)


def test_lmax1_64_channels_translation_and_rotation(hip_lib, model_dir):
    """The 256-atom box of test_lmax1_64_channels_full_tiles translated, and rotated rigidly by a quarter turn about z (which maps the cubic cell onto itself): energies
    invariant to 1e-6 relative, forces rotated within 5e-5 -- the criteria of test_gpu_fused.py: test_full_size_properties_10k.  The lifted model's l = 2 components are
    zero for every orientation, not only the one the oracle comparison saw."""
    c = fsc.measure(hip_lib, fsc.model(model_dir, "CuPd256", "l1", num_layers=3, num_tensor_features=64))
    a = c["fused"]
    cell, pos = np.asarray(c["cell"], dtype=float), np.asarray(c["pos"], dtype=float)
    assert np.allclose(cell, np.eye(3) * cell[0, 0])
    shifted = lmp_like.wrap(cell, pos + np.array([1.234, -0.77, 3.1]))
    b = util.run_pair(hip_lib, c["path"], cell, shifted, c["types"], c["names"])
    assert b["info"]["path"] == "fused_f16x2"
    np.testing.assert_allclose(b["pe"], a["pe"], rtol=1e-6)
    assert np.abs(b["forces"] - a["forces"]).max() < 5e-5
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rotated = lmp_like.wrap(cell, pos @ R.T)
    r = util.run_pair(hip_lib, c["path"], cell, rotated, c["types"], c["names"])
    assert r["info"]["path"] == "fused_f16x2"
    np.testing.assert_allclose(r["pe"], a["pe"], rtol=1e-6)
    np.testing.assert_allclose(r["eatom"], a["eatom"], rtol=1e-6, atol=1e-6 * np.abs(a["eatom"]).max())
    print(f"rotated box: max|F' - R F| {np.abs(r['forces'] - a['forces'] @ R.T).max():.3e}, translated: {np.abs(b['forces'] - a['forces']).max():.3e}")
    assert np.abs(r["forces"] - a["forces"] @ R.T).max() < 5e-5
