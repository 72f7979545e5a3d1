"""GPU tests of the read-out-width-64 instances of k_fused, k_fused_lx and k_fused_lx2 (template parameter RT = 4: csrc/fused.hip, csrc/fused_lx.hip, csrc/fused_lx2.hip;
objects fused_hq.o, fused_lx_q.o and fused_lx2_q.o): a model with 33 <= `readout_mlp_hidden_layers_width` <= 64 (32 in the reference's
tests/test_data/test_repro_allegro.yaml:98) runs fused, zero-padded to read-out width 64, on the f16x2 arithmetic with MLP width <= 64 and read-out depth 1.  Before these
instances existed such a model ran on the layer-at-a-time float32 kernels (`generic_f32`).

Geometries and bars are those of tests/fused_shape_cases.py: the 7-atom triclinic Cu2AgO4 golden (3 types, degrees 36..39: ragged tiles), the 256-atom CuPd box relabelled
O / H (degree 42: every wave carries edges), the same box doubled along x, the 108-atom jittered fcc Cu box at r_max 6.1 (78 neighbours: the 8-wave tile of k_fused).  The
float64 oracle runs once per model and is shared.  `twin` is the readout_width = 32 model of the same kernel, depths, layers and geometry, so the bars come from the project
(fused_shape_cases.assert_bars): max|dF| against the float64 oracle below parity_cases.NORTH_STAR_DF and below max(3 e_generic, 1e-5), e_generic being the error of the
layer-at-a-time float32 kernels on the same file -- or twice the twin's error where the twin itself misses that bar; energies and virial util.assert_close_to(.., 5e-4).
Every figure is printed before it is asserted.
Measured on the MI355X (max|dF|, eV/A): the 27 width-64 instances on Cu2AgO4 3.0e-7 .. 1.3e-6, their width-32 twins 3.4e-7 .. 1.9e-6 (always inside max(3 e_generic, 1e-5),
so the fall-back bar is not in use), the layer-at-a-time float32 kernels 6.5e-7 .. 4.5e-6; widths 33 / 40 / 48 3.5e-7 .. 9.6e-7; the narrow model at width 50 1.0e-6
(k_fused) / 3.6e-7 (k_fused_lx); 256-atom box 1.2e-6 (k_fused) / 1.3e-6 (k_fused_lx) / 2.0e-6 (k_fused_lx2); the 8-wave tile of k_fused 1.2e-6; more tiles than
workgroups: no per-atom energy differs, max|dF| between the two grids 0, against the oracle 1.3e-6 .. 2.0e-6; atomic_virial max|dW| 4.9e-7 .. 6.8e-7 of max|W| 0.8 .. 1.7."""
import numpy as np
import pytest
import torch

import atomic_virial_ref as av
import fused_shape_cases as fsc
import parity_cases as pc
import util
from pair_allegro_amd import model_file

pytestmark = pytest.mark.gpu

KERNELS = ["k_fused", "k_fused_lx", "k_fused_lx2"]


def _pair(model_dir, tag, kernel, width=64, **over):
    """The model of read-out width `width` and its readout_width = 32 twin (same kernel, other widths, depths, layers, geometry)."""
    over.setdefault("readout_depth", 1)
    return fsc.model(model_dir, tag, kernel, **dict(over, readout_width=width)), fsc.model(model_dir, tag, kernel, **dict(over, readout_width=32))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("md", [1, 2, 3])
def test_every_readout_width_64_instance_ragged_tiles(hip_lib, model_dir, md, nl, kernel):
    """Every compiled width-64 instance (3 kernels x 1..3 layers x latent MLP depth 1..3) on Cu2AgO4: fused_f16x2 under default options, within the bars."""
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, num_layers=nl, mlp_depth=md)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} {nl} layers MLP depth {md} read-out width 64")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("width", [33, 40, 48])
def test_padding_inside_the_new_width(hip_lib, model_dir, kernel, width):
    """Widths that do not fill the 4 read-out tiles: 33 (one feature in the third tile), 40 (a half-filled tile), 48 (the fourth tile all padding)."""
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, width=width, num_layers=2)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} read-out width {width}")


@pytest.mark.parametrize("kernel,U", [("k_fused", 16), ("k_fused_lx", 16), ("k_fused_lx2", 16), ("k_fused_lx2", 40)])
def test_narrow_model_with_readout_width_50(hip_lib, model_dir, kernel, U):
    """S 48, U 16, MLP width 40 with read-out width 50: every width padded at once, the read-out to 64.  (With 16 tensor features an l_max = 2 model is k_fused_lx's
    whatever its base configuration; U = 40 is the narrow model that k_fused_lx2 pads, to 64 tensor features.)"""
    over = dict(fsc.NARROW, num_tensor_features=U)
    over.pop("readout_width")
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, width=50, **over)
    assert c["cfg"]["readout_width"] == 50 and twin["cfg"]["readout_width"] == 32 and c["cfg"]["num_scalar_features"] == 48 and c["cfg"]["mlp_width"] == 40
    assert c["cfg"]["num_tensor_features"] == U
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} narrow model (U = {U}), read-out width 50")


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_width_64_full_tiles(hip_lib, model_dir, kernel):
    """Three layers on the 256-atom box: degree 42, so every wave of a tile works on real edges."""
    c, twin = _pair(model_dir, "CuPd256", kernel, num_layers=3)
    fsc.assert_bars(hip_lib, c, twin, f"CuPd256 {kernel} read-out width 64")
    assert c["fused"]["info"]["max_degree"] > 32


def test_readout_width_64_eight_wave_tile_of_k_fused(hip_lib, model_dir):
    """fcc Cu at r_max 6.1: 78 neighbours per atom, more than a 64-slot tile, so the 8-wave / 128-slot instances of k_fused run."""
    c, twin = _pair(model_dir, "Cu108", "k_fused")
    fsc.assert_bars(hip_lib, c, twin, "Cu108 k_fused (8-wave tiles) read-out width 64")
    assert 64 < c["fused"]["info"]["max_degree"] <= 128


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_width_64_more_tiles_than_workgroups(hip_lib, model_dir, kernel):
    """One workgroup consumes the (changed-length) weight stream more than once and prefetches across the tile boundary: reserve_wgs=128 leaves CUs - 64 workgroups for
    the 256 tiles of the 256-atom box on the wide kernels, 2 CUs - 128 for the 512 tiles of the doubled box on k_fused.  Against reserve_wgs=0 on the same model: per-atom
    energies bit for bit, forces within 1e-9 of max|F| (float64 atomics in arrival order) -- the criterion of test_gpu_soak.py."""
    tag = "CuPd512" if kernel == "k_fused" else "CuPd256"
    c = fsc.model(model_dir, tag, kernel, readout_width=64, readout_depth=1, num_layers=3)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    grid = 2 * ncu - 128 if kernel == "k_fused" else ncu - 64
    pair, rs, f1, e1, pe1 = fsc.one_evaluation(hip_lib, c, {"reserve_wgs": "128"})
    try:
        assert pair.model.last_path == "fused_f16x2"
        used, total = pair.model.tile_occupancy()
        tiles = total // 64
        print(f"{kernel} on {tag}: {tiles} tiles ({used} edges) on {grid} workgroups of {ncu} CUs")
        assert total % 64 == 0 and tiles > grid > 0, (tiles, grid)
    finally:
        pair.model.close()
    pair, _, f0, e0, pe0 = fsc.one_evaluation(hip_lib, c, {"reserve_wgs": "0"}, rs=rs)
    try:
        assert pair.model.last_path == "fused_f16x2"
    finally:
        pair.model.close()
    print(f"{kernel} on {tag}: per-atom energies that differ {int((e1 != e0).sum())}, max|dF| {np.abs(f1 - f0).max():.3e} (max|F| {np.abs(f0).max():.3e})")
    assert int((e1 != e0).sum()) == 0
    assert np.abs(f1 - f0).max() <= 1e-9 * np.abs(f0).max()
    assert abs(pe1 - pe0) <= 1e-12 * abs(pe0)
    forces = np.zeros((len(c["pos"]), 3))
    np.add.at(forces, rs.tag - 1, f1)
    err = np.abs(forces - c["ref"]["forces"]).max()
    print(f"{kernel} on {tag}: max|dF| vs f64 oracle {err:.3e}")
    assert err < pc.NORTH_STAR_DF


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_width_64_without_f16x2_is_refused_or_falls_back(hip_lib, model_dir, monkeypatch, kernel):
    """Width 64 exists on the f16x2 arithmetic only (k_fused: with the tabulated two-body embedding): fused_arith=f32 sends the model to the layer-at-a-time float32
    kernels, path=fused then fails with the gate's reason; fused_arith=auto with its first-evaluation self-check on (whose float32 pass runs on the layer-at-a-time
    kernels) ends on f16x2 and says so."""
    monkeypatch.delenv("AHIP_NO_ARITH_SELFCHECK", raising=False)
    c = fsc.model(model_dir, "Cu2AgO4", kernel, readout_width=64, readout_depth=1, num_layers=3)
    exact = fsc.run(hip_lib, c, {"fused_arith": "f32"})
    print(f"{kernel} read-out width 64, fused_arith=f32: {exact['info']['path']}")
    assert exact["info"]["path"] == "generic_f32"
    util.assert_close_to(exact, c["ref"], 5e-4, what="read-out width 64, fused_arith=f32")
    with pytest.raises(Exception, match="fused path unavailable.*read-out width 33..64 runs on the f16x2 arithmetic"):
        fsc.run(hip_lib, c, {"path": "fused", "fused_arith": "f32"})
    if kernel == "k_fused":
        with pytest.raises(Exception, match="fused path unavailable.*read-out width 33..64 runs on the f16x2 arithmetic with the tabulated two-body embedding only"):
            fsc.run(hip_lib, c, {"path": "fused", "fused_tb": "mlp"})
        mlp = fsc.run(hip_lib, c, {"fused_tb": "mlp"})
        assert mlp["info"]["path"] == "generic_f32"
        util.assert_close_to(mlp, c["ref"], 5e-4, what="read-out width 64, fused_tb=mlp")
    auto = fsc.run(hip_lib, c, {"fused_arith": "auto"})
    print(f"{kernel} read-out width 64, fused_arith=auto: {auto['info']['path']}, note: {auto['info']['arith_note']}")
    assert auto["info"]["path"] == "fused_f16x2"
    assert "f16x2 kept" in auto["info"]["arith_note"], auto["info"]["arith_note"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="read-out width 64, fused_arith=auto")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("what,over,reason", [
    ("read-out width 65", dict(readout_width=65, readout_depth=1), "read-out width 64"),
    ("read-out depth 2", dict(readout_width=64, readout_depth=2), "read-out width 33..64 runs with read-out depth 1 only"),
    ("MLP width 128", dict(readout_width=64, readout_depth=1, mlp_width=128), "read-out width 33..64 has no fused instance with MLP width 65..128"),
])
def test_limits_next_to_the_new_width_stay_refused(hip_lib, model_dir, kernel, what, over, reason):
    """Read-out width 65, read-out depth 2 with width 64, MLP width 128 with width 64: layer-at-a-time float32 kernels by default, within 5e-4 of the oracle; path=fused
    fails naming the limit."""
    d = fsc.model(model_dir, "Cu2AgO4", kernel, num_layers=2, **over)
    res = fsc.run(hip_lib, d)
    print(f"{kernel} {what}: {res['info']['path']}, max|dF| vs f64 oracle {np.abs(res['forces'] - d['ref']['forces']).max():.3e}")
    assert res["info"]["path"] == "generic_f32"
    util.assert_close_to(res, d["ref"], 5e-4, what=what)
    with pytest.raises(Exception, match="fused path unavailable.*" + reason):
        fsc.run(hip_lib, d, {"path": "fused"})


def test_wide_tile_auto_with_readout_width_64_is_the_64_slot_shape(hip_lib, model_dir):
    """k_fused_lx has no 128-slot instance of read-out width 64: wide_tile=auto behaves as "64" and is no error.  On fcc Cu at r_max 6.1 (78 neighbours, above a 64-slot
    tile) the model then runs as it does under wide_tile=64, within 5e-4 of the oracle."""
    c = fsc.model(model_dir, "Cu108", "k_fused_lx", readout_width=64, readout_depth=1)
    auto = fsc.run(hip_lib, c, {"wide_tile": "auto"})
    s64 = fsc.run(hip_lib, c, {"wide_tile": "64"})
    print(f"Cu108 k_fused_lx read-out width 64: wide_tile=auto {auto['info']['path']}, wide_tile=64 {s64['info']['path']}, max degree {auto['info']['max_degree']}")
    assert 64 < auto["info"]["max_degree"] <= 128
    assert auto["info"]["path"] == s64["info"]["path"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="read-out width 64, wide_tile=auto")
    util.assert_close_to(s64, c["ref"], 5e-4, what="read-out width 64, wide_tile=64")


AV_NAMES = ["Ag", "Cu", "O"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_width_64_atomic_virial(hip_lib, model_dir, kernel):
    """The VAR_VA twins of the width-64 instances: output atomic_virial against the float64 oracle's W, bars of test_gpu_atomic_virial.py (2e-5 of max|W|; the symmetrised
    sum of W against the virial at 1e-6 of the row scale)."""
    g = util.load_golden("Cu2AgO4_r5")
    base, over = fsc.KERNELS[kernel]
    cfg = base(**dict(over, type_names=AV_NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), readout_width=64))
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/r64_av_{kernel}.ahip"
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
    print(f"atomic_virial read-out width 64 {kernel}: max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)
