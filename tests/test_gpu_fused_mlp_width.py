"""GPU tests of the MLP-width-128 instances of k_fused and k_fused_lx (template parameters WT / HT = 8: csrc/fused.hip, csrc/fused_lx.hip; objects fused_hm.o and
fused_lx_m.o): a model with 65 <= `allegro_mlp_hidden_layers_width` <= 128 (64 in the reference's tests/test_data/test_repro_allegro.yaml:95) runs fused, zero-padded to
hidden width 128, on the f16x2 arithmetic with read-out depth 1.  Before these instances existed such a model ran on the layer-at-a-time float32 kernels (`generic_f32`).

Geometries and bars are those of tests/fused_shape_cases.py: the 7-atom triclinic Cu2AgO4 golden (3 types, degrees 36..39: ragged tiles), the 256-atom CuPd box relabelled
O / H (degree 42: every wave carries edges), the same box doubled along x, the 108-atom jittered fcc Cu box at r_max 6.1 (78 neighbours: the 8-wave tile of k_fused).  The
float64 oracle runs once per model and is shared.  `twin` is the mlp_width = 64 model of the same kernel, depths and geometry, so the bars come from the project
(fused_shape_cases.assert_bars): max|dF| against the float64 oracle below parity_cases.NORTH_STAR_DF and below max(3 e_generic, 1e-5), e_generic being the error of the
layer-at-a-time float32 kernels on the same file -- or twice the twin's error where the twin itself misses that bar; energies and virial util.assert_close_to(.., 5e-4).
Every figure is printed before it is asserted.
Measured on the MI355X (max|dF|, eV/A): the 18 width-128 instances on Cu2AgO4 6.1e-7 .. 2.6e-6, their width-64 twins 3.4e-7 .. 1.9e-6 (always inside max(3 e_generic, 1e-5),
so the fall-back bar is not in use), the layer-at-a-time float32 kernels 1.1e-6 .. 6.4e-6; widths 65 / 72 / 96 / 100 3.1e-7 .. 1.7e-6; 256-atom box 5.7e-7 (k_fused) /
1.6e-6 (k_fused_lx); the 8-wave tile of k_fused 8.3e-7; the f16x2 linear alone 4.9e-7 at 64 x 64 and 0.91 .. 1.39 times that at the new shapes."""
import numpy as np
import pytest
import torch

import atomic_virial_ref as av
import fused_shape_cases as fsc
import parity_cases as pc
import util
from pair_allegro_amd import model_file

pytestmark = pytest.mark.gpu

KERNELS = ["k_fused", "k_fused_lx"]


def _pair(model_dir, tag, kernel, width=128, **over):
    """The model of MLP width `width` and its mlp_width = 64 twin (same kernel, other widths, depths, layers, geometry)."""
    over.setdefault("readout_depth", 1)
    return fsc.model(model_dir, tag, kernel, **dict(over, mlp_width=width)), fsc.model(model_dir, tag, kernel, **over)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("md", [1, 2, 3])
def test_every_mlp_width_128_instance_ragged_tiles(hip_lib, model_dir, md, nl, kernel):
    """Every compiled width-128 instance (2 kernels x 1..3 layers x latent MLP depth 1..3) on Cu2AgO4: fused_f16x2 under default options, within the bars."""
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, num_layers=nl, mlp_depth=md)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} {nl} layers MLP depth {md} MLP width 128")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("width", [65, 72, 96])
def test_padding_inside_the_new_width(hip_lib, model_dir, kernel, width):
    """Widths that do not fill the 8 hidden tiles: 65 (one feature in the fifth tile), 72 (a half-filled tile), 96 (6 tiles, the last pair all padding)."""
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, width=width, num_layers=2)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} MLP width {width}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_narrow_model_with_mlp_width_100(hip_lib, model_dir, kernel):
    """S 48, U 16, read-out width 24 with MLP width 100: every width padded at once, the hidden one to 128."""
    over = dict(fsc.NARROW, mlp_width=64)
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, width=100, **over)
    assert c["cfg"]["mlp_width"] == 100 and twin["cfg"]["mlp_width"] == 64 and c["cfg"]["num_scalar_features"] == 48
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} narrow model, MLP width 100")


@pytest.mark.parametrize("kernel", KERNELS)
def test_mlp_width_128_full_tiles(hip_lib, model_dir, kernel):
    """Three layers on the 256-atom box: degree 42, so every wave of a tile works on real edges."""
    c, twin = _pair(model_dir, "CuPd256", kernel, num_layers=3)
    fsc.assert_bars(hip_lib, c, twin, f"CuPd256 {kernel} MLP width 128")
    assert c["fused"]["info"]["max_degree"] > 32


def test_mlp_width_128_eight_wave_tile_of_k_fused(hip_lib, model_dir):
    """fcc Cu at r_max 6.1: 78 neighbours per atom, more than a 64-slot tile, so the 8-wave / 128-slot instances of k_fused run."""
    c, twin = _pair(model_dir, "Cu108", "k_fused")
    fsc.assert_bars(hip_lib, c, twin, "Cu108 k_fused (8-wave tiles) MLP width 128")
    assert 64 < c["fused"]["info"]["max_degree"] <= 128


@pytest.mark.parametrize("kernel", KERNELS)
def test_mlp_width_128_more_tiles_than_workgroups(hip_lib, model_dir, kernel):
    """One workgroup consumes the (longer) weight stream more than once and prefetches across the tile boundary: reserve_wgs=128 leaves CUs - 64 workgroups for the 256
    tiles of the 256-atom box on k_fused_lx, 2 CUs - 128 for the 512 tiles of the doubled box on k_fused.  Against reserve_wgs=0 on the same model: per-atom energies bit
    for bit, forces within 1e-9 of max|F| (float64 atomics in arrival order) -- the criterion of test_gpu_soak.py."""
    tag = "CuPd512" if kernel == "k_fused" else "CuPd256"
    c = fsc.model(model_dir, tag, kernel, mlp_width=128, readout_depth=1, num_layers=3)
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
    assert np.abs(forces - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF


@pytest.mark.parametrize("kernel", KERNELS)
def test_mlp_width_128_without_f16x2_is_refused_or_falls_back(hip_lib, model_dir, monkeypatch, kernel):
    """Width 128 exists on the f16x2 arithmetic only (k_fused: with the tabulated two-body embedding): fused_arith=f32 sends the model to the layer-at-a-time float32
    kernels, path=fused then fails with the gate's reason; fused_arith=auto with its first-evaluation self-check on (whose float32 pass runs on the layer-at-a-time
    kernels) ends on f16x2 and says so."""
    monkeypatch.delenv("AHIP_NO_ARITH_SELFCHECK", raising=False)
    c = fsc.model(model_dir, "Cu2AgO4", kernel, mlp_width=128, readout_depth=1, num_layers=3)
    exact = fsc.run(hip_lib, c, {"fused_arith": "f32"})
    assert exact["info"]["path"] == "generic_f32"
    util.assert_close_to(exact, c["ref"], 5e-4, what="MLP width 128, fused_arith=f32")
    with pytest.raises(Exception, match="fused path unavailable.*MLP width 65..128 runs on the f16x2 arithmetic"):
        fsc.run(hip_lib, c, {"path": "fused", "fused_arith": "f32"})
    if kernel == "k_fused":
        with pytest.raises(Exception, match="fused path unavailable.*MLP width 65..128 runs on the f16x2 arithmetic with the tabulated two-body embedding only"):
            fsc.run(hip_lib, c, {"path": "fused", "fused_tb": "mlp"})
        mlp = fsc.run(hip_lib, c, {"fused_tb": "mlp"})
        assert mlp["info"]["path"] == "generic_f32"
    auto = fsc.run(hip_lib, c, {"fused_arith": "auto"})
    assert auto["info"]["path"] == "fused_f16x2"
    assert "f16x2 kept" in auto["info"]["arith_note"], auto["info"]["arith_note"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="MLP width 128, fused_arith=auto")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("what,over,reason", [
    ("read-out depth 2", dict(mlp_width=128, readout_depth=2), "MLP width 65..128 runs with read-out depth 1 only"),
    ("64 tensor features", dict(mlp_width=128, readout_depth=1, num_tensor_features=64), "33..64 tensor features"),
    ("MLP width 129", dict(mlp_width=129, readout_depth=1), "MLP width 128"),
])
def test_limits_next_to_the_new_width_stay_refused(hip_lib, model_dir, kernel, what, over, reason):
    """Read-out depth 2 with width 128, 33..64 tensor features (k_fused_lx2) with width 128, and width 129: layer-at-a-time float32 kernels by default, within 5e-4 of the
    oracle; path=fused fails naming the limit."""
    d = fsc.model(model_dir, "Cu2AgO4", kernel, num_layers=2, **over)
    res = fsc.run(hip_lib, d)
    print(f"{kernel} {what}: {res['info']['path']}, max|dF| vs f64 oracle {np.abs(res['forces'] - d['ref']['forces']).max():.3e}")
    assert res["info"]["path"] == "generic_f32"
    util.assert_close_to(res, d["ref"], 5e-4, what=what)
    with pytest.raises(Exception, match="fused path unavailable.*" + reason):
        fsc.run(hip_lib, d, {"path": "fused"})


def test_wide_tile_auto_with_mlp_width_128_is_the_64_slot_shape(hip_lib, model_dir):
    """k_fused_lx has no 128-slot instance of width 128: wide_tile=auto behaves as "64" and is no error.  On fcc Cu at r_max 6.1 (78 neighbours, above a 64-slot tile) the
    model then runs as it does under wide_tile=64 -- on the layer-at-a-time kernels -- within 5e-4 of the oracle."""
    c = fsc.model(model_dir, "Cu108", "k_fused_lx", mlp_width=128, readout_depth=1)
    auto = fsc.run(hip_lib, c, {"wide_tile": "auto"})
    s64 = fsc.run(hip_lib, c, {"wide_tile": "64"})
    print(f"Cu108 k_fused_lx MLP width 128: wide_tile=auto {auto['info']['path']}, wide_tile=64 {s64['info']['path']}, max degree {auto['info']['max_degree']}")
    assert 64 < auto["info"]["max_degree"] <= 128
    assert auto["info"]["path"] == s64["info"]["path"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="MLP width 128, wide_tile=auto")
    util.assert_close_to(s64, c["ref"], 5e-4, what="MLP width 128, wide_tile=64")


AV_NAMES = ["Ag", "Cu", "O"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_mlp_width_128_atomic_virial(hip_lib, model_dir, kernel):
    """The VAR_VA twins of the width-128 instances: output atomic_virial against the float64 oracle's W, bars of test_gpu_atomic_virial.py (2e-5 of max|W|; the symmetrised
    sum of W against the virial at 1e-6 of the row scale)."""
    g = util.load_golden("Cu2AgO4_r5")
    base, over = fsc.KERNELS[kernel]
    cfg = base(**dict(over, type_names=AV_NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), mlp_width=128))
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/w128_av_{kernel}.ahip"
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
    print(f"atomic_virial MLP width 128 {kernel}: max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)


def _linear_error(hip_lib, K, N):
    """max |out - x @ W| of the streamed f16x2 linear against the float64 product.  W ~ N(0, 1 / K), as a model's variance-preserving weights are, so that the outputs are
    O(1) at every K and the absolute errors of different shapes compare; W and x are float32 values, so the figure is the arithmetic's error alone."""
    rng = np.random.RandomState(K * 100 + N)
    W = (rng.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32).astype(np.float64)
    x = rng.normal(size=(32, K)).astype(np.float32)
    out = hip_lib.debug_fused_linear(W, x)
    ref = x.astype(np.float64) @ W
    return float(np.abs(out - ref).max()), float(np.abs(ref).max())


def test_f16x2_linear_primitive_at_the_new_shapes(hip_lib, monkeypatch):
    """The f16x2 linear alone at the (K-steps, output tiles) the width-128 instances use -- (3, 8), (4, 8), (4, 4), (1, 8), (4, 6), and (2, 8), (4, 2) of the backward
    and folded read-out linears: error no larger than twice that of the existing 64 x 64 shape measured in this run (DESIGN 4.2a's yardstick, not assumed)."""
    monkeypatch.setenv("AHIP_FUSED_ARITH", "f16x2")
    e64, s64 = _linear_error(hip_lib, 64, 64)
    print(f"f16x2 linear 64 x 64: max error {e64:.3e} (max|out| {s64:.2f})")
    assert 0.0 < e64 < 2e-5 * s64          # the bar of test_gpu_fused.py: test_mfma_linear_primitive
    bad = []
    for K, N in [(96, 128), (128, 128), (128, 64), (32, 128), (128, 96), (64, 128), (128, 32)]:
        e, s = _linear_error(hip_lib, K, N)
        print(f"f16x2 linear {K} x {N}: max error {e:.3e} (max|out| {s:.2f}), {e / e64:.2f} x the 64 x 64 figure")
        if not e <= 2.0 * e64:
            bad.append((K, N, e))
    assert not bad, (bad, e64)
