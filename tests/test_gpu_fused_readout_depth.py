"""GPU tests of the read-out-depth-2 instances of the three fused kernels (template parameter RD of k_fused, k_fused_lx, k_fused_lx2: csrc/fused.hip, csrc/fused_lx.hip,
csrc/fused_lx2.hip): `readout_mlp_hidden_layers_depth` = 2 (1 in /root/reference/tests/test_data/test_repro_allegro.yaml), f16x2 arithmetic only.

Geometries (tests/fused_shape_cases.py): the 7-atom triclinic Cu2AgO4 golden (3 types, degrees 36..39, several centres per tile), the 256-atom CuPd box relabelled O / H
(degree 42: every wave carries edges), the same box doubled along x, and the 108-atom jittered fcc Cu box at r_max 6.1 (78 neighbours: the 8-wave tile of k_fused).  The float64
oracle runs once per model and is shared.

Error bars of max|dF| against the float64 oracle are those of tests/test_gpu_fused_lx_depth.py (fused_shape_cases.assert_bars): below parity_cases.NORTH_STAR_DF and below
max(3 e_generic, 1e-5), e_generic being the error of the layer-at-a-time float32 kernels on the same file; where the existing read-out-depth-1 instance of the same shape itself
misses that second bar, twice that instance's measured error instead.  Energies and virial: util.assert_close_to(.., 5e-4).  Every figure is printed before it is asserted.
Measured on the MI355X (max|dF|, eV/A): the 27 RD = 2 instances on Cu2AgO4 2.1e-7 .. 2.3e-6, their RD = 1 twins 3.4e-7 .. 1.9e-6 (always inside max(3 e_generic, 1e-5), so
the fall-back bar is not in use), the layer-at-a-time float32 kernels 6.4e-7 .. 5.7e-6; 256-atom box 2.5e-6 (k_fused) / 6.4e-7 (k_fused_lx) / 8.4e-7 (k_fused_lx2); the 8-wave tile
of k_fused 1.1e-6 ("Read-out depth 2")."""
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


def _pair(model_dir, tag, kernel, **over):
    """The read-out-depth-2 model and its depth-1 twin (same kernel, widths, layers, geometry)."""
    return fsc.model(model_dir, tag, kernel, readout_depth=2, **over), fsc.model(model_dir, tag, kernel, readout_depth=1, **over)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("md", [1, 2, 3])
def test_every_readout_depth_2_instance_ragged_tiles(hip_lib, model_dir, md, nl, kernel):
    """Every compiled RD = 2 instance (3 kernels x 1..3 layers x latent MLP depth 1..3) on Cu2AgO4: fused_f16x2 under default options, within the bars."""
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, num_layers=nl, mlp_depth=md)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} {nl} layers MLP depth {md} read-out depth 2")


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_depth_2_full_tiles(hip_lib, model_dir, kernel):
    """Three layers on the 256-atom box: degree 42, so every wave of a tile (both waves of every pair of k_fused_lx2) works on real edges."""
    c, twin = _pair(model_dir, "CuPd256", kernel, num_layers=3)
    fsc.assert_bars(hip_lib, c, twin, f"CuPd256 {kernel} read-out depth 2")
    assert c["fused"]["info"]["max_degree"] > 32


def test_readout_depth_2_eight_wave_tile_of_k_fused(hip_lib, model_dir):
    """fcc Cu at r_max 6.1: 78 neighbours per atom, more than a 64-slot tile, so the 8-wave / 128-slot instances of k_fused run."""
    c, twin = _pair(model_dir, "Cu108", "k_fused")
    fsc.assert_bars(hip_lib, c, twin, "Cu108 k_fused (8-wave tiles) read-out depth 2")
    assert 64 < c["fused"]["info"]["max_degree"] <= 128


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_depth_2_more_tiles_than_workgroups(hip_lib, model_dir, kernel):
    """One workgroup consumes the weight stream more than once and prefetches across the tile boundary: reserve_wgs=128 leaves CUs - 64 workgroups for the 256 tiles of the
    256-atom box on the wide kernels, 2 CUs - 128 for the 512 tiles of the doubled box on k_fused.  Against reserve_wgs=0 on the same model: per-atom energies bit for
    bit, forces within 1e-9 of max|F| (float64 atomics in arrival order) -- the criterion of test_gpu_soak.py."""
    tag = "CuPd512" if kernel == "k_fused" else "CuPd256"
    c = fsc.model(model_dir, tag, kernel, readout_depth=2, num_layers=3)
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
    assert int((e1 != e0).sum()) == 0
    assert np.abs(f1 - f0).max() <= 1e-9 * np.abs(f0).max()
    assert abs(pe1 - pe0) <= 1e-12 * abs(pe0)
    forces = np.zeros((len(c["pos"]), 3))
    np.add.at(forces, rs.tag - 1, f1)
    assert np.abs(forces - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_depth_2_without_f16x2_is_refused_or_falls_back(hip_lib, model_dir, monkeypatch, kernel):
    """RD = 2 exists on the f16x2 arithmetic only: fused_arith=f32 sends the model to the layer-at-a-time float32 kernels, path=fused then fails with the gate's reason;
    fused_arith=auto with its first-evaluation self-check on (whose float32 pass runs on the layer-at-a-time kernels) ends on f16x2 and says so.  Read-out depth 0 and 3
    have no instance at all."""
    monkeypatch.delenv("AHIP_NO_ARITH_SELFCHECK", raising=False)
    c = fsc.model(model_dir, "Cu2AgO4", kernel, readout_depth=2, num_layers=3)
    exact = fsc.run(hip_lib, c, {"fused_arith": "f32"})
    assert exact["info"]["path"] == "generic_f32"
    util.assert_close_to(exact, c["ref"], 5e-4, what="read-out depth 2, fused_arith=f32")
    with pytest.raises(Exception, match="fused path unavailable.*read-out depth 2 runs on the f16x2 arithmetic"):
        fsc.run(hip_lib, c, {"path": "fused", "fused_arith": "f32"})
    auto = fsc.run(hip_lib, c, {"fused_arith": "auto"})
    assert auto["info"]["path"] == "fused_f16x2"
    assert "f16x2 kept" in auto["info"]["arith_note"], auto["info"]["arith_note"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="read-out depth 2, fused_arith=auto")
    for rd in (0, 3):
        d = fsc.model(model_dir, "Cu2AgO4", kernel, readout_depth=rd, num_layers=2)
        res = fsc.run(hip_lib, d, {"fused_arith": "auto"})
        assert res["info"]["path"] == "generic_f32"
        util.assert_close_to(res, d["ref"], 5e-4, what=f"read-out depth {rd}")
        with pytest.raises(Exception, match="fused path unavailable.*read-out depth 1..2"):
            fsc.run(hip_lib, d, {"path": "fused"})


def _shift_readout_scale(w):
    w["out.w1"] = np.asarray(w["out.w1"]) * 2.0 ** -14
    w["out.w2"] = np.asarray(w["out.w2"]) * 2.0 ** 14


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_depth_2_tiny_second_layer_leaves_f16x2_under_auto(hip_lib, model_dir, kernel):
    """out.w1 scaled by 2^-14 (every weight below 2^-10: float16 subnormal territory for the split) and out.w2 by 2^14: fused_arith=auto leaves f16x2 with the float16-range
    reason in its note; there is no float32 instance of RD = 2, so the model runs on the layer-at-a-time kernels, within 5e-4 of the oracle.  An explicit f16x2 keeps
    its documented behaviour: a tiny linear is the caller's choice, the model runs on the f16x2 instance (the split keeps an absolute 2^-36 of such a matrix, i.e. 2^-20
    of these pre-activations: still inside 5e-4)."""
    c = fsc.model(model_dir, "Cu2AgO4", kernel, edit=_shift_readout_scale, edit_name="_rdscale", readout_depth=2, num_layers=2)
    assert np.abs(c["w"]["out.w1"]).max() < 2.0 ** -10
    auto = fsc.run(hip_lib, c, {"fused_arith": "auto"})
    print(f"{kernel}: {auto['info']}")
    assert auto["info"]["path"] == "generic_f32"
    assert "float32 instance" in auto["info"]["arith_note"] and "float16" in auto["info"]["arith_note"], auto["info"]["arith_note"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="tiny out.w1, fused_arith=auto")
    forced = fsc.run(hip_lib, c, {"fused_arith": "f16x2"})
    print(f"{kernel}: explicit f16x2 max|dF| vs f64 oracle {np.abs(forced['forces'] - c['ref']['forces']).max():.3e}")
    assert forced["info"]["path"] == "fused_f16x2"
    util.assert_close_to(forced, c["ref"], 5e-4, what="tiny out.w1, explicit f16x2")


@pytest.mark.parametrize("kernel", ["k_fused", "k_fused_lx"])
def test_readout_depth_2_narrow_model_zero_padded(hip_lib, model_dir, kernel):
    """A narrower model (S 48, U 16, MLP width 40, read-out width 24) with RD = 2 runs zero-padded: out.w1 [24][24] is padded to [32][32]."""
    c, twin = _pair(model_dir, "Cu2AgO4", kernel, **fsc.NARROW)
    fsc.assert_bars(hip_lib, c, twin, f"Cu2AgO4 {kernel} narrow model read-out depth 2")


AV_NAMES = ["Ag", "Cu", "O"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_readout_depth_2_atomic_virial(hip_lib, model_dir, kernel):
    """The VAR_VA twins of the RD = 2 instances: output atomic_virial against the float64 oracle's W, bars of test_gpu_atomic_virial.py (2e-5 of max|W|; the symmetrised
    sum of W against the virial at 1e-6 of the row scale)."""
    g = util.load_golden("Cu2AgO4_r5")
    base, over = fsc.KERNELS[kernel]
    cfg = base(**dict(over, type_names=AV_NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), readout_depth=2))
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/rd2_av_{kernel}.ahip"
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
    print(f"atomic_virial read-out depth 2 {kernel}: max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)
