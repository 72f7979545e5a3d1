"""Option wide_tile=auto on the MI355X: k_fused_lx (l_max = 2, 32 tensor features) on its 8-wave / 128-slot tile shape where the list's largest degree is 65..128,
so that such centres stay on the fused kernel instead of going to the layer-at-a-time kernels as "heavy" ones (tests/wide_tile_cases.py: the geometries, their degree
structure asserted by brute force).  Against the float64 oracle and against the same model on path=generic, at the tolerances of the fused parity tests."""
import numpy as np
import pytest

import atomic_virial_ref as av
import dense_centres_cases as dc
import parity_cases as pc
import util
import wide_tile_cases as wt
from pair_allegro_amd import capi
from pair_allegro_amd.pair import PairAllegro

pytestmark = pytest.mark.gpu

TOL = pc.TOL["float32"]
AUTO = {"wide_tile": "auto"}
_runs = {}


def _shared(lib, c, key, **kw):
    """An evaluation several tests compare against: computed once per model file."""
    if (c["path"], key) not in _runs:
        _runs[(c["path"], key)] = dc.run(lib, c, **kw)
    return _runs[(c["path"], key)]


def _generic(lib, c):
    return _shared(lib, c, "generic", options={"path": "generic"})


def _auto(lib, c):
    return _shared(lib, c, "auto", options=AUTO)


def _check_results(res, c, gen, what):
    ref = wt.reference(c)
    util.assert_close_to(res, ref, TOL, what=f"{what} vs the float64 oracle")
    assert np.abs(res["forces"] - ref["forces"]).max() < pc.NORTH_STAR_DF
    util.assert_close_to(res, gen, TOL, what=f"{what} vs path=generic")


def _check_all_fused(res, c, slots=128):
    """Every centre ran in a tile of the fused kernel: no heavy centre, every edge in a slot, tiles of `slots` slots."""
    deg = c["deg"]
    assert res["path"] in pc.FUSED_F32EQ
    assert res["heavy"] == (0, 0)
    assert res["max_degree"] == deg.max() and res["nedges"] == deg.sum()
    used, total = res["occupancy"]
    assert used == deg.sum() and total % slots == 0 and total >= used


@pytest.mark.parametrize("name", ["all78", "mixed", "sparse", "rows140"])
def test_centres_with_65_to_128_edges_stay_on_the_fused_kernel(hip_lib, model_dir, name):
    """1: 78-edge centres alone (every tile: one centre, waves 5..7 empty), beside 54-edge centres (two per tile), beside 12-edge centres (tiles closed by the centre
    limit), and behind list rows of 140 (two-pass edge build: the host picks the shape).  Nothing is heavy, every edge sits in a 128-slot tile, results as the oracle's."""
    c = wt.case(model_dir, name)
    gen, res = _generic(hip_lib, c), _auto(hip_lib, c)
    assert gen["path"] == "generic_f32"
    _check_all_fused(res, c)
    _check_results(res, c, gen, name)


def test_centres_above_128_edges_are_still_heavy(hip_lib, model_dir):
    """2: four centres with 134 edges beside 252 with 78: under dense_centres=split the 252 run in 128-slot tiles and the four on the layer-at-a-time kernels;
    without split the list goes to the layer-at-a-time kernels as a whole, as before."""
    c = wt.case(model_dir, "above128")
    deg = c["deg"]
    res = dc.run(hip_lib, c, options=dict(AUTO, dense_centres="split"))
    assert res["path"] in pc.FUSED_F32EQ
    assert res["heavy"] == (4, 4 * 134)
    assert res["max_degree"] == 134 and res["nedges"] == deg.sum()
    used, total = res["occupancy"]
    assert used == deg[deg <= 128].sum() and total % 128 == 0
    _check_results(res, c, _generic(hip_lib, c), "above128, split")
    whole = dc.run(hip_lib, c, options=AUTO)
    assert whole["path"] == "generic_f32" and whole["heavy"] == (0, 0)


def test_light_list_behind_long_rows_runs_the_64_slot_shape(hip_lib, model_dir):
    """3: list rows of 86 entries but degrees of 54: the host cannot know, both shapes are launched and the device word picks the 64-slot one."""
    c = wt.case(model_dir, "light")
    res, narrow = _auto(hip_lib, c), dc.run(hip_lib, c, options={"wide_tile": "64"})
    _check_all_fused(res, c, slots=64)
    assert res["occupancy"][1] == 64 * len(c["deg"])             # 54 + 54 > 64: one centre per 64-slot tile
    assert narrow["path"] == res["path"] and narrow["heavy"] == (0, 0)
    assert np.abs(res["f"] - narrow["f"]).max() <= 2e-5          # the stand-alone packing may cut the tiles elsewhere than the edge build's: another summation order
    _check_results(res, c, _generic(hip_lib, c), "light")


@pytest.mark.parametrize("over,options,path", [(dict(num_layers=1), {}, None), (dict(num_layers=2), {}, None), (dict(), {"fused_arith": "f32"}, "fused_f32")],
                         ids=["1_layer", "2_layers", "f32"])
def test_every_layer_count_and_both_arithmetics(hip_lib, model_dir, over, options, path):
    """4: the instances the three-layer default-arithmetic cases do not reach (fused_arith=auto runs the f32 and the f16x2 instance in its first evaluation)."""
    c = wt.case(model_dir, "all78", **over)
    res = dc.run(hip_lib, c, options=dict(AUTO, **options))
    _check_all_fused(res, c)
    if path:
        assert res["path"] == path
    _check_results(res, c, _generic(hip_lib, c), "all78 " + str(over or options))


def test_atomic_virial(hip_lib, model_dir):
    """5: the per-atom virial rows from the 8-wave instances (tests/atomic_virial_ref.py), the bars of tests/test_gpu_atomic_virial.py; their symmetric sum is the virial."""
    c = wt.case(model_dir, "all78")
    ref = av.oracle_w(c["cfg"], c["w"], c["rs"], wt.NAMES)
    res = dc.run(hip_lib, c, options=AUTO, register=True)
    _check_all_fused(res, c)
    assert res["W"].shape == ref.shape
    assert np.abs(res["W"] - ref).max() <= 2e-5 * np.abs(ref).max()
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    assert np.abs(av.sym_sum(res["W"]) - res["virial"]).max() <= 1e-6 * rowscale
    plain = _auto(hip_lib, c)                                     # registering the output changes nothing else
    assert np.abs(res["f"] - plain["f"]).max() <= 1e-10 * np.abs(plain["f"]).max()


def _device_model(lib, c):
    import torch
    rs = c["rs"]
    m = capi.Model(c["path"], 0, lib)
    m.set_option("wide_tile", "auto")
    m.neigh_update_csr(rs.nall, rs.ilist, rs.offsets, rs.flat)
    dev = torch.device("cuda", 0)
    return m, torch.tensor(rs.x, device=dev), torch.tensor(rs.type - 1, dtype=torch.int32, device=dev), dev


def test_device_resident_call(hip_lib, model_dir):
    """6a: ahip_compute_dev with the option: forces (added to the caller's device array), the seven sums and the per-atom energies equal the host-pointer call's."""
    import torch
    c = wt.case(model_dir, "mixed")
    rs = c["rs"]
    host = _auto(hip_lib, c)
    m, x, mt, dev = _device_model(hip_lib, c)
    f = torch.ones_like(x)
    ea = torch.zeros(rs.nall, dtype=torch.float64, device=dev)
    ev = torch.zeros(7, dtype=torch.float64, device=dev)
    m.compute_dev(rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), ea.data_ptr(), ev.data_ptr())
    torch.cuda.synchronize()
    path, heavy, occ = m.last_path, m.last_heavy_centres, m.tile_occupancy()
    m.close()
    assert path == host["path"] and heavy == (0, 0) and occ == host["occupancy"]
    fs = np.abs(host["f"]).max()
    assert np.abs(f.cpu().numpy() - 1.0 - host["f"]).max() <= 1e-9 * max(fs, 1.0)
    evh = ev.cpu().numpy()
    assert abs(evh[0] - host["pe"]) <= 1e-9 * abs(host["pe"])
    assert np.abs(evh[1:] - host["virial"]).max() <= 1e-9 * np.abs(host["virial"]).max()
    e_dev = np.zeros(len(c["pos"]))
    e_dev[rs.tag[: rs.nlocal] - 1] = ea.cpu().numpy()[: rs.nlocal]
    assert np.abs(e_dev - host["eatom"]).max() <= 1e-9 * np.abs(host["eatom"]).max()


def test_device_resident_range_call(hip_lib, model_dir):
    """6b: two ahip_compute_dev_range halves add up to the whole-list call (78-edge centres 5, 100 and 102 in the first, 201 in the second)."""
    import torch
    c = wt.case(model_dir, "mixed")
    rs = c["rs"]
    host = _auto(hip_lib, c)
    m, x, mt, dev = _device_model(hip_lib, c)
    f = torch.zeros_like(x)
    pe = 0.0
    for c0, c1 in ((0, 150), (150, rs.nlocal)):
        ev = torch.zeros(7, dtype=torch.float64, device=dev)
        m.compute_dev_range(c0, c1, rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), 0, ev.data_ptr())
        torch.cuda.synchronize()
        assert m.last_path == host["path"] and m.last_heavy_centres == (0, 0)
        assert m.tile_occupancy()[1] % 128 == 0
        pe += float(ev[0])
    m.close()
    np.testing.assert_allclose(f.cpu().numpy(), host["f"], rtol=0, atol=2e-5)         # other tile boundaries: another float32 summation order (tests/test_gpu_dense_centres.py)
    np.testing.assert_allclose(pe, host["pe"], rtol=TOL, atol=TOL)


def test_forces_are_added_to_f(hip_lib, model_dir):
    """7: f is not zero on entry."""
    c = wt.case(model_dir, "all78")
    f0 = np.random.RandomState(3).normal(size=c["rs"].x.shape)
    res, plain = dc.run(hip_lib, c, options=AUTO, f0=f0), _auto(hip_lib, c)
    assert res["path"] == plain["path"] and res["heavy"] == (0, 0)
    np.testing.assert_allclose(res["f"] - f0, plain["f"], rtol=0, atol=1e-12 * max(1.0, np.abs(f0).max()) + 1e-10 * np.abs(plain["f"]).max())


@pytest.mark.parametrize("over", [dict(mlp_depth=3), dict(num_tensor_features=64)], ids=["mlp_depth_3", "lx64"])
def test_auto_is_the_64_slot_route_where_no_8_wave_instance_exists(hip_lib, model_dir, over):
    """8a: a latent MLP of depth 3 (k_fused_lx, f16x2 instances without an 8-wave twin) and 64 tensor features (k_fused_lx2): auto is not an error and changes nothing."""
    c = wt.case(model_dir, "all78", **over)
    narrow, res = dc.run(hip_lib, c, options={"wide_tile": "64"}), dc.run(hip_lib, c, options=AUTO)
    assert res["path"] == narrow["path"] and res["heavy"] == narrow["heavy"]
    assert res["occupancy"] == narrow["occupancy"]
    util.assert_close_to(res, narrow, TOL, what="auto vs 64 without an 8-wave instance")
    assert np.abs(res["f"] - narrow["f"]).max() <= 2e-5


def test_option_lifecycle_on_one_model(hip_lib, model_dir):
    """8b: one model object, 64 -> auto -> 64 on the same list: the four 78-edge centres are heavy, in tiles, heavy again; the same forces."""
    c = wt.case(model_dir, "mixed")
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"]] + wt.NAMES, ntypes=2)
    pair.init_style()
    runs = [dc.run(hip_lib, c, options={"wide_tile": v}, pair=pair) for v in ("64", "auto", "64")]
    pair.model.close()
    assert [r["heavy"] for r in runs] == [(4, 312), (0, 0), (4, 312)]
    assert all(r["path"] in pc.FUSED_F32EQ for r in runs)
    for r in runs[1:]:
        util.assert_close_to(r, runs[0], TOL, what="64 -> auto -> 64")


def test_option_values(hip_lib, model_dir):
    """9: anything but 64 | auto is an error that names the accepted values."""
    c = wt.case(model_dir, "all78")
    m = capi.Model(c["path"], 0, hip_lib)
    try:
        with pytest.raises(Exception, match=r"64\|auto"):
            m.set_option("wide_tile", "96")
        m.set_option("wide_tile", "auto")
        m.set_option("wide_tile", "64")
    finally:
        m.close()
