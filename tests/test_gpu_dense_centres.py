"""Option dense_centres=split on the MI355X: a list with a few centres above a fused kernel's tile (128 edges for k_fused, 64 for the wide kernels) behind list rows
of more than 128 entries keeps the fused kernel for the other centres; the few go to the layer-at-a-time kernels (tests/dense_centres_cases.py: the geometries, their
degree structure asserted by brute force).  Against the float64 oracle and against the same model on path=generic, at the tolerances of the fused parity tests."""
import numpy as np
import pytest

import atomic_virial_ref as av
import dense_centres_cases as dc
import parity_cases as pc
import util
from pair_allegro_amd import capi
from pair_allegro_amd.pair import PairAllegro

pytestmark = pytest.mark.gpu

TOL = pc.TOL["float32"]
SPLIT = {"dense_centres": "split"}
_runs = {}


def _shared(lib, model_dir, name, key, **kw):
    """An evaluation several tests compare against: computed once."""
    if (name, key) not in _runs:
        _runs[(name, key)] = dc.run(lib, dc.case(model_dir, name), **kw)
    return _runs[(name, key)]


def _generic(lib, model_dir, name):
    return _shared(lib, model_dir, name, "generic", options={"path": "generic"})


def _split(lib, model_dir, name):
    return _shared(lib, model_dir, name, "split", options=SPLIT)


def _check_results(res, c, gen, what):
    util.assert_close_to(res, c["ref"], TOL, what=f"{what} vs the float64 oracle")
    assert np.abs(res["forces"] - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF
    util.assert_close_to(res, gen, TOL, what=f"{what} vs path=generic")


def _check_structure(c, nheavy_max_over_8=True):
    deg, thresh = c["deg"], c["thresh"]
    nh = int((deg > thresh).sum())
    assert nh >= 1 and deg.max() > thresh
    assert (nh * 8 <= len(deg)) == nheavy_max_over_8
    assert int(c["rs"].numneigh.max()) > 128                 # a list row longer than the single-pass edge build takes: the two-pass route
    return nh


@pytest.mark.parametrize("name", ["S_light4", "S_light8"])
def test_model_S_keeps_k_fused_beside_centres_above_128_edges(hip_lib, model_dir, name):
    """Cases 1 and 2: four centres with 134 edges, every other centre with 54 (light tiles of 64 slots, 4 waves) or 78 (128 slots, 8 waves: wrong if the tile shape
    followed the list's largest degree or another header word).  The fused path is reported, the heavy count and edge total equal the brute-force ones, the tiles hold
    exactly the light centres' edges, and forces, per-atom energies, energy and virial are within tolerance of the oracle and of path=generic."""
    c = dc.case(model_dir, name)
    _check_structure(c)
    light = c["deg"][c["deg"] <= 128]
    assert c["deg"].max() > 128
    if name == "S_light4":
        assert light.max() <= 64
    else:
        assert ((light >= 65) & (light <= 128)).any()
    gen, res = _generic(hip_lib, model_dir, name), _split(hip_lib, model_dir, name)
    assert gen["path"] == "generic_f32" and gen["heavy"] == (0, 0)
    assert res["path"] in pc.FUSED_F32EQ
    assert res["heavy"] == dc.heavy_counts(c)
    assert res["max_degree"] == c["deg"].max() and res["nedges"] == c["deg"].sum()
    used, total = res["occupancy"]
    assert used == light.sum()                               # only the slots of processed tiles: no slot of theirs went to a heavy centre
    slots = 64 if name == "S_light4" else 128
    assert total % slots == 0 and used <= total < 2 * used
    _check_results(res, c, gen, name)


def test_dense_centres_whole_is_the_default_and_sends_the_list_to_the_layer_at_a_time_kernels(hip_lib, model_dir):
    c = dc.case(model_dir, "S_light4")
    res = dc.run(hip_lib, c)
    assert res["path"] == "generic_f32" and res["heavy"] == (0, 0) and res["occupancy"] == (0, 0)
    util.assert_close_to(res, _generic(hip_lib, model_dir, "S_light4"), TOL, what="default vs path=generic")


def test_model_S_more_than_one_centre_in_eight_is_heavy(hip_lib, model_dir):
    """Case 3, the give-up rule: with a quarter of the centres above 128 edges the whole list goes to the layer-at-a-time kernels under split too."""
    c = dc.case(model_dir, "S_giveup")
    nh = _check_structure(c, nheavy_max_over_8=False)
    assert nh * 8 > len(c["deg"])
    gen, res = _generic(hip_lib, model_dir, "S_giveup"), dc.run(hip_lib, c, options=SPLIT)
    assert res["path"] == "generic_f32" and res["heavy"] == (0, 0)
    _check_results(res, c, gen, "give-up")
    with pytest.raises(Exception, match="one centre in eight"):          # path=fused turns the refusal into the error, with its reason
        dc.run(hip_lib, c, options=dict(SPLIT, path="fused"))


def test_wide_model_with_long_list_rows(hip_lib, model_dir):
    """Case 4: k_fused_lx, four centres with 78 edges, the rest with 54, list rows of 140 and more entries (skin 1.3 A).  Fused under split; the default takes the
    layer-at-a-time kernels for the whole list, as before."""
    c = dc.case(model_dir, "lx_rows")
    _check_structure(c)
    assert c["deg"][c["deg"] <= 64].size == len(c["deg"]) - len(dc.HEAVY) and c["deg"].max() <= 128
    whole = dc.run(hip_lib, c)
    assert whole["path"] == "generic_f32"
    gen, res = _generic(hip_lib, model_dir, "lx_rows"), _split(hip_lib, model_dir, "lx_rows")
    assert res["path"] in pc.FUSED_F32EQ
    assert res["heavy"] == dc.heavy_counts(c)
    assert res["occupancy"][0] == c["deg"][c["deg"] <= 64].sum()
    _check_results(res, c, gen, "k_fused_lx, long rows")


def test_atomic_virial_with_heavy_centres_of_model_S(hip_lib, model_dir):
    """Case 5: the per-atom virial rows (tests/atomic_virial_ref.py) with the heavy centres' edges coming from the layer-at-a-time kernels' instance, the
    bars of tests/test_gpu_atomic_virial.py; their symmetric sum is the virial."""
    c = dc.case(model_dir, "S_light4")
    ref = dc.oracle_w(c)
    res = dc.run(hip_lib, c, options=SPLIT, register=True)
    assert res["path"] in pc.FUSED_F32EQ and res["heavy"] == dc.heavy_counts(c)
    assert res["W"].shape == ref.shape
    assert np.abs(res["W"] - ref).max() <= 2e-5 * np.abs(ref).max()
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    assert np.abs(av.sym_sum(res["W"]) - res["virial"]).max() <= 1e-6 * rowscale
    plain = _split(hip_lib, model_dir, "S_light4")                        # registering the output changes nothing else
    assert np.abs(res["f"] - plain["f"]).max() <= 1e-10 * np.abs(plain["f"]).max()


def test_forces_are_added_to_f(hip_lib, model_dir):
    """Case 6: f is not zero on entry; both contributions (fused kernel, heavy centres) are added to it."""
    c = dc.case(model_dir, "S_light4")
    f0 = np.random.RandomState(3).normal(size=c["rs"].x.shape)
    res = dc.run(hip_lib, c, options=SPLIT, f0=f0)
    plain = _split(hip_lib, model_dir, "S_light4")
    assert res["path"] == plain["path"]
    np.testing.assert_allclose(res["f"] - f0, plain["f"], rtol=0, atol=1e-12 * max(1.0, np.abs(f0).max()) + 1e-10 * np.abs(plain["f"]).max())


def test_device_resident_call(hip_lib, model_dir):
    """Case 7: ahip_compute_dev with the option: forces (added to the caller's device array), the seven sums and the per-atom energies equal the host-pointer call's."""
    import torch
    c = dc.case(model_dir, "S_light4")
    rs, cfg = c["rs"], c["cfg"]
    host = _split(hip_lib, model_dir, "S_light4")
    m = capi.Model(c["path"], 0, hip_lib)
    m.set_option("dense_centres", "split")
    m.neigh_update_csr(rs.nall, rs.ilist, rs.offsets, rs.flat)
    dev = torch.device("cuda", 0)
    x = torch.tensor(rs.x, device=dev)
    mt = torch.tensor(rs.type - 1, dtype=torch.int32, device=dev)         # LAMMPS types 1, 2 -> model types 0, 1 (NAMES order)
    f = torch.ones_like(x)
    ea = torch.zeros(rs.nall, dtype=torch.float64, device=dev)
    ev = torch.zeros(7, dtype=torch.float64, device=dev)
    m.compute_dev(rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), ea.data_ptr(), ev.data_ptr())
    torch.cuda.synchronize()
    path, heavy = m.last_path, m.last_heavy_centres
    m.close()
    assert path == host["path"] and heavy == dc.heavy_counts(c)
    fs = np.abs(host["f"]).max()
    assert np.abs(f.cpu().numpy() - 1.0 - host["f"]).max() <= 1e-9 * max(fs, 1.0)
    evh = ev.cpu().numpy()
    assert abs(evh[0] - host["pe"]) <= 1e-9 * abs(host["pe"])
    assert np.abs(evh[1:] - host["virial"]).max() <= 1e-9 * np.abs(host["virial"]).max()
    e_dev = np.zeros(len(c["pos"]))
    e_dev[rs.tag[: rs.nlocal] - 1] = ea.cpu().numpy()[: rs.nlocal]
    assert np.abs(e_dev - host["eatom"]).max() <= 1e-9 * np.abs(host["eatom"]).max()


def test_device_resident_range_call(hip_lib, model_dir):
    """ahip_compute_dev_range narrows the list and evaluates it like the whole-list call, heavy centres included: two ranges add up to the whole."""
    import torch
    c = dc.case(model_dir, "S_light4")
    rs = c["rs"]
    host = _split(hip_lib, model_dir, "S_light4")
    m = capi.Model(c["path"], 0, hip_lib)
    m.set_option("dense_centres", "split")
    m.neigh_update_csr(rs.nall, rs.ilist, rs.offsets, rs.flat)
    dev = torch.device("cuda", 0)
    x = torch.tensor(rs.x, device=dev)
    mt = torch.tensor(rs.type - 1, dtype=torch.int32, device=dev)
    f = torch.zeros_like(x)
    pe, seen = 0.0, []
    for c0, c1 in ((0, 150), (150, rs.nlocal)):               # heavy centres 5, 100 and 102 in the first range, 201 in the second
        ev = torch.zeros(7, dtype=torch.float64, device=dev)
        m.compute_dev_range(c0, c1, rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), 0, ev.data_ptr())
        torch.cuda.synchronize()
        assert m.last_path == host["path"]
        seen.append(m.last_heavy_centres[0])
        pe += float(ev[0])
    m.close()
    assert seen == [3, 1]
    np.testing.assert_allclose(f.cpu().numpy(), host["f"], rtol=0, atol=2e-5)         # other tile boundaries: another float32 summation order (tests/test_gpu_fused.py: fused vs generic)
    np.testing.assert_allclose(pe, host["pe"], rtol=TOL, atol=TOL)


def test_option_lifecycle_on_one_model(hip_lib, model_dir):
    """Case 8: one model object, whole -> split -> whole on the same geometry: generic_f32, a fused path, generic_f32 again, the same forces."""
    c = dc.case(model_dir, "S_light4")
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"]] + dc.NAMES, ntypes=2)
    pair.init_style()
    runs = [dc.run(hip_lib, c, options={"dense_centres": v}, pair=pair) for v in ("whole", "split", "whole")]
    pair.model.close()
    assert runs[0]["path"] == "generic_f32" and runs[1]["path"] in pc.FUSED_F32EQ and runs[2]["path"] == "generic_f32"
    assert [r["heavy"][0] for r in runs] == [0, len(dc.HEAVY), 0]
    for r in runs[1:]:
        util.assert_close_to(r, runs[0], TOL, what="whole -> split -> whole")
