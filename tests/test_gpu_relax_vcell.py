"""GPU: ahip_relax_vcell.  The variable-cell kernels (csrc/neigh.hip: k_vcell_gather, k_vcell_decide, k_vcell_move, k_vcell_positions) and the host loop in
float64 against the numpy statement of vcell_cases over a fresh ahip_compute_cell on a second handle, on the golden models: the cases of the CPU tests plus
257 atoms for 12 moves (a block boundary and a partial wave in the row kernels) and a cell of one atom with c = 1, whose rebuilds the cell term
sum_d M_d g_d alone decides; then the float32 golden models on the fused kernels against that float64 reference.

The end point of a float32 run cannot match the float64 reference to 1e-9 A.  As in test_gpu_relax.py the bar is four times the deviation that the numpy
algorithm over the float32 ahip_compute_cell -- code from before this entry point -- shows from the float64 reference on the same case, over the positions
and the nine cell entries.  Measured on one MI355X, largest difference [A]:
    Cu-cubic-vcell              (86 moves, 7 rebuilds)   deviation 1.9456e-07   bar 7.7826e-07   (ahip_relax_vcell itself: 2.120e-07)
    Cu-cubic-vcell-hydrostatic  (79 moves, 5 rebuilds)   deviation 1.6392e-07   bar 6.5566e-07   (9.364e-08)
    Cu2AgO4-vcell               (30 moves, 6 rebuilds)   deviation 1.1017e-06   bar 4.4066e-06   (8.716e-07)
    CuPd-cubic-big-vcell        (30 moves, 3 rebuilds)   deviation 3.7544e-07   bar 1.5018e-06   (3.440e-07)
(two repetitions of the numpy route gave the same digits.)
"""
import os

import numpy as np
import pytest

import cell_reuse_cases as rc
import parity_cases as pc
import util
import vcell_cases as vc
from oracle import allegro_torch
from pair_allegro_amd import capi, model_file

pytestmark = pytest.mark.gpu
F64_KEYS = list(vc.GOLDEN)
F32_KEYS = ["cubic", "hydrostatic", "triclinic", "big"]
# the numpy algorithm over the float32 ahip_compute_cell against the float64 reference, largest difference of positions and cell entries [A] (docstring)
F32_DEVIATION = {"Cu-cubic-vcell": 1.9456e-07, "Cu-cubic-vcell-hydrostatic": 1.6392e-07, "Cu2AgO4-vcell": 1.1017e-06, "CuPd-cubic-big-vcell": 3.7544e-07}
_ref = {}


def golden(geom, model_dir):
    g = util.load_golden(rc.GOLDEN_OF.get(geom, geom) + "_r5")
    path, cfg, _ = util.golden_model(g, model_dir, "float32")
    _, _, sym = rc.geometry(geom)
    return path, cfg, np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)


def end_point_distance(a, b):
    return max(float(np.abs(a["positions"] - b["positions"]).max()), float(np.abs(a["cell"] - b["cell"]).max()))


def reference(hip_lib, model_dir, key, precision="float64"):
    """the numpy algorithm over a fresh ahip_compute_cell on a handle of its own; the float64 one is computed once, shared, never modified"""
    spec = vc.GOLDEN[key]
    if precision != "float64" or key not in _ref:
        path, cfg, mt = golden(spec["geom"], model_dir)
        fresh = capi.Model(path, 0, hip_lib)
        if precision == "float64":
            fresh.set_option("precision", "float64")
        ref = vc.reference(spec, lambda x, cell: fresh.compute_cell(x, mt, cell, vc.FULL, vc.SKIN), rc.largest_cutoff(fresh))
        assert fresh.last_path == "generic_f64" if precision == "float64" else fresh.last_path.startswith("fused_"), fresh.last_path
        fresh.close()
        if precision != "float64":
            return ref
        _ref[key] = ref
    return _ref[key]


@pytest.mark.parametrize("key", F64_KEYS)
def test_float64_relaxation_equals_the_numpy_algorithm(hip_lib, model_dir, key):
    spec = vc.GOLDEN[key]
    ref = reference(hip_lib, model_dir, key)
    path, cfg, mt = golden(spec["geom"], model_dir)
    assert ref["margin"] >= vc.MARGIN
    if spec["fmax"] > 0:
        assert ref["converged"] and ref["steps"] < spec["max_steps"]
    else:
        assert ref["steps"] == spec["max_steps"]
    if key == "one":
        assert ref["rebuilds"] >= 2 and ref["fmax"] < 1e-12              # no force: the cell term alone has asked for the rebuilds
    model = capi.Model(path, 0, hip_lib)
    model.set_option("precision", "float64")
    want = vc.expected_evaluations(dict(steps=ref["steps"], rebuilds=ref["rebuilds"]), ref, spec["max_steps"])
    for every in (1, 4):
        res = vc.run(model, spec, mt, check_every=every)
        assert model.last_path == "generic_f64"
        info = res["info"]
        print(f"{spec['name']}: check_every {every} {info} rows={len(res['rows'])} det D range of the reference {ref['det_range']} distance from the numpy "
              f"algorithm {end_point_distance(res, ref):.3e}")
        vc.check_run(res, ref)
        if every == 1:
            assert info["evaluations"] == want, (info, want)
        rc.check_edges(res, res["cell"], res["positions"], vc.FULL, cfg["r_max"])
    vc.check_hold(model, res, mt)
    model.close()


@pytest.mark.parametrize("key", F32_KEYS)
def test_float32_golden_models_on_the_fused_kernels(hip_lib, model_dir, key):
    spec = vc.GOLDEN[key]
    ref = reference(hip_lib, model_dir, key)
    path, cfg, mt = golden(spec["geom"], model_dir)
    model, fresh = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    fresh.set_option("precision", "float64")
    tol = pc.TOL["float32"]
    res = vc.run(model, spec, mt)
    info = res["info"]
    assert model.last_path.startswith("fused_"), model.last_path
    dx = end_point_distance(res, ref)
    want = rc.as_result(fresh, fresh.compute_cell(res["positions"], mt, res["cell"], vc.FULL, vc.SKIN))
    df = float(np.abs(res["forces"] - want["forces"]).max())
    bar = 4 * F32_DEVIATION[spec["name"]]
    print(f"{spec['name']}: path={model.last_path} {info} distance from the float64 reference {dx:.3e} (bar {bar:.3e}) max|dF| against float64 at the returned "
          f"configuration {df:.3e}")
    assert (info["steps"], info["rebuilds"], info["converged"]) == (ref["steps"], ref["rebuilds"], ref["converged"]), (info, ref["steps"], ref["rebuilds"])
    util.assert_close_to(res, want, tol, what=f"{spec['name']} at the returned configuration")
    assert df < pc.NORTH_STAR_DF, df
    assert len(res["edges"][0]) == len(want["edges"][0])
    assert dx <= bar, (dx, F32_DEVIATION[spec["name"]])

    def check(got, res):
        util.assert_close_to(got, res, tol, what="the hold against the relaxation's own result")

    vc.check_hold(model, res, mt, check=check)
    model.close(); fresh.close()


def test_float16_range_alarm(hip_lib, model_dir):
    """the case of test_gpu_relax.py::test_float16_range_alarm through ahip_relax_vcell: under fused_arith=auto the relaxation degrades to the float32 instance
    inside the call and goes on; under an explicit f16x2 it returns AHIP_ERR_STATE with x and f untouched"""
    cfg = model_file.model_S(type_names=["Cu", "Pd"], avg_num_neighbors=40.0)
    w = model_file.init_weights(cfg)
    w["l1.lat.w0"] = np.asarray(w["l1.lat.w0"]) * 1e3
    w["l1.lat.w1"] = np.asarray(w["l1.lat.w1"]) * 1e3
    path = f"{model_dir}/vcell_overflow.nequip.pth"
    allegro_torch.export_nequip_pth(path, cfg, w)
    spec = vc.GOLDEN["big"]
    cell, x0, sym = vc.start(spec)
    mt = np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)
    kw = dict(fmax=0.0, smax=0.0, max_steps=3, pressure=spec["pressure"], **spec["par"])
    os.environ["AHIP_NO_ARITH_SELFCHECK"] = "1"
    try:
        auto, f32, f16 = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
        for m in (auto, f32, f16):
            m.set_option("path", "fused")
        f32.set_option("fused_arith", "f32")
        f16.set_option("fused_arith", "f16x2")
        got = auto.relax_vcell(x0, mt, cell, vc.FULL, vc.SKIN, **kw)
        want = f32.relax_vcell(x0, mt, cell, vc.FULL, vc.SKIN, **kw)
        assert auto.last_path == f32.last_path == "fused_f32" and "float32 instance" in auto.arith_note
        assert got[5]["steps"] == want[5]["steps"] == 3 and got[5]["evaluations"] == want[5]["evaluations"] + 1
        assert np.isfinite(got[2]).all()
        np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-5)     # same instance; three moves of at most 0.2 A, float32 forces summed in another order
        np.testing.assert_allclose(got[6], want[6], rtol=0, atol=1e-5)
        x, f = x0.copy(), np.full_like(x0, 7.0)
        with pytest.raises(capi.AhipError) as e:
            f16.relax_vcell(None, mt, cell, vc.FULL, vc.SKIN, x_inout=x, f=f, **kw)
        assert e.value.code == capi.AHIP_ERR_STATE and "fused_arith=f32" in e.value.msg
        assert np.array_equal(x, x0) and np.all(f == 7.0)
        for m in (auto, f32, f16):
            m.close()
    finally:
        os.environ.pop("AHIP_NO_ARITH_SELFCHECK", None)
