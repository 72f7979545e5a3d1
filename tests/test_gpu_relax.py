"""GPU: ahip_relax_cell.  The three relaxation kernels (csrc/neigh.hip: k_relax_gather, k_relax_decide, k_relax_move) and the host loop in float64 against the
numpy FIRE of relax_cases over a fresh ahip_compute_cell on a second handle, on the cases of the CPU tests plus 257 atoms for 12 moves (a block boundary and a
partial wave in the row kernels) and a cell of one atom; then the float32 golden models on the fused kernels against that float64 reference.

The end point of a float32 run cannot match the float64 reference to 1e-9 A: its forces differ by some 1e-5 eV/A and FIRE carries that along.  The bar is four
times the deviation that the numpy FIRE over the float32 ahip_compute_cell -- code from before the relaxation -- shows from the float64 reference on the same
case (the factor covers the run-to-run accumulation order of the fused kernels).  Measured on one MI355X, largest coordinate difference [A]:
    Cu-cubic-relax        (59 moves)   deviation 9.579e-08   bar 3.832e-07   (ahip_relax_cell itself: 1.152e-07)
    Cu2AgO4-relax         (30 moves)   deviation 2.641e-07   bar 1.056e-06   (1.781e-07)
    Cu2AgO4-slab-relax    (30 moves)   deviation 4.210e-06   bar 1.684e-05   (4.445e-06)
    CuPd-cubic-big-relax  (30 moves)   deviation 4.063e-07   bar 1.625e-06   (3.586e-07)
(three repetitions of the numpy route gave the same digits: ahip_compute_cell builds rows and list afresh in the same order every time.)
"""
import os

import numpy as np
import pytest

import cell_reuse_cases as rc
import parity_cases as pc
import relax_cases as xc
import util
from oracle import allegro_torch
from pair_allegro_amd import capi, model_file

pytestmark = pytest.mark.gpu
F64_SPECS = xc.CASES + [xc.BIG, xc.BLOCK, xc.ONE]
F32_SPECS = [xc.CASES[0], xc.CASES[1], xc.CASES[2], xc.BIG]
# the numpy FIRE over the float32 ahip_compute_cell against the float64 reference, largest coordinate difference of the end points [A] (docstring)
F32_DEVIATION = {"Cu-cubic-relax": 9.579e-08, "Cu2AgO4-relax": 2.6405e-07, "Cu2AgO4-slab-relax": 4.2103e-06, "CuPd-cubic-big-relax": 4.0633e-07}
_ref = {}


def _golden(geom, model_dir):
    g = util.load_golden(rc.GOLDEN_OF.get(geom, geom) + "_r5")
    path, cfg, _ = util.golden_model(g, model_dir, "float32")
    _, _, sym = rc.geometry(geom)
    return path, cfg, np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)


def _reference(hip_lib, model_dir, spec):
    """the numpy FIRE over a fresh float64 ahip_compute_cell on a handle of its own: computed once, shared, never modified"""
    if spec[0] not in _ref:
        path, cfg, mt = _golden(spec[1], model_dir)
        cell, x0, _ = xc.start(spec)
        fresh = capi.Model(path, 0, hip_lib)
        fresh.set_option("precision", "float64")
        ref = xc.reference(spec, lambda x: fresh.compute_cell(x, mt, cell, spec[2], xc.SKIN))
        assert fresh.last_path == "generic_f64"
        fresh.close()
        _ref[spec[0]] = ref
    return _ref[spec[0]]


@pytest.mark.parametrize("spec", F64_SPECS, ids=[s[0] for s in F64_SPECS])
def test_float64_relaxation_equals_the_numpy_fire(hip_lib, model_dir, spec):
    ref = _reference(hip_lib, model_dir, spec)
    path, cfg, mt = _golden(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    if spec[3] > 0:
        assert ref["converged"] and ref["steps"] < spec[4]
    else:
        assert ref["steps"] == spec[4]
    model = capi.Model(path, 0, hip_lib)
    model.set_option("precision", "float64")
    for every in (1, 4):
        res = xc.as_result(model, model.relax_cell(x0, mt, cell, spec[2], xc.SKIN, fmax=spec[3], max_steps=spec[4], check_every=every))
        assert model.last_path == "generic_f64"
        info = res["info"]
        print(f"{spec[0]}: check_every {every} {info} rows={len(res['rows'])} max|dx| against the numpy FIRE {np.abs(res['positions'] - ref['positions']).max():.3e}")
        xc.check_run(res, ref)
        if every == 1:
            assert info["evaluations"] == xc.expected_evaluations(info, spec[4]), info
        rc.check_edges(res, cell, res["positions"], spec[2], cfg["r_max"])
    if spec[0] == xc.SLAB[0]:
        assert len(xc.left_cell(cell, res["positions"], spec[2])) >= 1
    xc.check_hold(model, res, mt, cell, spec[2])
    model.close()


@pytest.mark.parametrize("spec", F32_SPECS, ids=[s[0] for s in F32_SPECS])
def test_float32_golden_models_on_the_fused_kernels(hip_lib, model_dir, spec):
    ref = _reference(hip_lib, model_dir, spec)
    path, cfg, mt = _golden(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    model, fresh = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    fresh.set_option("precision", "float64")
    tol = pc.TOL["float32"]
    res = xc.as_result(model, model.relax_cell(x0, mt, cell, spec[2], xc.SKIN, fmax=spec[3], max_steps=spec[4]))
    info = res["info"]
    assert model.last_path.startswith("fused_"), model.last_path
    dx = float(np.abs(res["positions"] - ref["positions"]).max())
    want = rc.as_result(fresh, fresh.compute_cell(res["positions"], mt, cell, spec[2], xc.SKIN))
    df = float(np.abs(res["forces"] - want["forces"]).max())
    fm = float(np.linalg.norm(want["forces"], axis=1).max())
    print(f"{spec[0]}: path={model.last_path} {info} max|dx| against the float64 reference {dx:.3e} (bar {4 * F32_DEVIATION[spec[0]]:.3e}) max|dF| against float64 "
          f"at the returned positions {df:.3e}, max|F| there {fm:.5f}")
    assert (info["steps"], info["rebuilds"], info["converged"]) == (ref["steps"], ref["rebuilds"], ref["converged"]), (info, ref["steps"], ref["rebuilds"])
    util.assert_close_to(res, want, tol, what=f"{spec[0]} at the returned positions")
    assert df < pc.NORTH_STAR_DF, df
    assert len(res["edges"][0]) == len(want["edges"][0])
    if spec[3] > 0:
        assert info["converged"] and fm <= spec[3] + pc.NORTH_STAR_DF
    assert dx <= 4 * F32_DEVIATION[spec[0]], (dx, F32_DEVIATION[spec[0]])

    def check(got, res):
        util.assert_close_to(got, res, tol, what="the hold against the relaxation's own result")

    xc.check_hold(model, res, mt, cell, spec[2], check=check)
    model.close(); fresh.close()


def test_float16_range_alarm(hip_lib, model_dir):
    """the model of test_gpu_fused.py::_blown_up_model (an activation leaves float16's range) without the first-evaluation self-check: under fused_arith=auto the
    relaxation degrades to the float32 instance inside the call and goes on; under an explicit f16x2 it returns AHIP_ERR_STATE with x and f untouched"""
    cfg = model_file.model_S(type_names=["Cu", "Pd"], avg_num_neighbors=40.0)
    w = model_file.init_weights(cfg)
    w["l1.lat.w0"] = np.asarray(w["l1.lat.w0"]) * 1e3
    w["l1.lat.w1"] = np.asarray(w["l1.lat.w1"]) * 1e3
    path = f"{model_dir}/relax_overflow.nequip.pth"
    allegro_torch.export_nequip_pth(path, cfg, w)
    cell, x0, sym = xc.start(xc.BIG)
    mt = np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)
    os.environ["AHIP_NO_ARITH_SELFCHECK"] = "1"
    try:
        auto, f32, f16 = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
        for m in (auto, f32, f16):
            m.set_option("path", "fused")
        f32.set_option("fused_arith", "f32")
        f16.set_option("fused_arith", "f16x2")
        got = auto.relax_cell(x0, mt, cell, (1, 1, 1), xc.SKIN, fmax=0.0, max_steps=3)
        want = f32.relax_cell(x0, mt, cell, (1, 1, 1), xc.SKIN, fmax=0.0, max_steps=3)
        assert auto.last_path == f32.last_path == "fused_f32" and "float32 instance" in auto.arith_note
        assert got[5]["steps"] == want[5]["steps"] == 3 and got[5]["evaluations"] == want[5]["evaluations"] + 1
        assert np.isfinite(got[2]).all()
        np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-5)     # same instance; three moves of at most 0.2 A, float32 forces summed in another order
        x, f = x0.copy(), np.full_like(x0, 7.0)
        with pytest.raises(capi.AhipError) as e:
            f16.relax_cell(None, mt, cell, (1, 1, 1), xc.SKIN, x_inout=x, f=f, fmax=0.0, max_steps=3)
        assert e.value.code == capi.AHIP_ERR_STATE and "fused_arith=f32" in e.value.msg
        assert np.array_equal(x, x0) and np.all(f == 7.0)
        for m in (auto, f32, f16):
            m.close()
    finally:
        os.environ.pop("AHIP_NO_ARITH_SELFCHECK", None)
