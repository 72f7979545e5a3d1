"""GPU: ahip_md_cell.  The three MD kernels (csrc/neigh.hip: k_md_gather, k_md_decide, k_md_move), the noise generator and the host loop in float64 against the
numpy BAOAB of md_onecall_cases over a fresh ahip_compute_cell on a second handle, NVE and Langevin, on the cases of the CPU tests plus 257 atoms (a block
boundary and a partial wave in the row kernels) and a cell of one atom; then the float32 golden models on the fused kernels against that float64 reference.

The end point of a float32 run cannot match the float64 reference to 1e-9 A: its forces differ by some 1e-5 eV/A and the integrator carries that along.  The bar
is four times the deviation that the numpy BAOAB over the float32 ahip_compute_cell -- code from before ahip_md_cell -- shows from the float64 reference on the
same case (the factor covers the run-to-run accumulation order of the fused kernels, as in test_gpu_relax.py).  Measured on one MI355X, largest coordinate
difference [A]:
    Cu-cubic-md-nve              (32 steps)   deviation 2.6648e-08   bar 1.0659e-07
    Cu-cubic-md-langevin         (32 steps)   deviation 1.9223e-08   bar 7.6892e-08
    Cu2AgO4-md-nve               (32 steps)   deviation 1.6671e-07   bar 6.6684e-07
    Cu2AgO4-md-langevin          (32 steps)   deviation 1.0275e-07   bar 4.1100e-07
    Cu2AgO4-slab-md-nve          (32 steps)   deviation 1.4787e-07   bar 5.9148e-07
    Cu2AgO4-slab-md-langevin     (32 steps)   deviation 1.3474e-07   bar 5.3896e-07
    CuPd-cubic-big-md-nve        (24 steps)   deviation 3.1226e-08   bar 1.2490e-07
    CuPd-cubic-big-md-langevin   (24 steps)   deviation 3.0371e-08   bar 1.2148e-07
(three repetitions of the numpy route gave the same digits: ahip_compute_cell builds rows and list afresh in the same order every time.)
"""
import os

import numpy as np
import pytest

import cell_reuse_cases as rc
import md_onecall_cases as mc
import parity_cases as pc
import util
from oracle import allegro_torch
from pair_allegro_amd import capi, model_file, units

pytestmark = pytest.mark.gpu
F64_SPECS = mc.CASES + [mc.BIG, mc.BLOCK, mc.ONE]
F32_SPECS = [mc.CASES[0], mc.CASES[1], mc.CASES[2], mc.BIG]
F64_RUNS = [(s, v) for s in F64_SPECS for v in mc.VARIANTS]
F32_RUNS = [(s, v) for s in F32_SPECS for v in mc.VARIANTS]
# the numpy BAOAB over the float32 ahip_compute_cell against the float64 reference, largest coordinate difference of the end points [A] (docstring)
F32_DEVIATION = {
    "Cu-cubic-md-nve": 2.6648e-08,
    "Cu-cubic-md-langevin": 1.9223e-08,
    "Cu2AgO4-md-nve": 1.6671e-07,
    "Cu2AgO4-md-langevin": 1.0275e-07,
    "Cu2AgO4-slab-md-nve": 1.4787e-07,
    "Cu2AgO4-slab-md-langevin": 1.3474e-07,
    "CuPd-cubic-big-md-nve": 3.1226e-08,
    "CuPd-cubic-big-md-langevin": 3.0371e-08,
}
_ref = {}


def _ids(runs):
    return [f"{s[0]}-{v[0]}" for s, v in runs]


def _golden(geom, model_dir):
    g = util.load_golden(rc.GOLDEN_OF.get(geom, geom) + "_r5")
    path, cfg, _ = util.golden_model(g, model_dir, "float32")
    _, _, sym = rc.geometry(geom)
    return path, cfg, np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)


def _reference(hip_lib, model_dir, spec, gamma):
    """the numpy BAOAB over a fresh float64 ahip_compute_cell on a handle of its own: computed once, shared, never modified"""
    key = (spec[0], gamma)
    if key not in _ref:
        path, cfg, mt = _golden(spec[1], model_dir)
        cell = mc.start(spec)[0]
        fresh = capi.Model(path, 0, hip_lib)
        fresh.set_option("precision", "float64")
        ref = mc.reference(spec, gamma, lambda x: fresh.compute_cell(x, mt, cell, spec[2], mc.SKIN), frame_every=5)
        assert fresh.last_path == "generic_f64"
        fresh.close()
        _ref[key] = ref
    return _ref[key]


def _md(model, mt, spec, gamma, x, v, mass, cell, **kw):
    kw = dict(dict(nsteps=spec[3], dt=mc.DT, gamma=gamma, kT=units.KB * mc.BATH, seed=mc.SEED), **kw)
    return mc.as_result(model, model.md_cell(x, v, mt, mass, cell, spec[2], mc.SKIN, **kw))


@pytest.mark.parametrize("spec,variant", F64_RUNS, ids=_ids(F64_RUNS))
def test_float64_md_equals_the_numpy_baoab(hip_lib, model_dir, spec, variant):
    gamma = variant[1]
    ref = _reference(hip_lib, model_dir, spec, gamma)
    path, cfg, mt = _golden(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    assert ref["margin"] >= mc.MARGIN
    model = capi.Model(path, 0, hip_lib)
    model.set_option("precision", "float64")
    for every in (1, 4):
        res = _md(model, mt, spec, gamma, x0, v0, mass, cell, check_every=every, frame_every=5)
        assert model.last_path == "generic_f64"
        info = res["info"]
        print(f"{spec[0]} {variant[0]}: check_every {every} {info} rows={len(res['rows'])} max|dx| against the numpy BAOAB "
              f"{np.abs(res['positions'] - ref['positions']).max():.3e} max|dv| {np.abs(res['velocities'] - ref['velocities']).max():.3e}")
        mc.check_run(res, ref)
        if every == 1:
            assert info["evaluations"] == mc.expected_evaluations(ref), (info, ref["final_rebuilt"])
        rc.check_edges(res, cell, res["positions"], spec[2], cfg["r_max"])
    for k, frame in enumerate(res["frames"]):
        np.testing.assert_allclose(frame, ref["path"][5 * k], rtol=0, atol=1e-9)
    if spec[0] == mc.SLAB[0]:
        assert len(mc.left_cell(cell, res["positions"], spec[2])) >= 1
    mc.check_hold(model, res, mt, cell, spec[2])
    model.close()


def test_noise_on_the_device(hip_lib, model_dir):
    model = capi.Model(_golden("Cu-cubic", model_dir)[0], 0, hip_lib)
    for step in (0, 5, 2 ** 32 + 3, 2 ** 63 + 11):
        seed = (mc.SEED + (step << 7)) % 2 ** 64
        got, want = model.debug_md_noise(seed, step, 257), mc.xi(seed, 257, step)
        print(f"step {step}: max|xi - numpy| {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    model.close()


@pytest.mark.parametrize("variant", mc.VARIANTS, ids=[v[0] for v in mc.VARIANTS])
def test_continuation(hip_lib, model_dir, variant):
    """one call of a + b steps equals a call of a steps, then one of b with step0 = a"""
    spec, a = mc.CASES[1], 13
    path, cfg, mt = _golden(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    model, other = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    for m in (model, other):
        m.set_option("precision", "float64")
    whole = _md(model, mt, spec, variant[1], x0, v0, mass, cell, step0=100)
    first = _md(other, mt, spec, variant[1], x0, v0, mass, cell, nsteps=a, step0=100)
    second = _md(other, mt, spec, variant[1], first["positions"], first["velocities"], mass, cell, nsteps=spec[3] - a, step0=100 + a)
    np.testing.assert_allclose(second["positions"], whole["positions"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(second["velocities"], whole["velocities"], rtol=0, atol=1e-9 / mc.DT)
    mc.check_thermo(second["thermo"][:1], first["thermo"][-1:])
    mc.check_thermo(np.concatenate([first["thermo"], second["thermo"][1:]]), whole["thermo"])
    model.close(); other.close()


@pytest.mark.parametrize("spec,variant", F32_RUNS, ids=_ids(F32_RUNS))
def test_float32_golden_models_on_the_fused_kernels(hip_lib, model_dir, spec, variant):
    gamma = variant[1]
    ref = _reference(hip_lib, model_dir, spec, gamma)
    path, cfg, mt = _golden(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    model, fresh = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    fresh.set_option("precision", "float64")
    tol = pc.TOL["float32"]
    res = _md(model, mt, spec, gamma, x0, v0, mass, cell)
    info = res["info"]
    assert model.last_path.startswith("fused_"), model.last_path
    dx = float(np.abs(res["positions"] - ref["positions"]).max())
    want = rc.as_result(fresh, fresh.compute_cell(res["positions"], mt, cell, spec[2], mc.SKIN))
    df = float(np.abs(res["forces"] - want["forces"]).max())
    bar = 4 * F32_DEVIATION[f"{spec[0]}-{variant[0]}"]
    print(f"{spec[0]} {variant[0]}: path={model.last_path} {info} max|dx| against the float64 reference {dx:.3e} (bar {bar:.3e}) max|dF| against float64 at the "
          f"returned positions {df:.3e}")
    assert (info["steps"], info["rebuilds"]) == (ref["steps"], ref["rebuilds"]), (info, ref["steps"], ref["rebuilds"])
    util.assert_close_to(res, want, tol, what=f"{spec[0]} at the returned positions")
    assert df < pc.NORTH_STAR_DF, df
    assert len(res["edges"][0]) == len(want["edges"][0])
    assert dx <= bar, (dx, bar)

    def check(got, res):
        util.assert_close_to(got, res, tol, what="the hold against the run's own result")

    mc.check_hold(model, res, mt, cell, spec[2], check=check)
    model.close(); fresh.close()


def test_float16_range_alarm(hip_lib, model_dir):
    """the model of test_gpu_fused.py::_blown_up_model (an activation leaves float16's range) without the first-evaluation self-check: under fused_arith=auto the
    run degrades to the float32 instance inside the call and goes on; under an explicit f16x2 it returns AHIP_ERR_STATE with x, v and f untouched"""
    cfg = model_file.model_S(type_names=["Cu", "Pd"], avg_num_neighbors=40.0)
    w = model_file.init_weights(cfg)
    w["l1.lat.w0"] = np.asarray(w["l1.lat.w0"]) * 1e3
    w["l1.lat.w1"] = np.asarray(w["l1.lat.w1"]) * 1e3
    path = f"{model_dir}/md_overflow.nequip.pth"
    allegro_torch.export_nequip_pth(path, cfg, w)
    cell, x0, v0, mass, sym = mc.start(mc.BIG)
    mt = np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)
    kw = dict(nsteps=3, dt=mc.DT, gamma=mc.GAMMA, kT=units.KB * mc.BATH, seed=mc.SEED)
    os.environ["AHIP_NO_ARITH_SELFCHECK"] = "1"
    try:
        auto, f32, f16 = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
        for m in (auto, f32, f16):
            m.set_option("path", "fused")
        f32.set_option("fused_arith", "f32")
        f16.set_option("fused_arith", "f16x2")
        got = auto.md_cell(x0, v0, mt, mass, cell, (1, 1, 1), mc.SKIN, **kw)
        want = f32.md_cell(x0, v0, mt, mass, cell, (1, 1, 1), mc.SKIN, **kw)
        assert auto.last_path == f32.last_path == "fused_f32" and "float32 instance" in auto.arith_note
        assert got[8]["steps"] == want[8]["steps"] == 3 and got[8]["evaluations"] == want[8]["evaluations"] + 1
        assert np.isfinite(got[3]).all() and np.isfinite(got[6]).all()
        np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-5)     # same instance; three steps, float32 forces summed in another order
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-5 / mc.DT)
        x, v, f = x0.copy(), v0.copy(), np.full_like(x0, 7.0)
        with pytest.raises(capi.AhipError) as e:
            f16.md_cell(None, None, mt, mass, cell, (1, 1, 1), mc.SKIN, x_inout=x, v_inout=v, f=f, **kw)
        assert e.value.code == capi.AHIP_ERR_STATE and "fused_arith=f32" in e.value.msg
        assert np.array_equal(x, x0) and np.array_equal(v, v0) and np.all(f == 7.0)
        for m in (auto, f32, f16):
            m.close()
    finally:
        os.environ.pop("AHIP_NO_ARITH_SELFCHECK", None)
