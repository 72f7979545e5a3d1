"""GPU: ahip_npt_cell.  The three NPT kernels (csrc/neigh.hip: k_npt_gather, k_npt_decide, k_npt_move), the barostat's noise and the host loop in float64 against
the numpy reference of npt_cases over a fresh ahip_compute_cell on a second handle, the deterministic barostat over velocity Verlet and the stochastic one over
Langevin BAOAB, on the cases of the CPU tests plus 257 atoms (a block boundary and a partial wave in the row kernels) and a cell of one atom (the cell term alone
decides its rebuilds); then the float32 golden models on the fused kernels against that float64 reference.

The end point of a float32 run cannot match the float64 reference to 1e-9 A: its forces and its virial differ in the fifth digit and integrator and barostat
carry that along.  The bar is four times the deviation that the numpy route over the float32 ahip_compute_cell -- code from before ahip_npt_cell -- shows from the
float64 reference on the same case (the factor covers the accumulation order of the fused kernels, as in test_gpu_md_onecall.py).  Measured on one MI355X,
largest difference of a coordinate or a cell entry [A]:
    Cu-cubic-npt-berendsen         (32 steps)   deviation 4.3275e-08   bar 1.7310e-07
    Cu-cubic-npt-npt               (32 steps)   deviation 5.3594e-08   bar 2.1438e-07
    Cu2AgO4-npt-berendsen          (32 steps)   deviation 1.8868e-07   bar 7.5472e-07
    Cu2AgO4-npt-npt                (32 steps)   deviation 1.2662e-07   bar 5.0648e-07
    CuPd-cubic-big-npt-berendsen   (24 steps)   deviation 2.9798e-08   bar 1.1919e-07
    CuPd-cubic-big-npt-npt         (24 steps)   deviation 3.1317e-08   bar 1.2527e-07
(two repetitions of the numpy route gave the same digits: ahip_compute_cell builds rows and list afresh in the same order every time.)
"""
import numpy as np
import pytest

import cell_reuse_cases as rc
import md_onecall_cases as mc
import npt_cases as nc
import parity_cases as pc
import util
from pair_allegro_amd import capi

pytestmark = pytest.mark.gpu
F64_RUNS = [(k, v) for k in nc.GOLDEN for v in nc.VARIANTS]
F32_RUNS = [(k, v) for k in ("cubic", "triclinic", "big") for v in nc.VARIANTS]
# the numpy route over the float32 ahip_compute_cell against the float64 reference, largest difference of a coordinate or a cell entry at the end [A] (docstring)
F32_DEVIATION = {
    "Cu-cubic-npt-berendsen": 4.3275e-08,
    "Cu-cubic-npt-npt": 5.3594e-08,
    "Cu2AgO4-npt-berendsen": 1.8868e-07,
    "Cu2AgO4-npt-npt": 1.2662e-07,
    "CuPd-cubic-big-npt-berendsen": 2.9798e-08,
    "CuPd-cubic-big-npt-npt": 3.1317e-08,
}
_ref = {}


def _ids(runs):
    return [f"{nc.GOLDEN[k]['name']}-{v[0]}" for k, v in runs]


def _golden(geom, model_dir):
    g = util.load_golden(rc.GOLDEN_OF.get(geom, geom) + "_r5")
    path, cfg, _ = util.golden_model(g, model_dir, "float32")
    _, _, sym = rc.geometry(geom)
    return path, cfg, np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)


def _reference(hip_lib, model_dir, key, variant):
    """the numpy reference over a fresh float64 ahip_compute_cell on a handle of its own: computed once, shared, never modified"""
    if (key, variant[0]) not in _ref:
        cs = nc.GOLDEN[key]
        path, cfg, mt = _golden(cs["spec"][1], model_dir)
        fresh = capi.Model(path, 0, hip_lib)
        fresh.set_option("precision", "float64")
        ref = nc.reference(cs, variant, lambda x, cell: fresh.compute_cell(x, mt, cell, nc.FULL, nc.SKIN), rc.largest_cutoff(fresh), frame_every=5)
        assert fresh.last_path == "generic_f64"
        fresh.close()
        _ref[(key, variant[0])] = ref
    return _ref[(key, variant[0])]


@pytest.mark.parametrize("key,variant", F64_RUNS, ids=_ids(F64_RUNS))
def test_float64_npt_equals_the_numpy_reference(hip_lib, model_dir, key, variant):
    cs = nc.GOLDEN[key]
    ref = _reference(hip_lib, model_dir, key, variant)
    path, cfg, mt = _golden(cs["spec"][1], model_dir)
    model = capi.Model(path, 0, hip_lib)
    model.set_option("precision", "float64")
    for every in (1, 4):
        res = nc.run(model, cs, variant, mt, check_every=every, frame_every=5)
        assert model.last_path == "generic_f64"
        info = res["info"]
        print(f"{cs['name']} {variant[0]}: check_every {every} {info} rows={len(res['rows'])} margin {ref['margin']:.2e} V/V0 {ref['v_range'][0]:.4f} .. {ref['v_range'][1]:.4f} "
              f"max|dx| against the numpy reference {np.abs(res['positions'] - ref['positions']).max():.3e} max|dcell| {np.abs(res['cell'] - ref['cell']).max():.3e} "
              f"max|dv| {np.abs(res['velocities'] - ref['velocities']).max():.3e}")
        nc.check_run(res, ref)
        if every == 1:
            assert info["evaluations"] == nc.expected_evaluations(ref), (info, ref["final_rebuilt"])
        rc.check_edges(res, res["cell"], res["positions"], nc.FULL, cfg["r_max"])
    for k in range(len(res["frames"])):
        np.testing.assert_allclose(res["frames"][k], ref["path"][5 * k], rtol=0, atol=1e-9)
        np.testing.assert_allclose(res["frame_cells"][k], ref["cells"][5 * k], rtol=0, atol=1e-9)
    nc.check_hold(model, res, mt)
    model.close()


def test_barostat_noise_on_the_device(hip_lib, model_dir):
    model = capi.Model(_golden("Cu-cubic", model_dir)[0], 0, hip_lib)
    for step in (0, 5, 2 ** 32 + 3, 2 ** 63 + 11):
        seed = (nc.SEED + (step << 7)) % 2 ** 64
        got, want = model.debug_npt_noise(seed, step), nc.xi_v(seed, step)
        print(f"step {step}: |xi_V - numpy| {abs(got - want):.3e}")
        assert abs(got - want) <= 1e-12
    model.close()


@pytest.mark.parametrize("variant", nc.VARIANTS, ids=[v[0] for v in nc.VARIANTS])
def test_continuation(hip_lib, model_dir, variant):
    """32 steps cut into 13 + 19 with x, v, cell and step0 carried"""
    cs, a = nc.GOLDEN["triclinic"], 13
    path, cfg, mt = _golden(cs["spec"][1], model_dir)
    model, other = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    for m in (model, other):
        m.set_option("precision", "float64")
    whole = nc.run(model, cs, variant, mt, step0=100)
    first = nc.run(other, cs, variant, mt, nsteps=a, step0=100)
    second = nc.run(other, cs, variant, mt, x=first["positions"], v=first["velocities"], cell=first["cell"], nsteps=cs["steps"] - a, step0=100 + a)
    np.testing.assert_allclose(second["positions"], whole["positions"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(second["cell"], whole["cell"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(second["velocities"], whole["velocities"], rtol=0, atol=1e-9 / nc.DT)
    nc.check_thermo(second["thermo"][:1], first["thermo"][-1:])
    nc.check_thermo(np.concatenate([first["thermo"], second["thermo"][1:]]), whole["thermo"])
    model.close(); other.close()


def test_fixed_atoms_follow_the_cell(hip_lib, model_dir):
    cs = nc.GOLDEN["block"]
    spec = cs["spec"]
    path, cfg, mt = _golden(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fixed = np.arange(len(x0)) % 3 == 0
    model = capi.Model(path, 0, hip_lib)
    model.set_option("precision", "float64")
    res = nc.run(model, cs, nc.VARIANTS[1], mt, fixed=fixed, nsteps=8)
    assert np.abs(res["cell"] - cell).max() > 1e-4
    np.testing.assert_allclose(res["positions"][fixed] @ np.linalg.inv(res["cell"]), x0[fixed] @ np.linalg.inv(cell), rtol=0, atol=1e-12)
    assert np.all(res["velocities"][fixed] == 0.0)
    rc.check_edges(res, res["cell"], res["positions"], nc.FULL, cfg["r_max"])
    model.close()


@pytest.mark.parametrize("key,variant", F32_RUNS, ids=_ids(F32_RUNS))
def test_float32_golden_models_on_the_fused_kernels(hip_lib, model_dir, key, variant):
    cs = nc.GOLDEN[key]
    ref = _reference(hip_lib, model_dir, key, variant)
    path, cfg, mt = _golden(cs["spec"][1], model_dir)
    model, fresh = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    fresh.set_option("precision", "float64")
    tol = pc.TOL["float32"]
    res = nc.run(model, cs, variant, mt)
    info = res["info"]
    assert model.last_path.startswith("fused_"), model.last_path
    dx = float(max(np.abs(res["positions"] - ref["positions"]).max(), np.abs(res["cell"] - ref["cell"]).max()))
    want = rc.as_result(fresh, fresh.compute_cell(res["positions"], mt, res["cell"], nc.FULL, nc.SKIN))
    df = float(np.abs(res["forces"] - want["forces"]).max())
    bar = 4 * F32_DEVIATION[f"{cs['name']}-{variant[0]}"]
    print(f"{cs['name']} {variant[0]}: path={model.last_path} {info} max|dx|, |dcell| against the float64 reference {dx:.3e} (bar {bar:.3e}) max|dF| against float64 at "
          f"the returned configuration {df:.3e}")
    assert (info["steps"], info["rebuilds"]) == (ref["steps"], ref["rebuilds"]), (info, ref["steps"], ref["rebuilds"])
    util.assert_close_to(res, want, tol, what=f"{cs['name']} at the returned configuration")
    assert df < pc.NORTH_STAR_DF, df
    assert len(res["edges"][0]) == len(want["edges"][0])
    assert dx <= bar, (dx, bar)

    def check(got, res):
        util.assert_close_to(got, res, tol, what="the hold against the run's own result")

    nc.check_hold(model, res, mt, check=check)
    model.close(); fresh.close()


def test_fused_arith_auto_completes_on_a_fused_path(hip_lib, model_dir):
    cs = nc.GOLDEN["big"]
    path, cfg, mt = _golden(cs["spec"][1], model_dir)
    model = capi.Model(path, 0, hip_lib)
    model.set_option("path", "fused")
    model.set_option("fused_arith", "auto")
    res = nc.run(model, cs, nc.VARIANTS[1], mt, nsteps=8)
    print(f"fused_arith=auto: path={model.last_path} {res['info']} note={model.arith_note!r}")
    assert model.last_path.startswith("fused_") and res["info"]["steps"] == 8
    assert np.isfinite(res["positions"]).all() and np.isfinite(res["cell"]).all() and np.isfinite(res["thermo"]).all()
    assert abs(res["thermo"][-1, 8] - abs(np.linalg.det(res["cell"]))) <= 1e-9 * res["thermo"][-1, 8]
    model.close()
