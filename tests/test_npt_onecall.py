"""ahip_npt_cell and Calculator.md(pressure=...) on the CPU emulation, float64: every case of npt_cases through the library, the deterministic (Berendsen-limit)
barostat over velocity Verlet and the stochastic one over Langevin BAOAB, against the numpy reference over a fresh ahip_compute_cell on a second handle (steps,
rebuilds, positions and the nine cell entries to 1e-9 A, velocities, every thermo row, the frames and their cells), the returned forces against the torch oracle
in the returned cell, check_every 1, 4 and 7, continuation, the barostat's noise, fixed atoms, the fixed-cell limit, the argument errors and the hold a success
leaves behind."""
import numpy as np
import pytest

import cell_reuse_cases as rc
import md_onecall_cases as mc
import npt_cases as nc
import util
from oracle import allegro_torch
from pair_allegro_amd import capi, units
from pair_allegro_amd.calculator import Calculator

RUNS = [(k, v) for k in nc.SMALL for v in nc.VARIANTS]
_oracles = {}


def _truth(c, cell, pos):
    """the torch oracle on the wrapped structure"""
    key = c["path"]
    if key not in _oracles:
        _oracles[key] = allegro_torch.build(c["cfg"], c["w"])
    big, x = rc.periodic_view(cell, pos, nc.FULL)
    return util.oracle_run(c["cfg"], c["w"], big, x, c["types"], c["names"], oracle=_oracles[key])


def _compute(fresh, c):
    return lambda x, cell: fresh.compute_cell(x, c["mt"], cell, nc.FULL, nc.SKIN)


@pytest.mark.parametrize("key,variant", RUNS, ids=[f"{nc.SMALL[k]['name']}-{v[0]}" for k, v in RUNS])
def test_npt_equals_the_numpy_reference(emu_lib, model_dir, key, variant):
    cs = nc.SMALL[key]
    spec = cs["spec"]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = nc.reference(cs, variant, _compute(fresh, c), rc.largest_cutoff(fresh), frame_every=5)
    want = nc.expected_evaluations(ref)
    for every in (1, 4, 7):
        xs, vs, cs_in = x0.copy(), v0.copy(), cell.copy()
        res = nc.run(model, cs, variant, c["mt"], x=xs, v=vs, cell=cs_in, check_every=every, frame_every=5)
        assert np.array_equal(xs, x0) and np.array_equal(vs, v0) and np.array_equal(cs_in, cell)
        assert model.last_path == "generic_f64"
        nc.check_run(res, ref)
        info = res["info"]
        if every == 1:
            assert info["evaluations"] == want, (info, ref["final_rebuilt"])
        else:
            assert want <= info["evaluations"] <= want + info["rebuilds"] * (every - 1), info
        rc.check_edges(res, res["cell"], res["positions"], nc.FULL, c["cfg"]["r_max"])
    assert res["frames"].shape == (cs["steps"] // 5 + 1, len(x0), 3) and res["frame_cells"].shape == (cs["steps"] // 5 + 1, 3, 3)
    for k in range(len(res["frames"])):
        np.testing.assert_allclose(res["frames"][k], ref["path"][5 * k], rtol=0, atol=1e-9)
        np.testing.assert_allclose(res["frame_cells"][k], ref["cells"][5 * k], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res["thermo"][:, 8], [abs(np.linalg.det(a)) for a in ref["cells"]], rtol=1e-10)
    rc.check_tight(res, _truth(c, res["cell"], res["positions"]))
    nc.check_hold(model, res, c["mt"])
    model.close(); fresh.close()


@pytest.mark.parametrize("variant", nc.VARIANTS, ids=[v[0] for v in nc.VARIANTS])
def test_continuation(emu_lib, model_dir, variant):
    """32 steps cut into 13 + 19 with x, v, cell and step0 carried"""
    cs, a = nc.SMALL["triclinic"], 13
    c = rc.small_case(cs["spec"][1], model_dir)
    model, other = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    whole = nc.run(model, cs, variant, c["mt"], step0=100)
    first = nc.run(other, cs, variant, c["mt"], nsteps=a, step0=100)
    second = nc.run(other, cs, variant, c["mt"], x=first["positions"], v=first["velocities"], cell=first["cell"], nsteps=cs["steps"] - a, step0=100 + a)
    np.testing.assert_allclose(second["positions"], whole["positions"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(second["cell"], whole["cell"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(second["velocities"], whole["velocities"], rtol=0, atol=1e-9 / nc.DT)
    nc.check_thermo(second["thermo"][:1], first["thermo"][-1:])
    nc.check_thermo(np.concatenate([first["thermo"], second["thermo"][1:]]), whole["thermo"])
    if variant[2] > 0:                        # step0 reaches the barostat's noise
        shifted = nc.run(other, cs, variant, c["mt"], step0=101)
        assert np.abs(shifted["cell"] - whole["cell"]).max() > 1e-5
    model.close(); other.close()


def test_barostat_noise(emu_lib, model_dir):
    """the library's xi_V against the numpy Philox; it is no atom's noise; moments over 4096 steps of the numpy one"""
    model = capi.Model(rc.small_case("Cu-cubic", model_dir)["path"], 0, emu_lib)
    for step in (0, 5, 2 ** 32 + 3, 2 ** 63 + 11):
        seed = (nc.SEED + (step << 7)) % 2 ** 64
        got, want = model.debug_npt_noise(seed, step), nc.xi_v(seed, step)
        assert abs(want) < 8.66 and abs(got - want) <= 1e-12, (step, got, want)
        assert np.abs(mc.xi(seed, 257, step)[:, 0] - want).min() > 0
    z = np.array([nc.xi_v(nc.SEED, step) for step in range(4096)])
    assert abs(z.mean()) <= 5.0 / np.sqrt(len(z)) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / len(z))
    assert nc.xi_v(nc.SEED, 3) != nc.xi_v(nc.SEED + 2 ** 32, 3)                   # the high word of the seed is part of the key
    model.close()


@pytest.mark.parametrize("variant", nc.VARIANTS, ids=[v[0] for v in nc.VARIANTS])
def test_fixed_atoms(emu_lib, model_dir, variant):
    """a fixed atom follows the cell affinely: its reduced coordinates never change, its velocity is 0 and it is left out of ke"""
    cs = nc.SMALL["triclinic"]
    spec = cs["spec"]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fixed = np.arange(len(x0)) % 3 == 0
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    kw = dict(gamma=variant[1], kT=variant[2], seed=cs["seed"])
    ref = nc.npt(_compute(fresh, c), cell, x0, v0, mass, cs["steps"], rc.largest_cutoff(fresh), cs["p0"], fixed=fixed, **kw)
    res = nc.run(model, cs, variant, c["mt"], fixed=fixed)
    assert np.abs(res["cell"] - cell).max() > 1e-3
    np.testing.assert_allclose(res["positions"][fixed] @ np.linalg.inv(res["cell"]), x0[fixed] @ np.linalg.inv(cell), rtol=0, atol=1e-12)
    assert np.all(res["velocities"][fixed] == 0.0)
    nc.check_run(res, ref)
    ke = 0.5 * units.MVV2E * float((mass[~fixed, None] * res["velocities"][~fixed] ** 2).sum())
    np.testing.assert_allclose(res["thermo"][-1, 1], ke, rtol=1e-12)
    assert res["thermo"][0, 1] < 0.5 * units.MVV2E * float((mass[:, None] * v0 ** 2).sum()) * (1 - 1e-6)      # the mask matters to ke, from the first row on
    rc.check_tight(res, _truth(c, res["cell"], res["positions"]))
    model.close(); fresh.close()


def test_fixed_cell_limit(emu_lib, model_dir):
    """a tau_p so large that |mu - 1| < 1e-13 per step, kT = 0: the trajectory of ahip_md_cell"""
    cs = nc.SMALL["triclinic"]
    spec = cs["spec"]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    model, other = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    for gamma in (0.0, nc.GAMMA):
        # Langevin particles need a kT; the barostat's share of it is scaled away with tau_p: sqrt(2 kT beta dt / (V tau_p)) < 1e-13 as well
        kT, tau = (0.0, 1e12) if gamma == 0.0 else (units.KB * nc.BATH, 1e24)
        res = nc.run(model, cs, ("limit", gamma, kT), c["mt"], tau_p=tau)
        assert np.abs(res["cell"] - cell).max() < 1e-13 * cs["steps"] * np.abs(cell).max()
        assert np.abs(res["thermo"][1:, 8] / res["thermo"][:-1, 8] - 1.0).max() < 3e-13
        md = mc.as_result(other, other.md_cell(x0, v0, c["mt"], mass, cell, nc.FULL, nc.SKIN, nsteps=cs["steps"], dt=nc.DT, gamma=gamma, kT=kT, seed=cs["seed"]))
        assert res["info"]["rebuilds"] == md["info"]["rebuilds"] >= 3
        np.testing.assert_allclose(res["positions"], md["positions"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(res["velocities"], md["velocities"], rtol=0, atol=1e-9 / nc.DT)
        mc.check_thermo(res["thermo"][:, :8], md["thermo"])
    model.close(); other.close()


def test_argument_errors_leave_x_v_cell_out_and_the_hold(emu_lib, model_dir):
    cs = nc.SMALL["triclinic"]
    spec = cs["spec"]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    mt = c["mt"]
    model = capi.Model(c["path"], 0, emu_lib)
    assert model.compute_cell_reuse(x0, mt, cell, nc.FULL, nc.SKIN)[4]
    singular = np.array(cell)
    singular[2] = singular[0] + singular[1]

    def changed(a, i, value):
        a = a.copy()
        a.flat[i] = value
        return a

    good = dict(nsteps=3, dt=nc.DT, pressure=cs["p0"], compressibility=nc.BETA, tau_p=nc.TAU_P)
    bad = [dict(pbc=(1, 1, 0)), dict(pbc=(0, 1, 1)), dict(pbc=(0, 0, 0)), dict(cell_out=False), dict(cell=singular), dict(skin=0.0), dict(params=False),
           dict(pressure=np.nan), dict(pressure=np.inf), dict(compressibility=0.0), dict(compressibility=-1.0), dict(compressibility=np.nan),
           dict(compressibility=np.inf), dict(tau_p=0.0), dict(tau_p=-0.1), dict(tau_p=np.nan), dict(tau_p=np.inf),
           dict(kT=-1e-3), dict(kT=np.nan), dict(gamma=1.0, kT=-1e-3), dict(gamma=-1.0), dict(nsteps=-1), dict(check_every=0), dict(sample_every=0),
           dict(frame_every=-1), dict(dt=0.0), dict(dt=np.nan), dict(ftm2v=0.0), dict(mvv2e=np.inf), dict(mass=changed(mass, 2, 0.0)),
           dict(v=changed(v0, 4, np.nan))]
    for kw in bad:
        a = dict(cell=cell, skin=nc.SKIN, mass=mass, v=v0, pbc=nc.FULL, cell_out=np.full((3, 3), 5.0))
        par = dict(good, **{k: v for k, v in kw.items() if k not in a})
        a.update({k: v for k, v in kw.items() if k in a})
        if par.get("params") is False:
            par = dict(params=False)
        x, v, f = x0.copy(), a["v"].copy(), np.full_like(x0, 7.0)
        with pytest.raises(capi.AhipError) as e:
            model.npt_cell(None, None, mt, a["mass"], a["cell"], a["pbc"], a["skin"], x_inout=x, v_inout=v, f=f, cell_out=a["cell_out"], **par)
        assert e.value.code == capi.AHIP_ERR_ARG, (kw, e.value)
        assert np.array_equal(x, x0) and np.array_equal(v, a["v"], equal_nan=True) and np.all(f == 7.0), kw
        assert a["cell_out"] is False or np.all(a["cell_out"] == 5.0), kw
        assert not model.compute_cell_reuse(x0, mt, cell, nc.FULL, nc.SKIN)[4], kw   # the hold is as it was
    # no atoms
    with pytest.raises(capi.AhipError) as e:
        model.npt_cell(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0), cell, nc.FULL, nc.SKIN, **good)
    assert e.value.code == capi.AHIP_ERR_ARG
    assert not model.compute_cell_reuse(x0, mt, cell, nc.FULL, nc.SKIN)[4]
    # frame_cells without a stride is refused; frames with a stride may go without frame_cells
    C = capi.C
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib = emu_lib.lib
    lib.ahip_npt_cell.argtypes = [C.c_void_p, C.c_int, D, D, I, D, D, I, C.c_double, I, C.POINTER(capi.NptParams), D, D, D, D, D, D, D, D, I, I]
    cc, pp, eng = np.ascontiguousarray(cell), np.array(nc.FULL, dtype=np.int32), C.c_double(0)
    x, v, f, co = x0.copy(), v0.copy(), np.full_like(x0, 7.0), np.full((3, 3), 5.0)
    p = model.npt_params(**dict(good, frame_every=0))
    code = lib.ahip_npt_cell(model.h, len(x), capi._p(x, C.c_double), capi._p(v, C.c_double), capi._p(mt, C.c_int), capi._p(mass, C.c_double), capi._p(cc, C.c_double),
                             capi._p(pp, C.c_int), nc.SKIN, None, C.byref(p), capi._p(co, C.c_double), capi._p(f, C.c_double), None, C.byref(eng), None, None, None,
                             capi._p(np.zeros((4, 9)), C.c_double), None, None)
    assert code == capi.AHIP_ERR_ARG and np.array_equal(x, x0) and np.array_equal(v, v0) and np.all(f == 7.0) and np.all(co == 5.0)
    assert not model.compute_cell_reuse(x0, mt, cell, nc.FULL, nc.SKIN)[4]
    out = model.npt_cell(x0, v0, mt, mass, cell, nc.FULL, nc.SKIN, want_frame_cells=False, **dict(good, frame_every=1))
    assert out[7].shape == (4, len(x0), 3) and out[10] is None
    with pytest.raises(TypeError, match="unknown NPT parameter"):
        model.npt_cell(x0, v0, mt, mass, cell, nc.FULL, nc.SKIN, taup=3.0)
    model.close()


def test_calculator_md_at_a_pressure(emu_lib, model_dir):
    cs = nc.SMALL["triclinic"]
    spec = cs["spec"]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    calc = Calculator(c["path"], lib=emu_lib, skin=nc.SKIN, reuse=True)
    model = capi.Model(c["path"], 0, emu_lib)
    common = dict(steps=cs["steps"], dt=nc.DT, velocities=v0, temperature=nc.BATH, friction=nc.GAMMA, seed=cs["seed"], step0=7, sample_every=4, frame_every=8, check_every=3)
    out = calc.md(cell, x0, c["symbols"], nc.FULL, pressure=cs["p0"], compressibility=nc.BETA, tau_p=nc.TAU_P, **common)
    want = nc.run(model, cs, nc.VARIANTS[1], c["mt"], step0=7, sample_every=4, frame_every=8, check_every=3)
    plain = calc.md(cell, x0, c["symbols"], nc.FULL, **common)
    assert set(plain) == {"energy", "forces", "atomic_energy", "virial", "stress", "positions", "velocities", "thermo", "frames", "info"}
    assert set(plain["thermo"]) == {"step", "pe", "ke", "temperature", "virial"}
    assert set(out) == set(plain) | {"cell", "frame_cells"} and set(out["thermo"]) == set(plain["thermo"]) | {"volume", "pressure"}
    assert {k: out["info"][k] for k in want["info"]} == want["info"]
    for k in ("positions", "velocities", "forces", "frames", "cell", "frame_cells"):
        np.testing.assert_array_equal(out[k], want[k])
    th = out["thermo"]
    assert np.array_equal(th["volume"], want["thermo"][:, 8]) and np.array_equal(th["pressure"], want["thermo"][:, 9]) and np.array_equal(th["virial"], want["thermo"][:, 2:8])
    np.testing.assert_allclose(th["volume"][-1], abs(np.linalg.det(out["cell"])), rtol=1e-12)
    assert abs(th["volume"][-1] / th["volume"][0] - 1.0) > 1e-3
    vir = out["virial"]
    vm = np.array([[vir[0], vir[3], vir[4]], [vir[3], vir[1], vir[5]], [vir[4], vir[5], vir[2]]])
    np.testing.assert_allclose(out["stress"], -vm / abs(np.linalg.det(out["cell"])), rtol=1e-14)
    np.testing.assert_allclose(th["pressure"][-1], (2.0 * th["ke"][-1] - np.trace(out["stress"]) * th["volume"][-1]) / (3.0 * th["volume"][-1]), rtol=1e-10)
    # the deterministic barostat needs no temperature once the velocities are given
    det = calc.md(cell, x0, c["symbols"], nc.FULL, steps=4, dt=nc.DT, velocities=v0, pressure=cs["p0"], compressibility=nc.BETA, tau_p=nc.TAU_P)
    byhand = model.npt_cell(x0, v0, c["mt"], mass, cell, nc.FULL, nc.SKIN, nsteps=4, dt=nc.DT, pressure=cs["p0"], compressibility=nc.BETA, tau_p=nc.TAU_P)
    np.testing.assert_array_equal(det["positions"], byhand[0])
    np.testing.assert_array_equal(det["cell"], byhand[9])
    assert det["frame_cells"] is None and det["frames"] is None
    again = calc.compute(det["cell"], det["positions"], c["symbols"], nc.FULL)
    assert not again["info"]["rebuilt"]       # a reuse=True calculator goes on from the hold of the run
    with pytest.raises(ValueError, match="all three axes periodic"):
        calc.md(cell, x0, c["symbols"], (1, 1, 0), steps=2, velocities=v0, pressure=0.1, compressibility=nc.BETA, tau_p=nc.TAU_P)
    with pytest.raises(ValueError, match="compressibility and tau_p"):
        calc.md(cell, x0, c["symbols"], nc.FULL, steps=2, velocities=v0, pressure=0.1, tau_p=nc.TAU_P)
    with pytest.raises(ValueError, match="compressibility and tau_p"):
        calc.md(cell, x0, c["symbols"], nc.FULL, steps=2, velocities=v0, pressure=0.1, compressibility=nc.BETA)
    assert not calc.compute(det["cell"], det["positions"], c["symbols"], nc.FULL)["info"]["rebuilt"]      # raised before any call
    calc.close(); model.close()
