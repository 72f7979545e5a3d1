"""ahip_md_cell and Calculator.md on the CPU emulation, float64: every case of md_onecall_cases through the library, NVE and Langevin, against the numpy BAOAB
over a fresh ahip_compute_cell on a second handle (steps, rebuilds, positions to 1e-9 A, velocities, every thermo row, the frames), the returned forces against
the torch oracle, check_every 1, 4 and 7, time reversal, continuation, fixed atoms, the noise, the argument errors, the degenerate inputs and the hold a success
leaves behind."""
import os

import numpy as np
import pytest

import cell_reuse_cases as rc
import md_onecall_cases as mc
import util
from oracle import allegro_torch
from pair_allegro_amd import capi, units
from pair_allegro_amd.calculator import Calculator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = mc.CASES + [mc.BIG]
RUNS = [(s, v) for s in ALL for v in mc.VARIANTS]
_oracles = {}


def _truth(c, cell, pos, pbc):
    """the torch oracle on the wrapped structure (open axes: in a cell they cannot see across)"""
    key = c["path"]
    if key not in _oracles:
        _oracles[key] = allegro_torch.build(c["cfg"], c["w"])
    big, x = rc.periodic_view(cell, pos, pbc)
    return util.oracle_run(c["cfg"], c["w"], big, x, c["types"], c["names"], oracle=_oracles[key])


def _md(model, c, spec, gamma, x, v, mass, cell, **kw):
    kw = dict(dict(nsteps=spec[3], dt=mc.DT, gamma=gamma, kT=units.KB * mc.BATH, seed=mc.SEED), **kw)
    return mc.as_result(model, model.md_cell(x, v, c["mt"], mass, cell, spec[2], mc.SKIN, **kw))


@pytest.mark.parametrize("spec,variant", RUNS, ids=[f"{s[0]}-{v[0]}" for s, v in RUNS])
def test_md_equals_the_numpy_baoab(emu_lib, model_dir, spec, variant):
    gamma = variant[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = mc.reference(spec, gamma, lambda x: fresh.compute_cell(x, c["mt"], cell, spec[2], mc.SKIN), frame_every=5)
    assert ref["margin"] >= mc.MARGIN and ref["rebuilds"] >= 3
    for every in (1, 4, 7):
        xs, vs = x0.copy(), v0.copy()
        res = _md(model, c, spec, gamma, xs, vs, mass, cell, check_every=every, frame_every=5)
        assert np.array_equal(xs, x0) and np.array_equal(vs, v0)
        assert model.last_path == "generic_f64"
        mc.check_run(res, ref)
        info = res["info"]
        if every == 1:
            assert info["evaluations"] == mc.expected_evaluations(ref), (info, ref["final_rebuilt"])
        else:
            assert mc.expected_evaluations(ref) <= info["evaluations"] <= mc.expected_evaluations(ref) + info["rebuilds"] * (every - 1), info
        rc.check_edges(res, cell, res["positions"], spec[2], c["cfg"]["r_max"])
    assert res["frames"].shape == (spec[3] // 5 + 1, len(x0), 3)
    for k, frame in enumerate(res["frames"]):
        np.testing.assert_allclose(frame, ref["path"][5 * k], rtol=0, atol=1e-9)
    rc.check_tight(res, _truth(c, cell, res["positions"], spec[2]))
    if spec[0] == mc.SLAB[0]:                 # never wrapped: the atom that left the cell keeps its continuous coordinate
        out = mc.left_cell(cell, res["positions"], spec[2])
        assert len(out) >= 1 and np.array_equal(out, mc.left_cell(cell, ref["positions"], spec[2]))
    mc.check_hold(model, res, c["mt"], cell, spec[2])
    model.close(); fresh.close()


def test_sampling_strides(emu_lib, model_dir):
    """sample_every and frame_every that do not divide the step count; no thermo buffer at all"""
    spec = mc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = mc.reference(spec, mc.GAMMA, lambda x: fresh.compute_cell(x, c["mt"], cell, spec[2], mc.SKIN), sample_every=3, frame_every=7)
    res = _md(model, c, spec, mc.GAMMA, x0, v0, mass, cell, sample_every=3, frame_every=7)
    assert res["thermo"].shape == (spec[3] // 3 + 1, 8) and res["frames"].shape == (spec[3] // 7 + 1, len(x0), 3)
    mc.check_run(res, ref)
    bare = model.md_cell(x0, v0, c["mt"], mass, cell, spec[2], mc.SKIN, want_thermo=False, want_eatom=False, nsteps=spec[3], dt=mc.DT, gamma=mc.GAMMA,
                         kT=units.KB * mc.BATH, seed=mc.SEED)
    assert bare[4] is None and bare[6] is None and bare[7] is None
    np.testing.assert_array_equal(bare[0], res["positions"])
    model.close(); fresh.close()


def test_time_reversal(emu_lib, model_dir):
    """gamma = 0: N steps, v -> -v, N steps bring the positions back"""
    for spec in (mc.CASES[1], mc.SLAB):
        c = rc.small_case(spec[1], model_dir)
        cell, x0, v0, mass, _ = mc.start(spec)
        model = capi.Model(c["path"], 0, emu_lib)
        there = _md(model, c, spec, 0.0, x0, v0, mass, cell)
        assert there["info"]["rebuilds"] >= 3 and np.abs(there["positions"] - x0).max() > 0.1
        back = _md(model, c, spec, 0.0, there["positions"], -there["velocities"], mass, cell)
        np.testing.assert_allclose(back["positions"], x0, rtol=0, atol=1e-9)
        np.testing.assert_allclose(back["velocities"], -v0, rtol=0, atol=1e-9 / mc.DT)
        model.close()


@pytest.mark.parametrize("variant", mc.VARIANTS, ids=[v[0] for v in mc.VARIANTS])
def test_continuation(emu_lib, model_dir, variant):
    """one call of a + b steps equals a call of a steps, then one of b with step0 = a"""
    spec, a = mc.CASES[1], 13
    b = spec[3] - a
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    model, other = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    whole = _md(model, c, spec, variant[1], x0, v0, mass, cell, step0=100)
    first = _md(other, c, spec, variant[1], x0, v0, mass, cell, nsteps=a, step0=100)
    second = _md(other, c, spec, variant[1], first["positions"], first["velocities"], mass, cell, nsteps=b, step0=100 + a)
    np.testing.assert_allclose(second["positions"], whole["positions"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(second["velocities"], whole["velocities"], rtol=0, atol=1e-9 / mc.DT)
    mc.check_thermo(second["thermo"][:1], first["thermo"][-1:])
    mc.check_thermo(np.concatenate([first["thermo"], second["thermo"][1:]]), whole["thermo"])
    if variant[1] > 0:                        # step0 reaches the noise
        shifted = _md(other, c, spec, variant[1], x0, v0, mass, cell, step0=101)
        assert np.abs(shifted["positions"] - whole["positions"]).max() > 1e-4
    model.close(); other.close()


@pytest.mark.parametrize("variant", mc.VARIANTS, ids=[v[0] for v in mc.VARIANTS])
def test_fixed_atoms(emu_lib, model_dir, variant):
    spec = mc.CASES[3]                        # aspirin, every third atom
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fixed = np.arange(len(x0)) % 3 == 0
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    kw = dict(gamma=variant[1], kT=units.KB * mc.BATH, seed=mc.SEED)
    compute = lambda x: fresh.compute_cell(x, c["mt"], cell, spec[2], mc.SKIN)      # noqa: E731
    ref = mc.baoab(compute, x0, v0, mass, spec[3], fixed=fixed, **kw)
    free = mc.baoab(compute, x0, v0, mass, spec[3], **kw)
    assert np.abs(ref["thermo"][:, 1] - free["thermo"][:, 1]).min() > 1e-6        # the mask matters to ke, from the first row on
    res = _md(model, c, spec, variant[1], x0, v0, mass, cell, fixed=fixed)
    assert np.array_equal(res["positions"][fixed], x0[fixed])                     # bit for bit
    assert np.all(res["velocities"][fixed] == 0.0)
    mc.check_run(res, ref)
    ke = 0.5 * units.MVV2E * float((mass[~fixed, None] * res["velocities"][~fixed] ** 2).sum())
    np.testing.assert_allclose(res["thermo"][-1, 1], ke, rtol=1e-12)
    assert np.abs(res["forces"][fixed]).min() > 0                                 # reported as the model gives them
    rc.check_tight(res, _truth(c, cell, res["positions"], spec[2]))
    model.close(); fresh.close()


def test_noise(emu_lib, model_dir):
    """the library's generator against the numpy one; moments of the numpy one over 257 x 64 (atom, step) pairs"""
    model = capi.Model(rc.small_case("Cu-cubic", model_dir)["path"], 0, emu_lib)
    for step in (0, 5, 2 ** 32 + 3, 2 ** 63 + 11):
        seed = (mc.SEED + (step << 7)) % 2 ** 64
        got = model.debug_md_noise(seed, step, 257)
        want = mc.xi(seed, 257, step)
        assert got.shape == (257, 3) and np.abs(want).max() < 8.66
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    z = np.stack([mc.xi(mc.SEED, 257, step) for step in range(64)])               # [64][257][3]
    n = z.shape[0] * z.shape[1]
    for d in range(3):
        assert abs(z[..., d].mean()) <= 5.0 / np.sqrt(n), (d, z[..., d].mean())
        assert abs(z[..., d].var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), (d, z[..., d].var())
    assert np.abs(np.corrcoef(z.reshape(-1, 3).T) - np.eye(3)).max() <= 5.0 / np.sqrt(n)
    assert not np.array_equal(mc.xi(mc.SEED, 4, 0), mc.xi(mc.SEED + 2 ** 32, 4, 0))      # the high word of the seed is part of the key
    assert model.debug_md_noise(1, 2, 0).shape == (0, 3)
    model.close()


def test_argument_errors_leave_x_v_and_the_hold(emu_lib, model_dir):
    spec = mc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    mt, pbc = c["mt"], spec[2]
    model = capi.Model(c["path"], 0, emu_lib)
    assert model.compute_cell_reuse(x0, mt, cell, pbc, mc.SKIN)[4]
    singular = np.array(cell)
    singular[2] = singular[0] + singular[1]
    nan = np.array(cell)
    nan[1, 1] = np.nan
    badtype = mt.copy()
    badtype[1] = model.num_types

    def changed(a, i, value):
        a = a.copy()
        a.flat[i] = value
        return a

    bad = [dict(cell=singular), dict(cell=nan), dict(mt=badtype), dict(skin=0.0), dict(skin=-1.0), dict(skin=np.nan), dict(nsteps=-1), dict(check_every=0),
           dict(sample_every=0), dict(frame_every=-1), dict(dt=0.0), dict(dt=-1e-3), dict(dt=np.nan), dict(dt=np.inf), dict(ftm2v=0.0), dict(ftm2v=np.inf),
           dict(mvv2e=0.0), dict(mvv2e=np.nan), dict(gamma=-1.0), dict(gamma=np.inf), dict(gamma=1.0, kT=-1e-3), dict(gamma=1.0, kT=np.nan),
           dict(mass=changed(mass, 2, 0.0)), dict(mass=changed(mass, 2, -1.0)), dict(mass=changed(mass, 2, np.inf)), dict(mass=changed(mass, 2, np.nan)),
           dict(v=changed(v0, 4, np.nan)), dict(v=changed(v0, 4, np.inf)), dict(nsteps=2 ** 31 - 1, frame_every=1), dict(params=False)]
    for kw in bad:
        a = dict(cell=cell, mt=mt, skin=mc.SKIN, mass=mass, v=v0)
        par = {k: v for k, v in kw.items() if k not in a}
        a.update({k: v for k, v in kw.items() if k in a})
        x, v, f = x0.copy(), a["v"].copy(), np.full_like(x0, 7.0)
        if par.get("nsteps") == 2 ** 31 - 1:  # more than 1 GiB of frames: the library must refuse before it touches the buffer, so a token one will do
            lib, p = emu_lib.lib, model.md_params(**par)
            D, I, C = capi.C.POINTER(capi.C.c_double), capi.C.POINTER(capi.C.c_int), capi.C
            lib.ahip_md_cell.argtypes = [C.c_void_p, C.c_int, D, D, I, D, D, I, C.c_double, I, C.POINTER(capi.MdParams), D, D, D, D, D, D, I, I]
            cc, pp, eng, token = np.ascontiguousarray(cell), np.array(pbc, dtype=np.int32), C.c_double(0), np.zeros(3)
            code = lib.ahip_md_cell(model.h, len(x), capi._p(x, C.c_double), capi._p(v, C.c_double), capi._p(mt, C.c_int), capi._p(mass, C.c_double), capi._p(cc, C.c_double),
                                    capi._p(pp, C.c_int), mc.SKIN, None, C.byref(p), capi._p(f, C.c_double), None, C.byref(eng), None, None, capi._p(token, C.c_double), None, None)
            with pytest.raises(capi.AhipError, match="fewer steps.*step0") as e:
                emu_lib.check(code)
            assert e.value.code == capi.AHIP_ERR_ARG
        else:
            with pytest.raises(capi.AhipError) as e:
                model.md_cell(None, None, a["mt"], a["mass"], a["cell"], pbc, a["skin"], x_inout=x, v_inout=v, f=f, **par)
            assert e.value.code == capi.AHIP_ERR_ARG, (kw, e.value)
        assert np.array_equal(x, x0) and np.array_equal(v, a["v"], equal_nan=True) and np.all(f == 7.0), kw
        assert not model.compute_cell_reuse(x0, mt, cell, pbc, mc.SKIN)[4], kw   # the hold is as it was
    # frames and frame_every must agree: a buffer without a stride, a stride without a buffer
    D, I, C = capi.C.POINTER(capi.C.c_double), capi.C.POINTER(capi.C.c_int), capi.C
    lib = emu_lib.lib
    lib.ahip_md_cell.argtypes = [C.c_void_p, C.c_int, D, D, I, D, D, I, C.c_double, I, C.POINTER(capi.MdParams), D, D, D, D, D, D, I, I]
    cc, pp, eng = np.ascontiguousarray(cell), np.array(pbc, dtype=np.int32), C.c_double(0)
    for every, frames in ((0, np.zeros((3, len(x0), 3))), (1, None)):
        x, v, f = x0.copy(), v0.copy(), np.full_like(x0, 7.0)
        p = model.md_params(nsteps=2, frame_every=every)
        code = lib.ahip_md_cell(model.h, len(x), capi._p(x, C.c_double), capi._p(v, C.c_double), capi._p(mt, C.c_int), capi._p(mass, C.c_double), capi._p(cc, C.c_double),
                                capi._p(pp, C.c_int), mc.SKIN, None, C.byref(p), capi._p(f, C.c_double), None, C.byref(eng), None, None, capi._p(frames, C.c_double), None, None)
        assert code == capi.AHIP_ERR_ARG and np.array_equal(x, x0) and np.array_equal(v, v0) and np.all(f == 7.0)
        assert not model.compute_cell_reuse(x0, mt, cell, pbc, mc.SKIN)[4]
    with pytest.raises(TypeError, match="unknown MD parameter"):
        model.md_cell(x0, v0, mt, mass, cell, pbc, mc.SKIN, nstep=3)
    model.close()


def test_two_coincident_atoms(emu_lib, model_dir):
    spec = mc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    x = x0.copy()
    x[1] = x[0]
    keep, v, f = x.copy(), v0.copy(), np.full_like(x, 7.0)
    model = capi.Model(c["path"], 0, emu_lib)
    with pytest.raises(capi.AhipError) as e:
        model.md_cell(None, None, c["mt"], mass, cell, spec[2], mc.SKIN, x_inout=x, v_inout=v, f=f, nsteps=5, dt=mc.DT)
    assert e.value.code == capi.AHIP_ERR_STATE and "not finite" in e.value.msg
    assert np.array_equal(x, keep) and np.array_equal(v, v0) and np.all(f == 7.0)
    assert model.compute_cell_reuse(x0, c["mt"], cell, spec[2], mc.SKIN)[4]       # a failure behind a launch ends the hold
    model.close()


def test_no_steps_returns_the_start(emu_lib, model_dir):
    spec = mc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    want = fresh.compute_cell(x0, c["mt"], cell, spec[2], mc.SKIN)
    res = _md(model, c, spec, mc.GAMMA, x0, v0, mass, cell, nsteps=0)
    assert np.array_equal(res["positions"], x0) and np.array_equal(res["velocities"], v0)
    for k, w in zip(("pe", "forces", "eatom", "virial"), want):
        np.testing.assert_array_equal(res[k], w)
    assert res["info"] == dict(steps=0, evaluations=1, rebuilds=1)
    assert res["thermo"].shape == (1, 8) and res["thermo"][0, 0] == want[0] and np.array_equal(res["thermo"][0, 2:], want[3])
    np.testing.assert_allclose(res["thermo"][0, 1], 0.5 * units.MVV2E * float((mass[:, None] * v0 ** 2).sum()), rtol=1e-13)
    model.close(); fresh.close()


def test_no_atoms_launches_nothing(emu_lib, model_dir):
    spec = mc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, _ = mc.start(spec)
    model = capi.Model(c["path"], 0, emu_lib)
    assert model.compute_cell_reuse(x0, c["mt"], cell, spec[2], mc.SKIN)[4]
    out = model.md_cell(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0), cell, spec[2], mc.SKIN, nsteps=6, dt=mc.DT, sample_every=2)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2] == 0.0 and np.all(out[5] == 0.0)
    assert out[6].shape == (4, 8) and np.all(out[6] == 0.0) and out[8] == dict(steps=6, evaluations=0, rebuilds=0)
    assert not model.compute_cell_reuse(x0, c["mt"], cell, spec[2], mc.SKIN)[4]   # no list was installed: the hold of before still serves
    model.close()


def test_calculator_md(emu_lib, model_dir):
    spec = mc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, v0, mass, sym = mc.start(spec)
    for skin in ({}, dict(skin=0.0)):
        calc = Calculator(c["path"], lib=emu_lib, **skin)
        with pytest.raises(ValueError, match="skin > 0"):
            calc.md(cell, x0, c["symbols"], steps=2, temperature=300.0)
        calc.close()
    calc = Calculator(c["path"], lib=emu_lib, skin=mc.SKIN, reuse=True)
    model = capi.Model(c["path"], 0, emu_lib)
    fixed = np.arange(len(x0)) == 2
    out = calc.md(cell, x0, c["symbols"], spec[2], steps=spec[3], dt=mc.DT, velocities=v0, temperature=mc.BATH, friction=mc.GAMMA, seed=mc.SEED, step0=7, fixed=fixed,
                  sample_every=4, frame_every=8, check_every=3)
    want = _md(model, c, spec, mc.GAMMA, x0, v0, mass, cell, step0=7, fixed=fixed, sample_every=4, frame_every=8, check_every=3)
    assert set(out) == {"energy", "forces", "atomic_energy", "virial", "stress", "positions", "velocities", "thermo", "frames", "info"}
    assert {"steps", "evaluations", "rebuilds", "path", "nghost", "nedges", "row_atom"} <= set(out["info"])
    assert {k: out["info"][k] for k in want["info"]} == want["info"] and out["info"]["steps"] == spec[3]
    for k in ("positions", "velocities", "forces", "frames"):
        np.testing.assert_array_equal(out[k], want[k])
    th = out["thermo"]
    assert set(th) == {"step", "pe", "ke", "temperature", "virial"}
    assert np.array_equal(th["step"], 7 + 4 * np.arange(spec[3] // 4 + 1))
    assert np.array_equal(th["pe"], want["thermo"][:, 0]) and np.array_equal(th["ke"], want["thermo"][:, 1]) and np.array_equal(th["virial"], want["thermo"][:, 2:])
    np.testing.assert_allclose(th["temperature"], 2.0 * th["ke"] / (3.0 * (len(x0) - 1) * units.KB), rtol=1e-14)
    assert out["energy"] == th["pe"][-1]
    again = calc.compute(cell, out["positions"], c["symbols"], spec[2])
    assert not again["info"]["rebuilt"]       # a reuse=True calculator goes on from the hold of the run
    # the drawn start: Maxwell-Boltzmann at `temperature` from `seed`, zero total momentum; the temperature column of row 0 is that of the draw
    nve = calc.md(cell, x0, c["symbols"], spec[2], steps=0, temperature=500.0, seed=3)
    drawn = units.maxwell_boltzmann(len(x0), mass, 500.0, 3)
    np.testing.assert_array_equal(nve["velocities"], drawn)
    np.testing.assert_allclose((mass[:, None] * nve["velocities"]).sum(axis=0), 0.0, atol=1e-9)
    np.testing.assert_allclose(nve["thermo"]["temperature"][0], units.MVV2E * float((mass[:, None] * drawn ** 2).sum()) / (3.0 * len(x0) * units.KB), rtol=1e-12)
    # masses: the table, the override, the unknown symbol
    assert np.array_equal(mass, [units.ATOMIC_WEIGHTS[s] for s in sym])
    heavy = calc.md(cell, x0, c["symbols"], spec[2], steps=4, dt=mc.DT, velocities=v0, masses={"O": 160.0})
    byhand = model.md_cell(x0, v0, c["mt"], np.where(np.array(sym) == "O", 160.0, mass), cell, spec[2], mc.SKIN, nsteps=4, dt=mc.DT)
    np.testing.assert_array_equal(heavy["positions"], byhand[0])
    assert np.abs(heavy["positions"] - calc.md(cell, x0, c["symbols"], spec[2], steps=4, dt=mc.DT, velocities=v0)["positions"]).max() > 1e-6
    with pytest.raises(ValueError, match="Xx"):
        units.masses_of(["Cu", "Xx"])
    assert units.masses_of(["Cu", "Xx"], {"Xx": 12.5})[1] == 12.5
    with pytest.raises(ValueError, match="needs a temperature"):
        calc.md(cell, x0, c["symbols"], spec[2], steps=2, velocities=v0, friction=1.0)
    with pytest.raises(ValueError, match="temperature to draw"):
        calc.md(cell, x0, c["symbols"], spec[2], steps=2)
    with pytest.raises(ValueError, match="differ in length"):
        calc.md(cell, x0, c["symbols"], spec[2], steps=2, velocities=v0[:-1])
    with pytest.raises(ValueError, match="not among the model's types"):
        calc.md(cell, x0, ["Xx"] * len(x0), spec[2], steps=2, temperature=300.0)
    calc.close(); model.close()


def test_units_module_needs_no_torch():
    """the constants moved out of md.py unchanged, and md.py still offers them"""
    import subprocess
    import sys
    code = "import sys; import pair_allegro_amd.units as u; assert 'torch' not in sys.modules; print(u.FTM2V, u.MVV2E, u.KB)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout.split()
    assert [float(v) for v in out] == [1.0 / 1.0364269e-4, 1.0364269e-4, 8.617343e-5]
    from pair_allegro_amd import md
    assert (md.FTM2V, md.MVV2E, md.KB, md.maxwell_boltzmann) == (units.FTM2V, units.MVV2E, units.KB, units.maxwell_boltzmann)
