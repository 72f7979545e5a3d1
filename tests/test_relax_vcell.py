"""ahip_relax_vcell and Calculator.relax(variable_cell=True) on the CPU emulation, float64: the cases of vcell_cases.SMALL through the library against the numpy
statement of the algorithm over a fresh ahip_compute_cell on a second handle (moves, rebuilds, convergence, positions and cell to 1e-9 A), the returned
energy, forces and virial against the torch oracle in the returned cell, check_every 1, 4 and 7, the sign and index conventions of the strain force against
central differences of the library's own energy, the strain mask, fixed atoms, the argument errors, a cell that would invert, and the hold a success leaves."""
import numpy as np
import pytest

import cell_reuse_cases as rc
import relax_cases as xc
import util
import vcell_cases as vc
from oracle import allegro_torch
from pair_allegro_amd import capi
from pair_allegro_amd.calculator import Calculator

FD_ORACLE = 3.336e-9    # eV: tests/test_calculator.py, central differences at h = 1e-5 against autograd on the torch oracle alone; the bar there and here is 10 FD_ORACLE
_oracles = {}


def _truth(c, cell, pos):
    key = c["path"]
    if key not in _oracles:
        _oracles[key] = allegro_torch.build(c["cfg"], c["w"])
    big, x = rc.periodic_view(cell, pos, vc.FULL)
    return util.oracle_run(c["cfg"], c["w"], big, x, c["types"], c["names"], oracle=_oracles[key])


def _fresh_compute(fresh, c):
    return lambda x, cell: fresh.compute_cell(x, c["mt"], cell, vc.FULL, vc.SKIN)


@pytest.mark.parametrize("key", list(vc.SMALL))
def test_relaxation_equals_the_numpy_algorithm(emu_lib, model_dir, key):
    spec = vc.SMALL[key]
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = vc.reference(spec, _fresh_compute(fresh, c), rc.largest_cutoff(fresh))
    assert ref["margin"] >= vc.MARGIN and vc.DET_WINDOW[0] <= ref["det_range"][0] <= ref["det_range"][1] <= vc.DET_WINDOW[1]
    assert np.abs(ref["cell"] - cell).max() > 1e-3                      # the cell has moved
    if spec["fmax"] > 0:
        assert ref["converged"] and 0 < ref["steps"] < spec["max_steps"]
    else:
        assert ref["steps"] == spec["max_steps"] and ref["rebuilds"] >= 2
    if spec["par"].get("hydrostatic"):                                  # only the volume changes: D is a multiple of I
        D = ref["D"]
        assert np.abs(D - D[0, 0] * np.eye(3)).max() < 1e-15 and abs(D[0, 0] - 1) > 1e-3
    want = vc.expected_evaluations(dict(steps=ref["steps"], rebuilds=ref["rebuilds"]), ref, spec["max_steps"])
    for every in (1, 4, 7):
        res = vc.run(model, spec, c["mt"], check_every=every)
        assert model.last_path == "generic_f64"
        vc.check_run(res, ref)
        info = res["info"]
        if every == 1:
            assert info["evaluations"] == want, (info, want)
        else:
            assert want <= info["evaluations"] <= want + info["rebuilds"] * (every - 1), (info, want)
        rc.check_edges(res, res["cell"], res["positions"], vc.FULL, c["cfg"]["r_max"])
    rc.check_tight(res, _truth(c, res["cell"], res["positions"]))
    vc.check_hold(model, res, c["mt"])
    model.close(); fresh.close()


def test_strain_force_is_minus_dH_dD_over_c(emu_lib, model_dir):
    """Conventions, without an optimiser.  With max_step so large that s = 1, the first move (v = 0: c1 = c2 = 0, dt = dt_start f_dec) leaves
    D' = I + dt^2 G_D / c, so the cell it returns exposes the strain force G_D the library handed to FIRE.  c G_D must be -dH/dD of H = E + pressure V at
    fixed q: central differences of the library's own energy under D = I +- 1e-5 e_ab, all nine (a, b), Cu2AgO4, float64; step and bar of
    tests/test_calculator.py::test_stress_equals_the_strain_derivative.  The max_steps = 0 outputs give W and smax by the same convention."""
    c = rc.small_case("Cu2AgO4", model_dir)
    cell, x0, _ = vc.start(vc.SMALL["triclinic"])
    n, pressure, h = len(x0), 0.15, 1e-5
    model = capi.Model(c["path"], 0, emu_lib)
    V0 = abs(np.linalg.det(cell))

    def enthalpy(D):
        A = cell @ D.T
        return model.compute_cell(x0 @ D.T, c["mt"], A, vc.FULL, vc.SKIN)[0] + pressure * abs(np.linalg.det(A))

    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            e = np.zeros((3, 3)); e[a, b] = h
            fd[a, b] = -(enthalpy(np.eye(3) + e) - enthalpy(np.eye(3) - e)) / (2 * h)
    assert np.abs(fd).max() > 0.1 and np.abs(fd - fd.T).max() < 10 * FD_ORACLE          # at D = I the force is the symmetric W_ext itself
    out = model.relax_vcell(x0, c["mt"], cell, vc.FULL, vc.SKIN, max_steps=0, pressure=pressure)
    W, V = vc.w_ext(out[4], cell, pressure)
    assert V == pytest.approx(V0, rel=1e-15)
    assert np.abs(W - fd).max() < 10 * FD_ORACLE, np.abs(W - fd).max()
    assert out[5]["smax"] == pytest.approx(np.abs(W).max() / V, rel=1e-12)
    for factor in (None, 2.5):
        cf = float(n) if factor is None else factor
        kw = {} if factor is None else dict(cell_factor=factor)
        one = model.relax_vcell(x0, c["mt"], cell, vc.FULL, vc.SKIN, fmax=0.0, smax=0.0, max_steps=1, max_step=1e9, pressure=pressure, **kw)
        assert one[5]["steps"] == 1
        dt = vc.FIRE["dt_start"] * vc.FIRE["f_dec"]
        D1 = np.linalg.solve(cell, one[6]).T                             # A' = A0 D'^T
        GD = (D1 - np.eye(3)) * cf / dt ** 2
        assert np.abs(cf * GD - fd).max() < 10 * FD_ORACLE, (factor, np.abs(cf * GD - fd).max())
        np.testing.assert_allclose(one[0], (x0 + dt ** 2 * out[2]) @ D1.T, rtol=0, atol=1e-12)      # q' = q + dt^2 F (G = F at D = I), x' = D' q'
    model.close()


def test_a_mask_of_zeros_is_the_fixed_cell_relaxation(emu_lib, model_dir):
    spec = xc.CASES[1]                        # Cu2AgO4, 30 moves with rebuilds
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    model = capi.Model(c["path"], 0, emu_lib)
    want = model.relax_cell(x0, c["mt"], cell, vc.FULL, vc.SKIN, fmax=spec[3], max_steps=spec[4])
    got = model.relax_vcell(x0, c["mt"], cell, vc.FULL, vc.SKIN, fmax=spec[3], smax=0.0, max_steps=spec[4], mask=(0, 0, 0, 0, 0, 0), pressure=0.3)
    assert np.array_equal(got[6], cell)                                  # bit for bit
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-9)
    assert (got[5]["steps"], got[5]["rebuilds"]) == (want[5]["steps"], want[5]["rebuilds"]) and want[5]["rebuilds"] >= 2
    assert got[5]["smax"] == 0.0
    model.close()


def test_a_zz_mask_moves_the_third_column_only(emu_lib, model_dir):
    """W_ext has the zz entry only, so D stays diag(1, 1, d): of the cell entries a_d = D a0_d only the z components change"""
    spec = vc.SMALL["triclinic"]
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    mask = (0, 0, 1, 0, 0, 0)
    ref = vc.reference(dict(spec, max_steps=12), _fresh_compute(fresh, c), rc.largest_cutoff(fresh), mask=mask)
    res = vc.run(model, spec, c["mt"], mask=mask, max_steps=12)
    vc.check_run(res, ref)
    assert res["info"]["steps"] == 12
    assert np.array_equal(res["cell"][:, :2], cell[:, :2])               # bit for bit
    assert abs(res["cell"][2, 2] / cell[2, 2] - 1) > 1e-4
    model.close(); fresh.close()


def test_fixed_atoms_follow_the_cell(emu_lib, model_dir):
    spec = dict(vc.SMALL["triclinic"], max_steps=12)
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    fixed = np.arange(len(x0)) % 3 == 0
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = vc.reference(spec, _fresh_compute(fresh, c), rc.largest_cutoff(fresh), fixed=fixed)
    free = vc.reference(spec, _fresh_compute(fresh, c), rc.largest_cutoff(fresh))
    assert np.array_equal(ref["q"][fixed], x0[fixed]) and np.abs(ref["positions"] - free["positions"])[~fixed].max() > 1e-3      # the mask matters
    res = vc.run(model, spec, c["mt"], fixed=fixed)
    vc.check_run(res, ref)
    D = np.linalg.solve(cell, res["cell"]).T
    np.testing.assert_allclose(res["positions"][fixed], x0[fixed] @ D.T, rtol=0, atol=1e-12)      # x = D q with q as given
    assert np.abs(res["positions"][fixed] - x0[fixed]).max() > 1e-4
    assert np.abs(res["forces"][fixed]).min() > 0                        # reported as the model gives them
    # with the cell held by the mask D = I exactly, and x = D q shows q itself: bit for bit
    still = vc.run(model, spec, c["mt"], fixed=fixed, mask=(0, 0, 0, 0, 0, 0))
    assert np.array_equal(still["positions"][fixed], x0[fixed]) and np.abs(still["positions"][~fixed] - x0[~fixed]).max() > 1e-3
    model.close(); fresh.close()


def test_no_moves_returns_the_start(emu_lib, model_dir):
    spec = vc.SMALL["triclinic"]
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    want = fresh.compute_cell(x0, c["mt"], cell, vc.FULL, vc.SKIN)
    res = vc.run(model, spec, c["mt"], max_steps=0)
    assert np.array_equal(res["positions"], x0) and np.array_equal(res["cell"], cell)
    for k, w in zip(("pe", "forces", "eatom", "virial"), want):
        np.testing.assert_array_equal(res[k], w)
    info = dict(res["info"])
    assert info.pop("fmax") == pytest.approx(np.linalg.norm(want[1], axis=1).max(), rel=1e-14)
    W, V = vc.w_ext(want[3], cell, spec["pressure"])
    assert info.pop("smax") == pytest.approx(np.abs(W).max() / V, rel=1e-13)
    assert info == dict(steps=0, converged=False, evaluations=1, rebuilds=1)
    model.close(); fresh.close()


def test_argument_errors_leave_x_and_the_hold(emu_lib, model_dir):
    spec = vc.SMALL["triclinic"]
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    mt = c["mt"]
    model = capi.Model(c["path"], 0, emu_lib)
    assert model.compute_cell_reuse(x0, mt, cell, vc.FULL, vc.SKIN)[4]
    singular = np.array(cell)
    singular[2] = singular[0] + singular[1]
    bad = [dict(pbc=(1, 1, 0)), dict(pbc=(0, 0, 0)), dict(smax=-1e-3), dict(smax=np.nan), dict(cell_factor=-1.0), dict(cell_factor=np.inf), dict(pressure=np.nan),
           dict(pressure=np.inf), dict(skin=0.0), dict(skin=-1.0), dict(params=False), dict(cell=singular), dict(fmax=-1.0), dict(check_every=0), dict(dt_start=0.0)]
    for kw in bad:
        x, f = x0.copy(), np.full_like(x0, 7.0)
        a = dict(cell=cell, pbc=vc.FULL, skin=vc.SKIN)
        par = {k: v for k, v in kw.items() if k not in a}
        a.update({k: v for k, v in kw.items() if k in a})
        with pytest.raises(capi.AhipError) as e:
            model.relax_vcell(None, mt, a["cell"], a["pbc"], a["skin"], x_inout=x, f=f, **par)
        assert e.value.code == capi.AHIP_ERR_ARG, (kw, e.value)
        assert np.array_equal(x, x0) and np.all(f == 7.0), kw
        assert not model.compute_cell_reuse(x0, mt, cell, vc.FULL, vc.SKIN)[4], kw      # the hold is as it was
    with pytest.raises(TypeError, match="unknown relaxation parameter"):
        model.relax_vcell(x0, mt, cell, vc.FULL, vc.SKIN, smaxx=0.1)
    model.close()


def test_a_cell_that_would_invert_is_a_state_error(emu_lib, model_dir):
    """cell_factor 1e-3 under a large pressure with max_step 1e3: the first move would make D' = I - (some 1e4) I.  Decision 5 refuses it inside the chunk."""
    spec = vc.SMALL["cubic"]
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    model = capi.Model(c["path"], 0, emu_lib)
    x, f = x0.copy(), np.full_like(x0, 7.0)
    with pytest.raises(capi.AhipError) as e:
        model.relax_vcell(None, c["mt"], cell, vc.FULL, vc.SKIN, x_inout=x, f=f, fmax=0.0, smax=0.0, max_steps=8, check_every=4, cell_factor=1e-3, max_step=1e3,
                          pressure=2.0, hydrostatic=1)
    assert e.value.code == capi.AHIP_ERR_STATE and "invert" in e.value.msg
    assert np.array_equal(x, x0) and np.all(f == 7.0)
    assert model.compute_cell_reuse(x0, c["mt"], cell, vc.FULL, vc.SKIN)[4]             # a failure behind a launch ends the hold
    model.close()


def test_calculator_relax_variable_cell(emu_lib, model_dir):
    spec = vc.SMALL["cubic"]
    c = rc.small_case(spec["geom"], model_dir)
    cell, x0, _ = vc.start(spec)
    calc = Calculator(c["path"], lib=emu_lib, skin=vc.SKIN, reuse=True)
    model = capi.Model(c["path"], 0, emu_lib)
    kw = dict(fmax=spec["fmax"], max_steps=spec["max_steps"], check_every=3)
    out = calc.relax(cell, x0, c["symbols"], variable_cell=True, smax=spec["smax"], pressure=spec["pressure"], **kw)
    want = vc.run(model, spec, c["mt"], check_every=3)
    assert set(out) == {"energy", "forces", "atomic_energy", "virial", "stress", "positions", "cell", "info"}
    assert {k: out["info"][k] for k in want["info"]} == want["info"] and out["info"]["converged"] and "smax" in out["info"]
    np.testing.assert_array_equal(out["positions"], want["positions"])
    np.testing.assert_array_equal(out["cell"], want["cell"])
    np.testing.assert_allclose(out["stress"], -vc.sym3(out["virial"]) / abs(np.linalg.det(out["cell"])), rtol=0, atol=1e-15)      # of the returned cell
    assert np.abs(out["stress"] + spec["pressure"] * np.eye(3)).max() <= spec["smax"]     # relaxed: stress = -pressure to within smax
    again = calc.compute(out["cell"], out["positions"], c["symbols"])
    assert not again["info"]["rebuilt"]       # a reuse=True calculator goes on from the hold of the relaxation
    for k in ("energy", "forces", "atomic_energy", "virial", "stress"):
        np.testing.assert_allclose(again[k], out[k], rtol=1e-10, atol=1e-9)
    hyd = calc.relax(cell, x0, c["symbols"], variable_cell=True, smax=spec["smax"], pressure=spec["pressure"], hydrostatic=True, strain_mask=[1] * 6, cell_factor=4, **kw)
    ratio = np.linalg.solve(cell, hyd["cell"])
    assert hyd["info"]["converged"] and np.abs(ratio - ratio[0, 0] * np.eye(3)).max() < 1e-14
    fixed_cell = calc.relax(cell, x0, c["symbols"], **kw)                                 # the default path is untouched
    assert "cell" not in fixed_cell and "smax" not in fixed_cell["info"]
    with pytest.raises(ValueError, match="variable_cell=True"):
        calc.relax(cell, x0, c["symbols"], pressure=0.1)
    calc.close(); model.close()
