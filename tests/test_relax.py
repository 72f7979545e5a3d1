"""ahip_relax_cell and Calculator.relax on the CPU emulation, float64: every case of relax_cases through the library against the numpy FIRE over a fresh
ahip_compute_cell on a second handle (moves, rebuilds, convergence, positions to 1e-9 A), the returned forces against the torch oracle, check_every 1, 4 and 7,
fixed atoms, atoms that leave the cell, the degenerate inputs, the argument errors and the hold a success leaves behind."""
import numpy as np
import pytest

import cell_reuse_cases as rc
import relax_cases as xc
import util
from oracle import allegro_torch
from pair_allegro_amd import capi
from pair_allegro_amd.calculator import Calculator

ALL = xc.CASES + [xc.BIG]
_oracles = {}


def _truth(c, cell, pos, pbc):
    """the torch oracle on the wrapped structure (open axes: in a cell they cannot see across)"""
    key = c["path"]
    if key not in _oracles:
        _oracles[key] = allegro_torch.build(c["cfg"], c["w"])
    big, x = rc.periodic_view(cell, pos, pbc)
    return util.oracle_run(c["cfg"], c["w"], big, x, c["types"], c["names"], oracle=_oracles[key])


def _relax(model, c, spec, x0, cell, **kw):
    kw = dict(dict(fmax=spec[3], max_steps=spec[4]), **kw)
    return xc.as_result(model, model.relax_cell(x0, c["mt"], cell, spec[2], xc.SKIN, **kw))


@pytest.mark.parametrize("spec", ALL, ids=[s[0] for s in ALL])
def test_relaxation_equals_the_numpy_fire(emu_lib, model_dir, spec):
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = xc.reference(spec, lambda x: fresh.compute_cell(x, c["mt"], cell, spec[2], xc.SKIN))
    assert ref["margin"] >= xc.MARGIN
    if spec[3] > 0:
        assert ref["converged"] and 0 < ref["steps"] < spec[4]
    else:
        assert ref["steps"] == spec[4] and ref["rebuilds"] >= 2
    for every in (1, 4, 7):
        start = x0.copy()
        res = _relax(model, c, spec, start, cell, check_every=every)
        np.testing.assert_array_equal(start, x0)
        assert model.last_path == "generic_f64"
        xc.check_run(res, ref)
        info = res["info"]
        if every == 1:
            assert info["evaluations"] == xc.expected_evaluations(info, spec[4]), info
        else:
            assert xc.expected_evaluations(info, spec[4]) <= info["evaluations"] <= xc.expected_evaluations(info, spec[4]) + info["rebuilds"] * (every - 1), info
        rc.check_edges(res, cell, res["positions"], spec[2], c["cfg"]["r_max"])
    rc.check_tight(res, _truth(c, cell, res["positions"], spec[2]))
    if spec[0] == xc.SLAB[0]:                 # never wrapped: the atom that left the cell keeps its continuous coordinate
        out = xc.left_cell(cell, res["positions"], spec[2])
        assert len(out) >= 1 and np.array_equal(out, xc.left_cell(cell, ref["positions"], spec[2]))
    xc.check_hold(model, res, c["mt"], cell, spec[2])
    model.close(); fresh.close()


def test_fixed_atoms(emu_lib, model_dir):
    spec = xc.FIXED                           # aspirin, every third atom
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    fixed = np.arange(len(x0)) % 3 == 0
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    ref = xc.reference(spec, lambda x: fresh.compute_cell(x, c["mt"], cell, spec[2], xc.SKIN), fixed=fixed)
    free = xc.reference(spec, lambda x: fresh.compute_cell(x, c["mt"], cell, spec[2], xc.SKIN))
    assert np.abs(ref["positions"] - free["positions"])[~fixed].max() > 1e-3      # the mask matters
    res = _relax(model, c, spec, x0, cell, fixed=fixed)
    assert np.array_equal(res["positions"][fixed], x0[fixed])                     # bit for bit
    xc.check_run(res, ref)
    assert np.abs(res["forces"][fixed]).min() > 0                                 # reported as the model gives them
    rc.check_tight(res, _truth(c, cell, res["positions"], spec[2]))
    model.close(); fresh.close()


def test_no_moves_returns_the_start(emu_lib, model_dir):
    spec = xc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    fresh, model = capi.Model(c["path"], 0, emu_lib), capi.Model(c["path"], 0, emu_lib)
    want = fresh.compute_cell(x0, c["mt"], cell, spec[2], xc.SKIN)
    res = _relax(model, c, spec, x0, cell, max_steps=0)
    assert np.array_equal(res["positions"], x0)
    for k, w in zip(("pe", "forces", "eatom", "virial"), want):
        np.testing.assert_array_equal(res[k], w)
    info = dict(res["info"])
    assert info.pop("fmax") == pytest.approx(np.linalg.norm(want[1], axis=1).max(), rel=1e-14)
    assert info == dict(steps=0, converged=False, evaluations=1, rebuilds=1)
    model.close(); fresh.close()


def test_one_atom_alone(emu_lib, model_dir):
    spec = xc.ONE
    c = rc.small_case("Cu-cubic", model_dir)
    cell, x0, _ = xc.start(spec)
    model = capi.Model(c["path"], 0, emu_lib)
    out = model.relax_cell(x0, c["mt"][:1], cell, spec[2], xc.SKIN, fmax=spec[3], max_steps=spec[4])
    assert np.array_equal(out[0], x0) and np.abs(out[2]).max() < 1e-12             # (its own images pull on it from opposite sides: zero to rounding)
    assert out[5]["steps"] == 0 and out[5]["converged"] and out[5]["fmax"] < 1e-12 and out[5]["rebuilds"] == 1
    model.close()


def test_two_coincident_atoms(emu_lib, model_dir):
    spec = xc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    x = x0.copy()
    x[1] = x[0]
    keep, f = x.copy(), np.full_like(x, 7.0)
    model = capi.Model(c["path"], 0, emu_lib)
    with pytest.raises(capi.AhipError) as e:
        model.relax_cell(None, c["mt"], cell, spec[2], xc.SKIN, x_inout=x, f=f, fmax=0.0, max_steps=5)
    assert e.value.code == capi.AHIP_ERR_STATE and "not finite" in e.value.msg
    assert np.array_equal(x, keep) and np.all(f == 7.0)
    assert model.compute_cell_reuse(x0, c["mt"], cell, spec[2], xc.SKIN)[4]       # a failure behind a launch ends the hold
    model.close()


def test_argument_errors_leave_x_and_the_hold(emu_lib, model_dir):
    spec = xc.CASES[1]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    mt, pbc = c["mt"], spec[2]
    model = capi.Model(c["path"], 0, emu_lib)
    assert model.compute_cell_reuse(x0, mt, cell, pbc, xc.SKIN)[4]
    singular = np.array(cell)
    singular[2] = singular[0] + singular[1]
    nan = np.array(cell)
    nan[1, 1] = np.nan
    badtype = mt.copy()
    badtype[1] = model.num_types
    bad = [dict(cell=singular), dict(cell=nan), dict(mt=badtype), dict(skin=0.0), dict(skin=-1.0), dict(skin=np.nan), dict(fmax=-1e-3), dict(fmax=np.nan),
           dict(max_steps=-1), dict(check_every=0), dict(dt_start=0.0), dict(dt_start=2.0), dict(dt_max=np.inf), dict(max_step=0.0), dict(n_min=-1),
           dict(f_inc=0.9), dict(f_dec=0.0), dict(f_dec=1.5), dict(alpha_start=-0.1), dict(alpha_start=1.5), dict(f_alpha=0.0), dict(f_alpha=1.1)]
    for kw in bad:
        x, f = x0.copy(), np.full_like(x0, 7.0)
        a = dict(cell=cell, mt=mt, skin=xc.SKIN)
        fire = {k: v for k, v in kw.items() if k not in a}
        a.update({k: v for k, v in kw.items() if k in a})
        with pytest.raises(capi.AhipError) as e:
            model.relax_cell(None, a["mt"], a["cell"], pbc, a["skin"], x_inout=x, f=f, **fire)
        assert e.value.code == capi.AHIP_ERR_ARG, (kw, e.value)
        assert np.array_equal(x, x0) and np.all(f == 7.0), kw
        assert not model.compute_cell_reuse(x0, mt, cell, pbc, xc.SKIN)[4], kw   # the hold is as it was
    with pytest.raises(TypeError, match="unknown FIRE parameter"):
        model.relax_cell(x0, mt, cell, pbc, xc.SKIN, fmaxx=0.1)
    model.close()


def test_calculator_relax(emu_lib, model_dir):
    spec = xc.CASES[0]
    c = rc.small_case(spec[1], model_dir)
    cell, x0, _ = xc.start(spec)
    for skin in ({}, dict(skin=0.0)):
        calc = Calculator(c["path"], lib=emu_lib, **skin)
        with pytest.raises(ValueError, match="skin > 0"):
            calc.relax(cell, x0, c["symbols"])
        calc.close()
    calc = Calculator(c["path"], lib=emu_lib, skin=xc.SKIN, reuse=True)
    model = capi.Model(c["path"], 0, emu_lib)
    out = calc.relax(cell, x0, c["symbols"], fmax=spec[3], max_steps=spec[4], check_every=3)
    want = _relax(model, c, spec, x0, cell, check_every=3)
    assert set(out) == {"energy", "forces", "atomic_energy", "virial", "stress", "positions", "info"}
    assert {"steps", "converged", "fmax", "evaluations", "rebuilds", "path", "nghost", "nedges", "row_atom"} <= set(out["info"])
    assert {k: out["info"][k] for k in want["info"]} == want["info"] and out["info"]["converged"]
    np.testing.assert_array_equal(out["positions"], want["positions"])
    np.testing.assert_array_equal(out["forces"], want["forces"])
    again = calc.compute(cell, out["positions"], c["symbols"])
    assert not again["info"]["rebuilt"]       # a reuse=True calculator goes on from the hold of the relaxation
    for k in ("energy", "forces", "atomic_energy", "virial", "stress"):
        np.testing.assert_allclose(again[k], out[k], rtol=1e-10, atol=1e-9)
    other = calc.relax(cell, x0, c["symbols"], fmax=spec[3], max_steps=spec[4], dt_start=0.2)
    assert other["info"]["converged"] and np.abs(other["positions"] - out["positions"]).max() > 1e-6      # the FIRE parameters reach the library
    calc.close(); model.close()
