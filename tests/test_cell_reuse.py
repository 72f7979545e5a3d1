"""ahip_compute_cell_reuse and Calculator(reuse=True) on the CPU emulation, float64: trajectories that mix reused and rebuilt calls (a walk, a straining
cell, open axes, callers that wrap in between) against the torch oracle at every step, the rebuild flag against the criterion stated in numpy, and
everything that must end a hold."""
import numpy as np
import pytest

import cell_reuse_cases as rc
import util
from oracle import allegro_torch
from pair_allegro_amd import capi
from pair_allegro_amd.calculator import Calculator

_oracles = {}


def _truth(c, cell, pos, pbc, types=None):
    """the torch oracle on the wrapped structure (open axes: in a cell they cannot see across)"""
    key = c["path"]
    if key not in _oracles:
        _oracles[key] = allegro_torch.build(c["cfg"], c["w"])
    big, x = rc.periodic_view(cell, pos, pbc)
    return util.oracle_run(c["cfg"], c["w"], big, x, c["types"] if types is None else types, c["names"], oracle=_oracles[key])


@pytest.mark.parametrize("spec", rc.SEQUENCES, ids=[s[0] for s in rc.SEQUENCES])
def test_trajectory_equals_the_oracle(emu_lib, model_dir, spec):
    c = rc.small_case(spec[1], model_dir)
    pbc = spec[2]
    model = capi.Model(c["path"], 0, emu_lib)
    steps, flags = rc.sequence(spec, rc.largest_cutoff(model) + rc.SKIN)
    got = []
    for cell, pos in steps:
        out = model.compute_cell_reuse(pos, c["mt"], cell, pbc, rc.SKIN)
        got.append(out[4])
        res = rc.as_result(model, out)
        rc.check_tight(res, _truth(c, cell, pos, pbc))
        rc.check_edges(res, cell, pos, pbc, c["cfg"]["r_max"])
        assert model.last_path == "generic_f64"
    assert got == flags
    assert model.cell_reuse_stats() == (len(steps), sum(flags))
    model.close()


def test_a_large_cell_change_rebuilds(emu_lib, model_dir):
    """sum_d g_d > min_d h0_d: skin 8 A on the 3.61 A Cu cell, every lattice vector changed by 1.3 A (3.9 A in all), the atoms carried along"""
    c = rc.small_case("Cu-cubic", model_dir)
    cell0, pos0, _ = rc.cc.geometry("Cu-cubic")
    pbc, skin = (1, 1, 1), 8.0
    model = capi.Model(c["path"], 0, emu_lib)
    assert model.compute_cell_reuse(pos0, c["mt"], cell0, pbc, skin)[4]
    assert not model.compute_cell_reuse(pos0, c["mt"], cell0, pbc, skin)[4]
    cell = cell0 + 1.3 * np.eye(3)
    pos = pos0 @ np.linalg.inv(cell0) @ cell
    g = np.linalg.norm(cell - cell0, axis=1)
    assert g.sum() > 1.001 * rc.heights(cell0).min()
    ok, margin = rc.predict((cell0, rc.wrap(cell0, pos0, pbc)), cell, pos, pbc, rc.largest_cutoff(model) + skin, skin)
    assert not ok and margin >= rc.MARGIN
    out = model.compute_cell_reuse(pos, c["mt"], cell, pbc, skin)
    assert out[4]
    res = rc.as_result(model, out)
    rc.check_tight(res, _truth(c, cell, pos, pbc))
    rc.check_edges(res, cell, pos, pbc, c["cfg"]["r_max"])
    assert model.cell_reuse_stats() == (3, 2)
    model.close()


def test_what_ends_a_hold(emu_lib, model_dir):
    c = rc.small_case("Cu2AgO4", model_dir)
    cell, pos, _ = rc.cc.geometry("Cu2AgO4")
    model = capi.Model(c["path"], 0, emu_lib)
    rc.check_invalidation(model, c["mt"], cell, pos, lambda res, cell, pos, mt, pbc: rc.check_tight(res, _truth(c, cell, pos, pbc, types=_lammps_types(c, mt))))
    model.close()


def _lammps_types(c, mt):
    return np.array([c["names"].index(c["cfg"]["type_names"][t]) + 1 for t in mt], dtype=np.int32)


def test_calculator_reuse(emu_lib, model_dir):
    spec = rc.SEQUENCES[1]
    c = rc.small_case(spec[1], model_dir)
    with pytest.raises(ValueError, match="skin"):
        Calculator(c["path"], lib=emu_lib, reuse=True)
    with pytest.raises(ValueError, match="skin"):
        Calculator(c["path"], lib=emu_lib, skin=0.0, reuse=True)
    calc = Calculator(c["path"], lib=emu_lib, skin=rc.SKIN, reuse=True)
    plain = Calculator(c["path"], lib=emu_lib, skin=rc.SKIN)
    steps, flags = rc.sequence(spec, rc.largest_cutoff(calc.model) + rc.SKIN)
    for (cell, pos), flag in zip(steps[:8], flags):
        out = calc.compute(cell, pos, c["symbols"])
        ref = plain.compute(cell, pos, c["symbols"])
        assert out["info"]["rebuilt"] == flag and "rebuilt" not in ref["info"]
        assert out["info"]["nedges"] == ref["info"]["nedges"] and out["info"]["path"] == ref["info"]["path"]
        for k in ("energy", "forces", "atomic_energy", "virial", "stress"):
            np.testing.assert_allclose(out[k], ref[k], rtol=1e-10, atol=1e-9)
    rc.check_tight(dict(pe=ref["energy"], forces=ref["forces"], eatom=ref["atomic_energy"], virial=ref["virial"]), _truth(c, *steps[7], spec[2]))
    assert not calc.compute(*steps[7], c["symbols"])["info"]["rebuilt"]
    calc.reset()
    assert calc.compute(*steps[7], c["symbols"])["info"]["rebuilt"]
    # compute_many is unaffected, apart from ending the hold
    many = calc.compute_many([(steps[7][0], steps[7][1], c["symbols"])])
    np.testing.assert_allclose(many[0]["forces"], ref["forces"], rtol=0, atol=1e-9)
    assert calc.compute(*steps[7], c["symbols"])["info"]["rebuilt"]
    assert not calc.compute(*steps[7], c["symbols"])["info"]["rebuilt"]
    calc.close(); plain.close()
