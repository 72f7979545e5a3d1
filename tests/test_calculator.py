"""`Calculator` (ahip_compute_cell) and `md.Simulation` with a 3x3 box on the CPU emulation, float64, against the torch oracle on the host-built
LAMMPS view: a cell thinner than the cutoff (Cu-cubic), a triclinic cell thinner than the cutoff in every direction (Cu2AgO4), a molecule in a large
box (aspirin)."""
import os

import numpy as np
import pytest
import torch

import util
from oracle import allegro_torch, glue
from pair_allegro_amd import capi, lmp_like, md, model_file
from pair_allegro_amd.calculator import Calculator

MASSES = {"Cu": 63.546, "Ag": 107.8682, "O": 15.999, "Pd": 106.42, "C": 12.011, "H": 1.008}
_cache = {}
FD_ORACLE = 3.336e-9    # eV: central differences at h = 1e-5 against autograd, torch oracle alone, worst of the six strain components (test_stress_...)
FD_LIB = 3.158e-9       # eV: the library's stress V against central differences of its own energy, same strains (measured; the bar is 10 FD_ORACLE)


def _case(name, model_dir):
    """golden geometry + a small float64 model with the golden case's type_names and r_max (widths as tests/test_md_emu.py::_small_cfg)"""
    if name not in _cache:
        g = util.load_golden(name + "_r5")
        cfg = model_file.model_S(model_dtype="float64", num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8,
                                 avg_num_neighbors=28.0, type_names=list(g["cfg"]["type_names"]), r_max=float(g["cfg"]["r_max"]))
        w = model_file.init_weights(cfg)
        path = os.path.join(model_dir, f"calc_{name}.ahip")
        model_file.save_ahip(path, cfg, w)
        cell, pos = np.array(g["cell"], dtype=np.float64), lmp_like.wrap(g["cell"], g["pos"])
        types, names = util.lammps_types(g)
        ref = util.oracle_run(cfg, w, cell, pos, types, names)              # computed once, shared, never modified
        _cache[name] = dict(g=g, cfg=cfg, w=w, path=path, cell=cell, pos=pos, types=types, names=names, ref=ref)
    return _cache[name]


def _check(out, ref):
    np.testing.assert_allclose(out["forces"], ref["forces"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["energy"], ref["pe"], rtol=1e-10)
    np.testing.assert_allclose(out["virial"], ref["virial"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["atomic_energy"], ref["eatom"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", ["Cu-cubic", "Cu2AgO4", "aspirin"])
def test_calculator_equals_the_oracle(emu_lib, model_dir, name):
    c = _case(name, model_dir)
    calc = Calculator(c["path"], lib=emu_lib)
    out = calc.compute(c["cell"], c["pos"], c["g"]["symbols"])
    _check(out, c["ref"])
    assert out["info"]["path"] == "generic_f64"
    # edges: the golden count, the brute-force distances, rows = atoms then ghosts
    assert out["info"]["nedges"] == int(c["g"]["nedges"])
    ei, rij = calc.model.get_edges()
    rows = out["info"]["row_atom"]
    n = len(c["pos"])
    assert len(rows) == n + out["info"]["nghost"] and np.array_equal(rows[:n], np.arange(n)) and ei[0].max() < n
    bi, bj, bd = glue.brute_force_edges(c["cell"], c["pos"], c["cfg"]["r_max"])
    assert sorted(zip(ei[0].tolist(), rows[ei[1]].tolist())) == sorted(zip(bi.tolist(), bj.tolist()))
    np.testing.assert_allclose(np.sort(rij), np.sort(bd), rtol=0, atol=1e-5)
    # every atom displaced by random lattice vectors: the same answer, in the caller's order
    k = np.random.RandomState(8).randint(-3, 4, size=c["pos"].shape)
    _check(calc.compute(c["cell"], c["pos"] + k @ c["cell"], c["g"]["symbols"]), c["ref"])
    # the skin only inflates the shell and the list
    calc2 = Calculator(c["path"], lib=emu_lib, skin=0.7)
    out2 = calc2.compute(c["cell"], c["pos"], c["g"]["symbols"])
    _check(out2, c["ref"])
    assert out2["info"]["nedges"] == out["info"]["nedges"] and out2["info"]["nghost"] >= out["info"]["nghost"]
    V = abs(np.linalg.det(c["cell"]))
    v = out["virial"]
    np.testing.assert_allclose(out["stress"] * V, -np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]]), rtol=0, atol=1e-12)
    calc.close(); calc2.close()


def test_calculator_open_axes_and_symbols(emu_lib, model_dir):
    c = _case("aspirin", model_dir)
    calc = Calculator(c["path"], lib=emu_lib)
    out = calc.compute(c["cell"], c["pos"], c["g"]["symbols"], pbc=(False, False, False))       # the molecule does not see its images at r_max 5 in a 50 A box
    assert out["stress"] is None and out["info"]["nghost"] == 0
    _check(out, c["ref"])
    assert calc.compute(c["cell"], c["pos"], c["g"]["symbols"], pbc=(True, True, False))["stress"] is None
    with pytest.raises(ValueError, match="Xx"):
        calc.compute(c["cell"], c["pos"], ["Xx"] + list(c["g"]["symbols"][1:]))
    calc.close()
    # a slab: Cu2AgO4 open along c equals the fully periodic evaluation of the same atoms in a cell 40 A tall
    c = _case("Cu2AgO4", model_dir)
    calc = Calculator(c["path"], lib=emu_lib)
    slab = calc.compute(c["cell"], c["pos"], c["g"]["symbols"], pbc=(True, True, False))
    tall = c["cell"].copy(); tall[2] *= 40.0 / np.linalg.norm(tall[2])
    ref = util.oracle_run(c["cfg"], c["w"], tall, lmp_like.wrap(tall, c["pos"]), c["types"], c["names"])
    np.testing.assert_allclose(slab["forces"], ref["forces"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(slab["energy"], ref["pe"], rtol=1e-10)
    assert slab["info"]["nghost"] < calc.compute(c["cell"], c["pos"], c["g"]["symbols"])["info"]["nghost"]
    calc.close()


def _strained_energy(fn, cell, pos, a, b, delta):
    e = np.zeros((3, 3)); e[a, b] = e[b, a] = delta
    F = np.eye(3) + e
    return fn(cell @ F, pos @ F)


def test_stress_equals_the_strain_derivative(emu_lib, model_dir):
    """stress V against central differences of the energy under symmetric strains of +-1e-5 applied to cell and positions, all six components (Cu2AgO4,
    float64).  d E / d delta of the strain e_ab = e_ba = delta is stress_ab V (a == b) or 2 stress_ab V (a != b)."""
    c = _case("Cu2AgO4", model_dir)
    calc = Calculator(c["path"], lib=emu_lib)
    sv = calc.compute(c["cell"], c["pos"], c["g"]["symbols"])["stress"] * abs(np.linalg.det(c["cell"]))
    oracle = allegro_torch.build(c["cfg"], c["w"])
    vr = c["ref"]["virial"]
    sv_oracle = -np.array([[vr[0], vr[3], vr[4]], [vr[3], vr[1], vr[5]], [vr[4], vr[5], vr[2]]])          # autograd
    e_lib = lambda cell, pos: calc.compute(cell, pos, c["g"]["symbols"])["energy"]
    e_orc = lambda cell, pos: util.oracle_run(c["cfg"], c["w"], cell, lmp_like.wrap(cell, pos), c["types"], c["names"], oracle=oracle)["pe"]
    h = 1e-5
    worst_oracle = worst_lib = 0.0
    for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)):
        mult = 1.0 if a == b else 2.0
        fd_orc = (_strained_energy(e_orc, c["cell"], c["pos"], a, b, h) - _strained_energy(e_orc, c["cell"], c["pos"], a, b, -h)) / (2 * h)
        fd_lib = (_strained_energy(e_lib, c["cell"], c["pos"], a, b, h) - _strained_energy(e_lib, c["cell"], c["pos"], a, b, -h)) / (2 * h)
        worst_oracle = max(worst_oracle, abs(fd_orc - mult * sv_oracle[a, b]))
        worst_lib = max(worst_lib, abs(fd_lib - mult * sv[a, b]))
    print(f"stress: finite difference vs autograd on the torch oracle alone {worst_oracle:.3e} eV; library stress V vs its own finite difference {worst_lib:.3e} eV")
    # Measured on the CPU: the same finite difference against autograd on the torch oracle alone disagrees by FD_ORACLE eV (truncation of the central
    # difference at h = 1e-5 plus cancellation in E(+h) - E(-h)); the library is allowed ten times that -- the margin covers the second evaluation path
    # (its own neighbor search and summation order), not looser arithmetic.  FD_ORACLE = 3.336e-9 eV, and the library's own discrepancy measured FD_LIB = 3.158e-9 eV.
    assert worst_lib < 10 * FD_ORACLE
    calc.close()


def _supercell(c, reps):
    g = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), -1).reshape(-1, 3)
    pos = (c["pos"][None, :, :] + (g @ c["cell"])[:, None, :]).reshape(-1, 3)
    return c["cell"] * np.asarray(reps, dtype=np.float64)[:, None], pos, np.tile(c["types"], len(g))


@pytest.mark.parametrize("name,reps,temperature", [("Cu2AgO4", (2, 2, 2), 30000.0), ("Cu-cubic", (1, 1, 1), 60000.0)])
def test_driver_on_a_general_cell(emu_lib, model_dir, name, reps, temperature):
    """md.Simulation with a 3x3 box: a 56-atom triclinic supercell (heights 7.4, 9.4, 10.4 A) and the 3.61 A Cu cell, thinner than rc.  Forces after setup and
    after a hot run with re-neighborings (wrap kernel, second ghost build) equal the oracle's at the same positions."""
    c = _case(name, model_dir)
    cell, pos, types = _supercell(c, reps)
    n = len(pos)
    assert n == len(c["pos"]) * int(np.prod(reps))
    mapper, _ = util.type_mapper_and_cutoffs(c["cfg"], c["names"])
    mt = mapper[types - 1].astype(np.int32)
    mass_by_mtype = [MASSES[s] for s in c["cfg"]["type_names"]]
    ref = util.oracle_run(c["cfg"], c["w"], cell, pos, types, c["names"], skin=0.2)
    model = capi.Model(c["path"], 0, emu_lib)
    vel = md.maxwell_boltzmann(n, np.array([mass_by_mtype[t] for t in mt]), temperature, 4)
    sim = md.Simulation(md.HipBackend(model, mass_by_mtype), cell, c["cfg"]["r_max"], 0.2, pos, mt, vel, torch.device("cpu"), dt=0.001)
    sim.setup()
    np.testing.assert_allclose(sim.gather_forces(), ref["forces"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(sim.thermo(mass_by_mtype)["pe"], ref["pe"], rtol=1e-10)
    steps = 0
    while sim.nrebuild < 2 and steps < 40:
        sim.step()
        steps += 1
    assert sim.nrebuild >= 2, f"no re-neighboring within {steps} steps"
    x = np.zeros((n, 3))
    x[sim.tag[: sim.nlocal].numpy()] = sim.x[: sim.nlocal].numpy()
    ref2 = util.oracle_run(c["cfg"], c["w"], cell, lmp_like.wrap(cell, x), types, c["names"], skin=0.2)
    np.testing.assert_allclose(sim.gather_forces(), ref2["forces"], rtol=0, atol=1e-9)
    assert np.abs(ref2["forces"] - ref["forces"]).max() > 1e-6          # the atoms moved
    model.close()


def test_general_cell_needs_one_rank(emu_lib, model_dir):
    c = _case("Cu-cubic", model_dir)
    model = capi.Model(c["path"], 0, emu_lib)
    be = md.HipBackend(model, [MASSES["Cu"]])
    mt = np.zeros(len(c["pos"]), np.int32)
    for kw in (dict(grid=(2, 1, 1)), dict(overlap=True)):
        with pytest.raises(ValueError, match="one rank"):
            md.Simulation(be, c["cell"], 5.0, 0.2, c["pos"], mt, None, torch.device("cpu"), **kw)
    with pytest.raises(ValueError, match="3x3"):
        md.Simulation(be, np.diag(c["cell"]) * 4, 5.0, 0.2, c["pos"], mt, None, torch.device("cpu"), pbc=(True, True, False))
    with pytest.raises(ValueError):                                      # the 3-vector box keeps its rule: thinner than r_max + skin is refused
        md.Simulation(be, np.diag(c["cell"]), 5.0, 0.2, c["pos"], mt, None, torch.device("cpu"))
    model.close()
