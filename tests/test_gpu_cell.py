"""GPU: any periodic cell on the device path.  The ghost builder and the wrap (csrc/neigh.hip) against the rule stated in numpy, ahip_compute_cell in
float32 against the committed goldens (cells thinner than the cutoff, triclinic, a molecule), and md.Simulation with a 3x3 box against the host-list path of
the same library."""
import numpy as np
import pytest
import torch

import cell_cases as cc
import parity_cases as pc
import util
from pair_allegro_amd import capi, lmp_like, md

pytestmark = pytest.mark.gpu
MASSES = {"Cu": 63.546, "Ag": 107.8682, "O": 15.999}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(hip_lib, model_dir):
    m = cc.border_model(hip_lib, model_dir, "float32")
    yield m
    m.close()


@pytest.mark.parametrize("name,rc,pbc,expected", cc.GHOST_CASES)
def test_ghost_set_equals_the_rule(model, dev, name, rc, pbc, expected):
    cell, x, sym = cc.geometry(name)
    cc.check_ghost_set(model, dev, cell, x, cc.types_of(sym), pbc, rc, expected)


def test_one_atom(model, dev):
    cell, x, sym = cc.geometry("Cu-cubic")
    cc.check_ghost_set(model, dev, cell, x[:1], cc.types_of(sym)[:1], (1, 1, 1), 6.0)


def test_257_atoms_cross_a_block_boundary(model, dev):
    cell, x, sym = cc.big_257()
    cc.check_ghost_set(model, dev, cell, x, cc.types_of(sym), (1, 1, 1), 6.0)


def test_capacity_protocol(model, dev):
    cc.check_capacity(model, dev)


def test_orthogonal_box_reduces_to_borders_local(model, dev):
    cc.check_orthogonal_reduction(model, dev)


def test_wrap(model, dev):
    cc.check_wrap(model, dev)
    cc.check_wrap(model, dev, "Cu2AgO4-rotated")


def test_argument_errors(model, dev):
    cc.check_errors(model, dev)


@pytest.mark.parametrize("tag", ["Cu-cubic_r5", "Cu-cubic_r15", "Cu2AgO4_r5", "aspirin_r5", "aspirin_r15", "CuPd-cubic-big_r5"])
def test_compute_cell_equals_the_golden(hip_lib, model_dir, tag):
    """ahip_compute_cell, float32 golden model, against the committed golden: the tolerance logic of parity_cases.check_golden, and the edge multiset
    (i, atom of row j) against the brute-force periodic search as in check_edges_vs_brute_force."""
    g = util.load_golden(tag)
    path, cfg, w = util.golden_model(g, model_dir, "float32")
    model = capi.Model(path, 0, hip_lib)
    mt = np.array([cfg["type_names"].index(s) for s in g["symbols"]], dtype=np.int32)
    pe, f, ea, vir = model.compute_cell(g["pos"], mt, g["cell"], (1, 1, 1), skin=1.0)
    rows = model.last_cell_rows()
    ei, rij = model.get_edges()
    res = dict(forces=f, eatom=ea, pe=pe, virial=vir, edges=(ei[0], rows[ei[1]], rij))
    df = float(np.abs(f - g["forces"]).max())
    print(f"{tag}: path={model.last_path} nghost={len(rows) - len(f)} nedges={ei.shape[1]} max|dF|={df:.3e} |dE|={abs(pe - float(g['pe'])):.3e}")
    tol = pc.TOL["float32"]
    if tag.startswith("aspirin"):
        tol *= 23
    util.assert_close_to(res, g, tol, what=f"{tag} compute_cell")
    if not tag.startswith("aspirin"):
        assert df < pc.NORTH_STAR_DF
    pc.check_edges_vs_brute_force(res, g)
    assert len(rows) >= len(f) and np.array_equal(rows[: len(f)], np.arange(len(f)))
    model.close()


@pytest.mark.parametrize("tag,reps,temperature", [("Cu2AgO4_r5", (2, 2, 2), 20000.0), ("Cu-cubic_r5", (1, 1, 1), 40000.0)])
def test_driver_on_a_general_cell(hip_lib, model_dir, dev, tag, reps, temperature):
    """md.Simulation with a 3x3 box, float32 golden models: the 56-atom triclinic supercell and the 3.61 A Cu cell.  20 hot steps with at least one
    re-neighboring (wrap kernel, second ghost build); the final forces equal those of the host-list path of the same library at the final positions."""
    g = util.load_golden(tag)
    path, cfg, w = util.golden_model(g, model_dir, "float32")
    types, names = util.lammps_types(g)
    cell0, pos0 = np.array(g["cell"], dtype=np.float64), lmp_like.wrap(g["cell"], g["pos"])
    grid = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), -1).reshape(-1, 3)
    pos = (pos0[None, :, :] + (grid @ cell0)[:, None, :]).reshape(-1, 3)
    cell = cell0 * np.asarray(reps, dtype=np.float64)[:, None]
    types = np.tile(types, len(grid))
    mapper, _ = util.type_mapper_and_cutoffs(cfg, names)
    mt = mapper[types - 1].astype(np.int32)
    n = len(pos)
    mass_by_mtype = [MASSES[s] for s in cfg["type_names"]]
    model = capi.Model(path, 0, hip_lib)
    vel = md.maxwell_boltzmann(n, np.array([mass_by_mtype[t] for t in mt]), temperature, 4)
    sim = md.Simulation(md.HipBackend(model, mass_by_mtype), cell, cfg["r_max"], 0.2, pos, mt, vel, dev, dt=0.001)
    sim.setup()
    for _ in range(20):
        sim.step()
    assert sim.nrebuild >= 2, "no re-neighboring in 20 steps"
    x = np.zeros((n, 3))
    x[sim.tag[: sim.nlocal].cpu().numpy()] = sim.x[: sim.nlocal].cpu().numpy()
    ref = util.run_pair(hip_lib, path, cell, lmp_like.wrap(cell, x), types, names)
    f = sim.gather_forces()
    print(f"{tag} x{reps}: nrebuild={sim.nrebuild} nghost={sim.nall - sim.nlocal} path={model.last_path} max|dF|={np.abs(f - ref['forces']).max():.3e} max|F|={np.abs(f).max():.3f}")
    tol = pc.TOL["float32"]
    np.testing.assert_allclose(f, ref["forces"], rtol=tol, atol=tol)
    np.testing.assert_allclose(sim.thermo(mass_by_mtype)["pe"], ref["pe"], rtol=tol, atol=tol * n ** 0.5)
    assert np.abs(x - pos).max() > 1e-3
    with pytest.raises(ValueError, match="one rank"):
        md.Simulation(md.HipBackend(model, mass_by_mtype), cell, cfg["r_max"], 0.2, pos, mt, vel, dev, grid=(2, 1, 1))
    model.close()
