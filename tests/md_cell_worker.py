"""Worker of tests/test_md_cell_ranks.py (one process per rank, gloo): md.Simulation with a 3x3 box -- the triclinic cell Q of tests/comm_cell_cases.py -- decomposed
over the ranks, against the one-rank run of the same cell."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

from pair_allegro_amd import capi, md, model_file

Q = np.array([[32.0, 0, 0], [8, 32, 0], [4, 8, 16]])
MASS = 28.0855


def atoms():
    """a perturbed 8 x 8 x 4 lattice in fractional coordinates: 256 atoms about 4 A apart, whole lattice planes within 0.4 A of the brick faces, some atoms left outside the cell (the first migration wraps them)"""
    rng = np.random.default_rng(31)
    s = np.stack(np.meshgrid(np.arange(8) / 8.0, np.arange(8) / 8.0, np.arange(4) / 4.0, indexing="ij"), -1).reshape(-1, 3) + 1.0 / 256
    x = s @ Q + rng.uniform(-0.3, 0.3, size=(len(s), 3))
    x[::17] += Q[0] - Q[2]
    return x


def run(lib, path, pos, vel, cfg, grid, rank, d, nsteps, skin, overlap):
    model = capi.Model(path, 0, lib)
    sim = md.Simulation(md.HipBackend(model, [MASS]), Q, cfg["r_max"], skin, pos, np.zeros(len(pos), np.int32), vel, torch.device("cpu"), grid=grid, rank=rank,
                        dist=d, dt=0.001, overlap=overlap, neigh_every=4, neigh_check=False)          # a re-neighboring (and with it a migration) forced every 4 steps
    own0 = set(sim.tag[: sim.nlocal].tolist())
    sim.setup()
    f = sim.gather_forces()
    for _ in range(nsteps):
        sim.step()
    x = torch.zeros((len(pos), 3), dtype=torch.float64)
    x[sim.tag[: sim.nlocal]] = sim.x[: sim.nlocal]
    moved = torch.tensor([len(set(sim.tag[: sim.nlocal].tolist()) - own0)])
    nl = torch.tensor([sim.nlocal])
    if d is not None and sim.nranks > 1:
        d.all_reduce(x); d.all_reduce(moved); d.all_reduce(nl)
    e = sim.thermo([MASS])["pe"]
    out = dict(f=f, x=x.numpy(), e=e, nreb=sim.nrebuild, moved=int(moved), nl=int(nl), lib_plan=bool(getattr(sim, "_lib_plan", False)), n_int=sim.n_int, overlap=sim.overlap)
    model.close()
    return out


def main():
    out, libpath, model_dir, temperature, nsteps, skin, overlap = sys.argv[1:8]
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    grid = md.choose_grid(world)
    lib = capi.Library(libpath)
    cfg = model_file.model_S(model_dtype="float64", num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8, avg_num_neighbors=28.0)
    path = os.path.join(model_dir, f"md_cell_r{rank}.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    pos = atoms()
    vel = md.maxwell_boltzmann(len(pos), np.full(len(pos), MASS), float(temperature), 12345)
    r2 = run(lib, path, pos, vel, cfg, grid, rank, dist, int(nsteps), float(skin), overlap == "1")
    assert r2["nl"] == len(pos), "atoms lost or duplicated in migration"
    assert r2["lib_plan"], "the re-neighboring did not go through ahip_comm_migrate_cell / ahip_comm_borders_cell"
    assert r2["overlap"] == (overlap == "1")
    if rank == 0:
        r1 = run(lib, path, pos, vel, cfg, (1, 1, 1), 0, None, int(nsteps), float(skin), False)
        inv = np.linalg.inv(Q)
        wrap = lambda x: x - np.floor(x @ inv + 1e-9) @ Q
        np.savez(out, f1=r1["f"], f2=r2["f"], x1=wrap(r1["x"]), x2=wrap(r2["x"]), e1=r1["e"], e2=r2["e"], nreb=r2["nreb"], nreb1=r1["nreb"], moved=r2["moved"], n_int=r2["n_int"])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
