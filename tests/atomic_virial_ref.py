"""Per-atom virial ("atomic_virial", [nall][9]): the float64 oracle's W and one library evaluation that returns it.  Shared by
tests/test_atomic_virial.py (CPU emulation) and tests/test_gpu_atomic_virial.py.

    W_j[a][b] = - sum over the edges e = (i -> j) with NEIGHBOUR j of r_e[a] * dE/dr_e[b],     r_e = x_j - x_i

Rows exist for locals and ghosts; the symmetric part of the sum over all rows is the global virial."""
import numpy as np

import path_parity
from pair_allegro_amd import lmp_like
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

SKIN = 1.0


def rank_system(cfg, cell, pos, types, grid=(1, 1, 1), rank=(0, 0, 0)):
    return lmp_like.build_rank_system(cell, pos, types, cfg["r_max"] + SKIN, grid=grid, rank=rank)


def w_from_edges(nall, ei, rvec, grad):
    """W [nall][9] from edges ei [2, E], edge vectors [E, 3] and gradients dE/dr_e [E, 3]."""
    w = np.zeros((nall, 9))
    np.add.at(w, np.asarray(ei[1]), -(np.asarray(rvec)[:, :, None] * np.asarray(grad)[:, None, :]).reshape(-1, 9))
    return w


def oracle_w(cfg, w, rs, names):
    ei, grad = path_parity.oracle_edge_gradients(cfg, w, rs, names)
    ei = np.asarray(ei)
    return w_from_edges(rs.nall, ei, rs.x[ei[1]] - rs.x[ei[0]], grad)


def sym_sum(w):
    """Sum over all rows, symmetrised, as (xx, yy, zz, xy, xz, yz) like the `virial` output of the pair style."""
    t = w.sum(axis=0).reshape(3, 3)
    s = 0.5 * (t + t.T)
    return np.array([s[0, 0], s[1, 1], s[2, 2], s[0, 1], s[0, 2], s[1, 2]])


def run(lib, model_path, rs, names, options=None, register=True):
    """One evaluation on one rank system; returns W (None unless registered), f [nall][3], eatom, energy, virial and the path taken."""
    pair = PairAllegro(me=0, nprocs=1, lib=lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", model_path] + list(names), ntypes=len(names))
    for k, v in (options or {}).items():
        pair.model.set_option(k, v)
    if register:
        pair.add_custom_output("atomic_virial")
    pair.init_style()
    atom = atom_from_rank_system(rs, len(names))
    pair.compute(atom, list_from_rank_system(rs))
    out = dict(f=atom.f.copy(), eatom=pair.eatom[: rs.nlocal].copy(), pe=pair.eng_vdwl, virial=pair.virial.copy(),
               path=pair.model.last_path, max_degree=pair.model.last_max_degree, W=None)
    if register:
        out["W"] = pair.custom_output("atomic_virial").reshape(-1, 9)
    pair.model.close()
    return out
