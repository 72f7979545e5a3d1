"""Geometries and one-evaluation runner of the dense_centres=split tests (tests/test_gpu_dense_centres.py, tests/test_dense_centres.py).

An fcc lattice (256 atoms, a = 3.615 A, 0.02 A jitter) whose degree structure is set by an ASYMMETRIC per-edge-type cutoff matrix: the cutoff of an edge is
that of its CENTRE's type, so the few atoms of the second type are the heavy centres and nothing else changes around them.  fcc shells: 12 at 2.56 A,
18 at 3.62, 42 at 4.43, 54 at 5.11, 78 at 5.72, 86 at 6.26, 134 at 6.76, 140 at 7.23, 164 at 7.67; the cutoffs sit >= 0.23 A from the nearest shell.
Every case asserts its degree structure by brute force over the rank system (degrees(): all pair distances, no neighbour list)."""
import numpy as np

import atomic_virial_ref as av
import util
from pair_allegro_amd import lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

NAMES = ["Cu", "Pd"]                 # Cu: the bulk, Pd: the heavy centres
A0, NCELL = 3.615, 4
R54, R78, R134 = 5.4, 5.95, 7.0      # cutoffs giving 54, 78 and 134 edges per centre
HEAVY = [5, 100, 102, 201]           # the heavy centres of most cases: 100 and 102 fall to one thread of the kernel that lists them (segments of >= 4 centres)


def fcc(heavy):
    """(cell, pos, types): 4 x 4 x 4 fcc cells, atoms `heavy` of type 2."""
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    g = np.array([[i, j, k] for i in range(NCELL) for j in range(NCELL) for k in range(NCELL)], dtype=np.float64)
    pos = (g[:, None, :] + base[None, :, :]).reshape(-1, 3) * A0
    cell = np.eye(3) * A0 * NCELL
    pos = lmp_like.wrap(cell, pos + np.random.RandomState(7).uniform(-0.02, 0.02, size=pos.shape))
    types = np.ones(len(pos), dtype=np.int32)
    types[np.asarray(heavy)] = 2
    return cell, pos, types


# name -> (model overrides, heavy atoms, cutoff of a Cu centre, cutoff of a Pd centre, skin, heavy threshold of the fused kernel)
CASES = {
    "S_light4": (dict(), HEAVY, R54, R134, 1.0, 128),                            # k_fused: 4 centres above 128, the rest at 54: 4-wave light tiles
    "S_light8": (dict(), HEAVY, R78, R134, 1.0, 128),                            # ... the rest at 78: 8-wave light tiles
    "S_giveup": (dict(), list(range(0, 256, 4)), R54, R134, 1.0, 128),           # one centre in four is heavy
    "lx_rows": (dict(l_max=2, num_layers=3, num_tensor_features=32), HEAVY, R54, R78, 1.3, 64),      # k_fused_lx: 4 centres at 78, list rows of 140+
}
_built = {}


def case(model_dir, name):
    """dict(cfg, w, path, cell, pos, types, skin, rs, thresh, deg, ref): the model file, the rank system, every local centre's degree and the float64 oracle's result."""
    if name not in _built:
        over, heavy, rc_cu, rc_pd, skin, thresh = CASES[name]
        cell, pos, types = fcc(heavy)
        pcut = [[rc_cu, rc_cu], [rc_pd, rc_pd]]
        cfg = model_file.model_S(type_names=NAMES, r_max=max(rc_cu, rc_pd), per_edge_type_cutoff=pcut, avg_num_neighbors=56.0, **over)
        w = model_file.init_weights(cfg)
        path = f"{model_dir}/dense_{name}.ahip"
        model_file.save_ahip(path, cfg, w)
        rs = lmp_like.build_rank_system(cell, pos, types, cfg["r_max"] + skin)
        ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, NAMES, skin=skin)
        _built[name] = dict(cfg=cfg, w=w, path=path, cell=cell, pos=pos, types=types, skin=skin, rs=rs, thresh=thresh,
                            deg=degrees(rs, np.asarray(pcut)), ref=ref)
    return _built[name]


def degrees(rs, pcut):
    """Edges of every local centre, by brute force: all distances from the centre to every atom of the rank system against the cutoff of (type_i, type_j)."""
    d = np.linalg.norm(rs.x[: rs.nlocal, None, :] - rs.x[None, :, :], axis=2)
    cut = pcut[rs.type[: rs.nlocal, None] - 1, rs.type[None, :] - 1]
    keep = d <= cut
    keep[np.arange(rs.nlocal), np.arange(rs.nlocal)] = False
    return keep.sum(axis=1)


def heavy_counts(c):
    """(centres, edges) above the fused kernel's tile, from the brute-force degrees."""
    h = c["deg"] > c["thresh"]
    return int(h.sum()), int(c["deg"][h].sum())


def run(lib, c, options=None, register=False, f0=None, pair=None):
    """One evaluation on the case's rank system through the Pair mirror (a fresh one unless `pair` is given; that one stays open).  f0: forces on entry.
    Returns per-global-atom forces / eatom like util.run_pair, the raw per-rank f, and what the model object reports."""
    rs = c["rs"]
    own = pair is None
    if own:
        pair = PairAllegro(me=0, nprocs=1, lib=lib, quiet=True)
        pair.settings([])
        pair.coeff(["*", "*", c["path"]] + NAMES, ntypes=len(NAMES))
        if register:
            pair.add_custom_output("atomic_virial")
        pair.init_style()
    for k, v in (options or {}).items():
        pair.model.set_option(k, v)
    atom = atom_from_rank_system(rs, len(NAMES))
    if f0 is not None:
        atom.f[:] = f0
    pair.compute(atom, list_from_rank_system(rs))
    n = len(c["pos"])
    forces = np.zeros((n, 3))
    np.add.at(forces, rs.tag - 1, atom.f)
    eatom = np.zeros(n)
    eatom[rs.tag[: rs.nlocal] - 1] = pair.eatom[: rs.nlocal]
    m = pair.model
    out = dict(forces=forces, eatom=eatom, pe=pair.eng_vdwl, virial=pair.virial.copy(), f=atom.f.copy(), path=m.last_path, heavy=m.last_heavy_centres,
               max_degree=m.last_max_degree, occupancy=m.tile_occupancy(), nedges=m.nedges(), W=None)
    if register:
        out["W"] = pair.custom_output("atomic_virial").reshape(-1, 9)
    if own:
        m.close()
    return out


def oracle_w(c):
    return av.oracle_w(c["cfg"], c["w"], c["rs"], NAMES)
