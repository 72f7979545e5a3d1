"""Geometries of the wide_tile=auto tests (tests/test_gpu_wide_tile.py): the 128-slot / 8-wave tile shape of k_fused_lx for centres with 65..128 edges.

The lattice, the asymmetric per-edge-type cutoff that sets the degree per centre type and the brute-force degree count are those of tests/dense_centres_cases.py
(256-atom fcc, 0.02 A jitter; shells: 12 at 2.56 A, 18 at 3.62, 42 at 4.43, 54 at 5.11, 78 at 5.72, 86 at 6.26, 134 at 6.76, 140 at 7.23).  Every cutoff and every
list cutoff (cutoff + skin) below sits >= 0.14 A from the nearest shell.  Model: l_max = 2, 32 tensor features, 3 layers unless a test overrides it.

  case       Cu cutoff   Pd cutoff   skin   pins
  all78      5.95        5.95        0.15   list rows <= 128: single-pass edge build, tile shape decided on the device; one centre per tile, waves 5..7 of every tile empty
  mixed      5.4         5.95        0.15   tiles of 54 + 54, and 54 + 78 does not fit -> 78 alone: two centres per tile
  sparse     3.0         5.95        0.15   12-edge centres: tiles close on the centre limit, not on slots; mostly empty tiles beside a 78-edge one
  rows140    5.4         5.95        1.3    list rows of 140+: two-pass edge build, the host decides the shape (dense_centres_cases: lx_rows)
  above128   5.95        7.0         0.15   four centres with 134 edges: still heavy (dense_centres=split), 252 centres in 128-slot tiles
  light      5.4         5.4         1.0    list rows of 86, degrees of 54: both shapes launched, the 64-slot one runs
"""
import numpy as np

import dense_centres_cases as dc
import util
from pair_allegro_amd import lmp_like, model_file

NAMES = dc.NAMES
R12 = 3.0                       # 12 edges per centre (first shell only)
LX = dict(l_max=2, num_layers=3, num_tensor_features=32)

# name -> (heavy atoms, Cu cutoff, Pd cutoff, skin, degree of a Cu centre, degree of a Pd centre, list rows: "single" (65..128 entries) or "two_pass" (> 128))
_ROWS = dc.CASES["lx_rows"]
CASES = {
    "all78": (dc.HEAVY, dc.R78, dc.R78, 0.15, 78, 78, "single"),
    "mixed": (dc.HEAVY, dc.R54, dc.R78, 0.15, 54, 78, "single"),
    "sparse": (dc.HEAVY, R12, dc.R78, 0.15, 12, 78, "single"),
    "rows140": (_ROWS[1], _ROWS[2], _ROWS[3], _ROWS[4], 54, 78, "two_pass"),
    "above128": (dc.HEAVY, dc.R78, dc.R134, 0.15, 78, 134, "two_pass"),
    "light": (dc.HEAVY, dc.R54, dc.R54, 1.0, 54, 54, "single"),
}
_geom, _built = {}, {}


def geometry(name):
    """dict(cell, pos, types, pcut, skin, rs, deg): the rank system and the brute-force degree of every local centre, its structure asserted."""
    if name not in _geom:
        heavy, rc_cu, rc_pd, skin, deg_cu, deg_pd, rows = CASES[name]
        cell, pos, types = dc.fcc(heavy)
        pcut = [[rc_cu, rc_cu], [rc_pd, rc_pd]]
        rs = lmp_like.build_rank_system(cell, pos, types, max(rc_cu, rc_pd) + skin)
        deg = dc.degrees(rs, np.asarray(pcut))
        # the structure the case is there for, before anything runs
        is_pd = rs.type[: rs.nlocal] == 2
        assert int(is_pd.sum()) == len(heavy)
        assert (deg[~is_pd] == deg_cu).all() and (deg[is_pd] == deg_pd).all()
        assert deg.min() == min(deg_cu, deg_pd) and deg.max() == max(deg_cu, deg_pd)
        nmax = int(rs.numneigh.max())
        assert (64 < nmax <= 128) if rows == "single" else nmax > 128, nmax
        _geom[name] = dict(cell=cell, pos=pos, types=types, pcut=pcut, skin=skin, rs=rs, deg=deg, r_max=max(rc_cu, rc_pd))
    return _geom[name]


def case(model_dir, name, **over):
    """The geometry plus a model written for it (LX with `over` applied): what dense_centres_cases.run takes."""
    key = (name,) + tuple(sorted(over.items()))
    if key not in _built:
        g = geometry(name)
        cfg = model_file.model_S(type_names=NAMES, r_max=g["r_max"], per_edge_type_cutoff=g["pcut"], avg_num_neighbors=56.0, **dict(LX, **over))
        w = model_file.init_weights(cfg)
        path = f"{model_dir}/wide_{name}_" + "_".join(f"{k}{v}" for k, v in sorted(over.items())) + ".ahip"
        model_file.save_ahip(path, cfg, w)
        _built[key] = dict(g, cfg=cfg, w=w, path=path)
    return _built[key]


def reference(c):
    """The float64 oracle's result for a case, computed once."""
    if "ref" not in c:
        c["ref"] = util.oracle_run(dict(c["cfg"], model_dtype="float64"), c["w"], c["cell"], c["pos"], c["types"], NAMES, skin=c["skin"])
    return c["ref"]
