"""Held neighbor lists (ahip_compute_cell_reuse), shared by the CPU-emulation tests (test_cell_reuse.py) and the GPU tests (test_gpu_cell_reuse.py): the
rebuild criterion stated in numpy, trajectories from fixed seeds whose every step decides with a margin, and the checks of one step."""
import os

import numpy as np

import cell_cases as cc
import util
from oracle import glue
from pair_allegro_amd import capi, lmp_like, model_file

SKIN = 1.0
STEPS = 12
MARGIN = 1e-3
# (name, geometry, pbc, kind, sigma of the Gaussian step per coordinate [A], seed).  The seeds were chosen so that `sequence` finds its asserts satisfied.
SEQUENCES = [
    ("Cu-cubic-walk", "Cu-cubic", (1, 1, 1), "walk", 0.12, 2),
    ("Cu2AgO4-walk", "Cu2AgO4", (1, 1, 1), "walk", 0.12, 2),
    ("Cu2AgO4-slab-walk", "Cu2AgO4", (1, 1, 0), "walk", 0.12, 2),
    ("aspirin-walk", "aspirin", (0, 0, 0), "walk", 0.12, 2),
    ("Cu-cubic-strain", "Cu-cubic", (1, 1, 1), "strain", 0.05, 1),
    ("Cu2AgO4-strain", "Cu2AgO4", (1, 1, 1), "strain", 0.05, 1),
    ("Cu2AgO4-slab-strain", "Cu2AgO4", (1, 1, 0), "strain", 0.05, 1),
    ("aspirin-strain", "aspirin", (0, 0, 0), "strain", 0.05, 1),
]
BIG_WALK = ("CuPd-cubic-big-walk", "CuPd-cubic-big", (1, 1, 1), "walk", 0.08, 2)
# the GPU tests add: 257 atoms (a thread block boundary and a partial wave in the row kernel) and a cell of one atom
BLOCK_WALK = ("CuPd-257-walk", "CuPd-257", (1, 1, 1), "walk", 0.08, 2)
ONE_WALK = ("Cu-one-walk", "Cu-one", (1, 1, 1), "walk", 0.12, 2)
GOLDEN_OF = {"CuPd-257": "CuPd-cubic-big", "Cu-one": "Cu-cubic"}
STRAIN_STEP = 5e-3          # entries of the symmetric strain increment per step


def geometry(name):
    """cell, wrapped positions, symbols: the committed geometries of cell_cases, its 257-atom cut, and the first atom of Cu-cubic alone in its cell"""
    if name == "CuPd-257":
        return cc.big_257()
    if name == "Cu-one":
        cell, pos, sym = cc.geometry("Cu-cubic")
        return cell, pos[:1], sym[:1]
    return cc.geometry(name)


def heights(cell):
    inv = np.linalg.inv(cell)
    return 1.0 / np.linalg.norm(inv, axis=0)


def wrap(cell, pos, pbc):
    """the library's wrap: the integer lattice combination that brings s_d into [0, 1) on the periodic axes"""
    s = pos @ np.linalg.inv(cell)
    return pos - (np.floor(s) * np.asarray(pbc, dtype=np.float64)) @ cell


def predict(hold, cell, pos, pbc, rc, skin):
    """The criterion of include/allegro_hip.h in numpy.  hold = (held cell, wrapped held positions).  Returns (reuse?, margin): the relative distance of the
    nearer of the two conditions from its threshold."""
    cell0, x0 = hold
    p = np.asarray(pbc, dtype=bool)
    u = pos - x0
    k = np.floor(u @ np.linalg.inv(cell) + 0.5) * p
    U = np.linalg.norm(u - k @ cell, axis=1).max() if len(pos) else 0.0
    h0 = heights(cell0)
    M = np.ceil(rc / h0) + 1
    g = np.linalg.norm(cell - cell0, axis=1)
    lhs = 2 * U + (M * g)[p].sum()
    margin = abs(lhs - skin) / skin
    ok = lhs <= skin
    if p.any():
        hmin = h0[p].min()
        ok = ok and g[p].sum() <= hmin
        margin = min(margin, abs(g[p].sum() - hmin) / hmin)
    return bool(ok), float(margin)


def expected_flags(steps, pbc, rc, skin):
    """rebuilt? for every (cell, pos) of `steps` on a fresh handle, following the hold as the library does; asserts the margin at every decision"""
    hold, flags = None, []
    for cell, pos in steps:
        reuse = False
        if hold is not None:
            reuse, margin = predict(hold, cell, pos, pbc, rc, skin)
            assert margin >= MARGIN, f"step {len(flags)}: a rounding could decide (margin {margin:.2e})"
        if not reuse:
            hold = (cell.copy(), wrap(cell, pos, pbc))
        flags.append(not reuse)
    return flags


def sequence(spec, rc, skin=SKIN, steps=STEPS):
    """[(cell, positions)] of one trajectory and its expected rebuilt flags.  walk: cumulative Gaussian steps on a fixed cell; strain: a cumulative symmetric
    strain of cell and positions with a small walk on top.  On every fourth step the caller "wraps": random lattice combinations in [-2, 2] per atom on the
    periodic axes."""
    _, geom, pbc, kind, sigma, seed = spec
    cell0, pos0, _ = geometry(geom)
    rng = np.random.RandomState(seed)
    out, F, walk = [], np.eye(3), np.zeros_like(pos0)
    for t in range(steps):
        if t > 0:
            walk = walk + rng.normal(0.0, sigma, size=pos0.shape)
            if kind == "strain":
                e = rng.normal(0.0, STRAIN_STEP, size=(3, 3))
                F = F @ (np.eye(3) + 0.5 * (e + e.T))
        cell = cell0 @ F
        pos = pos0 @ F + walk
        if t % 4 == 3:
            pos = pos + (rng.randint(-2, 3, size=pos.shape) * np.asarray(pbc)) @ cell
        out.append((cell, pos))
    flags = expected_flags(out, pbc, rc, skin)
    assert flags[0] and sum(flags[1:]) >= 2 and sum(not f for f in flags[1:]) >= 2, f"{spec[0]}: flags {''.join(str(int(f)) for f in flags)}"
    return out, flags


def periodic_view(cell, pos, pbc):
    """a fully periodic cell that the open axes cannot see across (40 A along an open lattice vector, as tests/test_calculator.py does for its slab), and the
    positions wrapped into it: what the oracle and the brute-force search take"""
    big = np.array(cell, dtype=np.float64)
    for d in range(3):
        if not pbc[d] and np.linalg.norm(big[d]) < 40.0:
            big[d] *= 40.0 / np.linalg.norm(big[d])
    return big, lmp_like.wrap(big, pos)


_small = {}


def small_case(geom, model_dir):
    """a small float64 model with the golden case's type names and r_max (as tests/test_calculator.py::_case), and what the oracle needs"""
    if geom not in _small:
        g = util.load_golden(geom + "_r5")
        cfg = model_file.model_S(model_dtype="float64", num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8,
                                 avg_num_neighbors=28.0, type_names=list(g["cfg"]["type_names"]), r_max=float(g["cfg"]["r_max"]))
        w = model_file.init_weights(cfg)
        path = os.path.join(model_dir, f"reuse_{geom}.ahip")
        model_file.save_ahip(path, cfg, w)
        types, names = util.lammps_types(g)
        mt = np.array([cfg["type_names"].index(s) for s in g["symbols"]], dtype=np.int32)
        _small[geom] = dict(g=g, cfg=cfg, w=w, path=path, types=types, names=names, mt=mt, symbols=g["symbols"])
    return _small[geom]


def largest_cutoff(model):
    return float(model.r_max if model.per_edge_type_cutoff is None else max(model.r_max, model.per_edge_type_cutoff.max()))


def as_result(model, out):
    """(energy, forces, eatom, virial[, rebuilt]) of a compute_cell / compute_cell_reuse call with the edges of that evaluation"""
    rows = model.last_cell_rows()
    ei, rij = model.get_edges()
    return dict(pe=out[0], forces=out[1], eatom=out[2], virial=out[3], edges=(ei[0], rows[ei[1]], rij), rows=rows)


def check_tight(res, ref):
    """the bars of tests/test_calculator.py::_check"""
    np.testing.assert_allclose(res["forces"], ref["forces"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res["pe"], ref["pe"], rtol=1e-10)
    np.testing.assert_allclose(res["virial"], ref["virial"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(res["eatom"], ref["eatom"], rtol=0, atol=1e-9)


def check_edges(res, cell, pos, pbc, r_max):
    """edge multiset (i, atom of row j) and sorted distances against the brute-force periodic search at the positions of this step"""
    big, x = periodic_view(cell, pos, pbc)
    bi, bj, bd = glue.brute_force_edges(big, x, r_max)
    ei, ej, rij = res["edges"]
    n = len(pos)
    assert np.array_equal(res["rows"][:n], np.arange(n)) and (len(ei) == 0 or ei.max() < n)
    assert sorted(zip(ei.tolist(), ej.tolist())) == sorted(zip(bi.tolist(), bj.tolist()))
    np.testing.assert_allclose(np.sort(rij), np.sort(bd), rtol=0, atol=1e-5)


def check_invalidation(model, mt, cell, pos, check, skin=SKIN):
    """Everything that ends a hold, and what must not.  `check(result, cell, pos, mt, pbc)` judges every evaluation against the caller's truth."""
    full = (1, 1, 1)

    def call(cell=cell, pos=pos, mt=mt, pbc=full, skin=skin):
        out = model.compute_cell_reuse(pos, mt, cell, pbc, skin)
        res = as_result(model, out)
        assert len(res["rows"]) >= len(pos) and np.array_equal(res["rows"][: len(pos)], np.arange(len(pos)))
        check(res, cell, pos, mt, pbc)
        return out[4]

    model.cell_reuse_reset()
    assert call() and not call()
    a = 0
    b = int(np.nonzero(mt != mt[a])[0][0])
    swapped = mt.copy()
    swapped[[a, b]] = mt[[b, a]]
    assert call(mt=swapped) and not call(mt=swapped)                 # two species swapped
    assert call() and not call()
    assert call(pos=pos[:-1], mt=mt[:-1])                            # one atom fewer
    assert call() and not call()
    assert call(pbc=(1, 1, 0)) and not call(pbc=(1, 1, 0))           # an axis opened
    assert call() and not call()
    assert call(skin=0.7 * skin)                                     # another skin
    assert call() and not call()
    model.compute_cell(pos, mt, cell, full, skin)
    assert call() and not call()
    model.compute_cells([0, len(pos)], pos, mt, [cell], [full], skin)
    assert call() and not call()
    model.compute_cells([0], np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3, 3)), np.zeros((0, 3)), skin)
    assert not call()                                                # a batch without atoms installs nothing: the hold stays, and so do its rows
    model.set_option("timing", "0")
    assert call() and not call()
    assert model.cell_reuse_stats()[0] > 0
    model.cell_reuse_reset()
    assert model.cell_reuse_stats() == (0, 0)
    assert call()
    singular = np.array(cell)
    singular[2] = singular[0] + singular[1]
    nan = np.array(cell)
    nan[1, 1] = np.nan
    badtype = mt.copy()
    badtype[1] = model.num_types
    for args in ((pos, mt, singular), (pos, mt, nan), (pos, badtype, cell)):
        try:
            model.compute_cell_reuse(args[0], args[1], args[2], full, skin)
        except capi.AhipError as e:
            assert e.code == capi.AHIP_ERR_ARG, e
        else:
            raise AssertionError("a bad argument was accepted")
    assert not call()                                                # a call refused for its arguments leaves the hold in place
    assert call(skin=0.0) and call(skin=0.0)                         # no skin: every call rebuilds
    assert model.cell_reuse_stats() == (4, 3)
