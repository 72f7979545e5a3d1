"""The batch of structures shared by the CPU-emulation tests (test_calculator_batch.py) and the GPU tests (test_gpu_cell_batch.py) of ahip_compute_cells /
Calculator.compute_many: one six-type model, eight structures built from the committed goldens' geometries, the float64 torch oracle of every structure
alone (computed once per model, never modified), and the checks both files run."""
import os

import numpy as np

import cell_cases as cc
import util
from oracle import glue
from pair_allegro_amd import capi, lmp_like, model_file

TYPE_NAMES = ["Cu", "Ag", "O", "Pd", "C", "H"]
R_MAX = 5.0
NAMES = ["Cu-cubic", "empty", "Cu2AgO4", "aspirin-open", "Cu2AgO4-slab", "Cu-atom", "big-257", "Cu-cubic-again"]
_cache = {}


def structures():
    """[(cell, positions, symbols, pbc)] in the order of NAMES"""
    cu = cc.geometry("Cu-cubic")
    tri = cc.geometry("Cu2AgO4")
    asp = cc.geometry("aspirin")
    asp_pos = asp[1] - asp[1].mean(axis=0) + np.array([1.0, -2.0, 0.5])       # around the origin of its 50 A cell: most atoms lie outside the cell
    inv = np.linalg.inv(asp[0])
    assert ((asp_pos @ inv) < 0).any() and ((asp_pos @ inv) > 0).any()
    big = cc.big_257()
    return [
        (cu[0], cu[1], list(cu[2]), (1, 1, 1)),
        (np.eye(3) * 7.0, np.zeros((0, 3)), [], (1, 1, 1)),
        (tri[0], tri[1], list(tri[2]), (1, 1, 1)),
        (asp[0], asp_pos, list(asp[2]), (0, 0, 0)),
        (tri[0], tri[1], list(tri[2]), (1, 1, 0)),
        (np.eye(3) * 20.0, np.array([[3.0, 4.0, 5.0]]), ["Cu"], (1, 1, 1)),
        (big[0], big[1], list(big[2]), (1, 1, 1)),
        (cu[0], cu[1], list(cu[2]), (1, 1, 1)),
    ]


def model(model_dir, dtype, small, type_names=None):
    """(path, cfg, w): model S with the six types -- full width (the fused kernel's shape) or the small float64 widths of test_calculator.py::_case"""
    names = list(type_names or TYPE_NAMES)
    key = (dtype, small, tuple(names))
    if key not in _cache:
        over = dict(num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8) if small else {}
        cfg = model_file.model_S(model_dtype=dtype, type_names=names, r_max=R_MAX, avg_num_neighbors=28.0, **over)
        w = model_file.init_weights(cfg)
        path = os.path.join(model_dir, f"batch_{dtype}_{'small' if small else 'S'}_{len(names)}.ahip")
        model_file.save_ahip(path, cfg, w)
        _cache[key] = (path, cfg, w)
    return _cache[key]


def oracle_cell(cell, pbc):
    """the fully periodic cell whose evaluation equals the open-axis one: every open axis stretched to 40 A (the tall-cell construction of test_calculator.py)"""
    tall = np.array(cell, dtype=np.float64)
    for d in range(3):
        if not pbc[d]:
            tall[d] *= max(1.0, 40.0 / np.linalg.norm(tall[d]))
    return tall


def references(cfg, w):
    """float64 torch oracle of every structure alone (util.oracle_run); empty: zeros; the isolated atom: its type's shift and no force.  Computed once."""
    key = ("ref", cfg["model_dtype"], cfg["num_scalar_features"], tuple(cfg["type_names"]))
    if key not in _cache:
        cfg64 = dict(cfg, model_dtype="float64")
        out = []
        for name, (cell, pos, sym, pbc) in zip(NAMES, structures()):
            n = len(pos)
            if n == 0:
                out.append(dict(forces=np.zeros((0, 3)), eatom=np.zeros(0), pe=0.0, virial=np.zeros(6)))
            elif n == 1:
                sh = float(w["shift"][cfg["type_names"].index(sym[0])])
                out.append(dict(forces=np.zeros((1, 3)), eatom=np.array([sh]), pe=sh, virial=np.zeros(6)))
            else:
                types = np.array([cfg["type_names"].index(s) + 1 for s in sym], dtype=np.int32)
                oc = oracle_cell(cell, pbc)        # (aspirin: its 50 A cell as it is; wrapped into it for the oracle's rank builder, the molecule stays whole through the images)
                r = util.oracle_run(cfg64, w, oc, lmp_like.wrap(oc, pos), types, list(cfg["type_names"]))
                out.append(dict(forces=r["forces"], eatom=r["eatom"], pe=float(r["pe"]), virial=np.asarray(r["virial"])))
        _cache[key] = out
    return _cache[key]


def pack(structs, type_names):
    """-> (first, x, mtype, cells, pbc) as Model.compute_cells takes them"""
    first = np.concatenate([[0], np.cumsum([len(s[1]) for s in structs])]).astype(np.int32)
    x = np.concatenate([np.asarray(s[1], dtype=np.float64).reshape(-1, 3) for s in structs]) if structs else np.zeros((0, 3))
    mt = np.array([type_names.index(a) for s in structs for a in s[2]], dtype=np.int32)
    cells = np.array([s[0] for s in structs], dtype=np.float64).reshape(-1, 3, 3)
    pbc = np.array([s[3] for s in structs], dtype=np.int32).reshape(-1, 3)
    return first, x, mt, cells, pbc


def run_batch(m, structs, type_names, skin=0.0):
    """Model.compute_cells on `structs`; per structure a dict of forces, eatom, pe, virial, plus the rows, the ghost counts and the edges of the call"""
    first, x, mt, cells, pbc = pack(structs, type_names)
    eng, f, ea, vir = m.compute_cells(first, x, mt, cells, pbc, skin)
    res = [dict(forces=f[first[k]: first[k + 1]], eatom=ea[first[k]: first[k + 1]], pe=float(eng[k]), virial=vir[k]) for k in range(len(structs))]
    return res, dict(first=first, eng=eng, f=f, eatom=ea, virial=vir, rows=m.last_cell_rows() if len(x) else np.zeros(0, np.int64),
                     ghosts=m.last_cells_ghosts(), edges=m.get_edges() if len(x) else (np.zeros((2, 0), np.int64), np.zeros(0)), path=m.last_path)


def row_structure(call):
    """structure index of every row (atoms, then ghosts) of a compute_cells call"""
    first = call["first"]
    return np.searchsorted(first, call["rows"], side="right") - 1


def check_ghost_contract(call, structs, dev, border, rc):
    """per structure: the ghost count and the row_atom sequence are those of ahip_borders_cell_dev on the structure alone (src + first[s]); the ghosts of the
    batch are grouped by structure, in order"""
    first, rows, ghosts = call["first"], call["rows"], call["ghosts"]
    n = int(first[-1])
    assert len(ghosts) == len(structs) and len(rows) == n + int(ghosts.sum()) and np.array_equal(rows[:n], np.arange(n))
    g0 = n
    for k, (cell, pos, sym, pbc) in enumerate(structs):
        if len(pos) == 0:
            assert ghosts[k] == 0
            continue
        x = cc.run_wrap(border, dev, cell, pos, pbc)
        mt = np.zeros(len(pos), np.int32)
        ng = cc.run_borders(border, dev, cell, x, mt, pbc, rc, 0)[0]
        assert ghosts[k] == ng, (NAMES[k] if len(structs) == len(NAMES) else k, int(ghosts[k]), ng)
        if ng:
            src = cc.run_borders(border, dev, cell, x, mt, pbc, rc, ng)[3]
            np.testing.assert_array_equal(rows[g0: g0 + ng], src[:ng] + first[k])
        g0 += ng


def check_no_cross_talk(call, structs, rc_model):
    """no edge joins rows of different structures, and the (centre, atom of the neighbour row) multiset of every structure equals the brute-force periodic
    search of the structure alone (open axes: the tall cell)"""
    ei, rij = call["edges"]
    rows, first = call["rows"], call["first"]
    rs = row_structure(call)
    assert np.array_equal(rs[ei[0]], rs[ei[1]]), "an edge joins two structures"
    counts = []
    for k, (cell, pos, sym, pbc) in enumerate(structs):
        sel = rs[ei[0]] == k
        counts.append(int(sel.sum()))
        if len(pos) == 0:
            assert counts[-1] == 0
            continue
        oc = oracle_cell(cell, pbc)
        bi, bj, bd = glue.brute_force_edges(oc, lmp_like.wrap(oc, pos) if not all(pbc) else pos, rc_model)
        assert counts[-1] == len(bi), (k, counts[-1], len(bi))
        mine = sorted(zip((ei[0][sel] - first[k]).tolist(), (rows[ei[1][sel]] - first[k]).tolist()))
        assert mine == sorted(zip(bi.tolist(), bj.tolist()))
        np.testing.assert_allclose(np.sort(rij[sel]), np.sort(bd), rtol=0, atol=1e-5)
    return counts
