"""GPU tests of what k_fused reads from the edge lists between tiles (csrc/fused.hip: tile_bounds, tile_fetch, the centre record, the chunk claim) and of the
short linears' in-place ring reload (csrc/fused_h.h: LATE), DESIGN 4.2c: the next tile's entries are requested through range-checked buffer loads a linear before
the tile ends, also for a tile index beyond the list, so the shapes here are the smallest at which such a fetch can go wrong:

  one_tile          a 6-atom cluster: the whole list is one tile, every fetch but the first lies beyond it
  chunk_tail        27 centres in 5 tiles, claimed in chunks of 4 (AHIP_TCHUNK): the last chunk is one tile long
  cluster_tail      a cluster in an empty box whose first centre has NO neighbour inside r_max and whose last tile holds one centre with 5 edges
  full_tile         simple cubic, 32 neighbours: two centres fill a tile's 64 slots exactly (no lane of the tile is out of range), the last tile holds one
  fcc42_wrap        fcc between the third and fourth shell: 42 edges per centre, one centre per tile, an idle fourth wave in every tile; 400 tiles on fewer workgroups
                    (reserve_wgs = 128), so claims wrap and every workgroup fetches beyond the list's last tile
  eight_wave        fcc out to the fifth shell, 78 neighbours: the 8-wave / 128-slot instance

Positions are jittered.  Bars: the float64 oracle within util.assert_close_to(.., parity_cases.TOL["float32"]) and max|dF| < parity_cases.NORTH_STAR_DF, as for every
model-S system; path=generic on the same file within 2e-5 on the forces (tests/test_gpu_fused.py: two float32-equivalent evaluations of one model, each within
parity_cases.F32EQ_DF = 5e-6 of the oracle on such systems).  Two consecutive evaluations of one model object must give bit-identical per-atom energies (they are summed
in slot order inside a workgroup; the forces go through float64 atomics in arrival order): a fetch that races with its use shows there.  Every figure is printed first."""
import numpy as np
import pytest
import torch

import parity_cases as pc
import util
from oracle import allegro_torch
from pair_allegro_amd import lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

pytestmark = pytest.mark.gpu

GENERIC_DF = 2e-5
_models = {}
_cases = {}


def _lattice(basis, a, reps, jitter, seed):
    cells = np.array([[i, j, k] for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])], dtype=float)
    pos = (cells[:, None, :] + np.asarray(basis, dtype=float)[None, :, :]).reshape(-1, 3) * a
    pos = pos + np.random.RandomState(seed).uniform(-jitter, jitter, size=pos.shape) + 0.25
    return np.diag(np.array(reps, dtype=float) * a), pos


FCC = [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]]


def _geometry(tag):
    """cell, positions (in the order the tiles are packed), r_max"""
    if tag in ("one_tile", "cluster_tail"):
        d = 2.6 / np.sqrt(2.0)                      # octahedron of edge 2.6: every vertex sees the other five
        octa = np.array([[d, 0, 0], [-d, 0, 0], [0, d, 0], [0, -d, 0], [0, 0, d], [0, 0, -d]])
        octa = octa + np.random.RandomState(11).uniform(-0.08, 0.08, size=octa.shape) + 15.0
        pos = octa if tag == "one_tile" else np.concatenate([[[4.0, 5.0, 6.0]], octa])      # the lone atom first: tile 0 = lone + five, tile 1 = the sixth
        return np.eye(3) * 30.0, pos, 5.0
    if tag == "chunk_tail":                         # simple cubic, a = 4: 6 neighbours, six centres per tile -> 27 centres in 5 tiles
        cell, pos = _lattice([[0, 0, 0]], 4.0, (3, 3, 3), 0.1, 7)
        return cell, pos, 5.0
    if tag == "full_tile":                          # simple cubic, a = 2.35: shells at 2.35, 3.32, 4.07, 4.70 | 5.25 -> 32 neighbours
        cell, pos = _lattice([[0, 0, 0]], 2.35, (3, 3, 3), 0.03, 5)
        return cell, pos, 5.0
    if tag == "fcc42_wrap":                         # fcc, a = 3.7: shells at 2.62, 3.70, 4.53 | 5.23 -> 42 neighbours
        cell, pos = _lattice(FCC, 3.7, (5, 5, 4), 0.05, 3)
        return cell, pos, 5.0
    if tag == "eight_wave":                         # the same lattice out to 5.85 | 6.41 -> 78 neighbours
        cell, pos = _lattice(FCC, 3.7, (2, 2, 2), 0.05, 9)
        return cell, pos, 6.1
    raise KeyError(tag)


def _model(model_dir, r_max):
    if r_max not in _models:
        cfg = model_file.model_S(type_names=["Cu"], r_max=r_max, avg_num_neighbors=30.0)
        w = model_file.init_weights(cfg)
        path = f"{model_dir}/queue_S_r{r_max}.nequip.pth"
        allegro_torch.export_nequip_pth(path, cfg, w)
        _models[r_max] = (path, cfg, w)
    return _models[r_max]


def _case(model_dir, tag):
    """geometry, model file and float64 oracle result: computed once, shared, never changed"""
    if tag not in _cases:
        cell, pos, r_max = _geometry(tag)
        path, cfg, w = _model(model_dir, r_max)
        types = np.ones(len(pos), dtype=np.int32)
        ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, ["Cu"])
        bi = util.glue.brute_force_edges(cell, pos, r_max)[0]
        _cases[tag] = dict(cell=cell, pos=pos, types=types, path=path, ref=ref, deg=np.bincount(bi, minlength=len(pos)))
    return _cases[tag]


def _twice(hip_lib, c, options):
    """two consecutive evaluations of one model object on the fused path: (result of the first as util.run_pair gives it, per-atom energies of both, tiles)"""
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"], "Cu"], ntypes=1)
    for k, v in dict(options, path="fused").items():
        pair.model.set_option(k, v)
    pair.init_style()
    try:
        rs = lmp_like.build_rank_system(c["cell"], c["pos"], c["types"], pair.init_one(1, 1) + 1.0)
        out = []
        for _ in range(2):
            atom = atom_from_rank_system(rs, 1)
            pair.compute(atom, list_from_rank_system(rs))
            assert pair.model.last_path == "fused_f16x2", pair.model.last_path
            n = len(c["pos"])
            forces = np.zeros((n, 3))
            np.add.at(forces, rs.tag - 1, atom.f)
            eatom = np.zeros(n)
            eatom[rs.tag[: rs.nlocal] - 1] = pair.eatom[: rs.nlocal]
            out.append(dict(forces=forces, eatom=eatom, pe=float(pair.eng_vdwl), virial=np.array(pair.virial, dtype=float)))
        used, total = pair.model.tile_occupancy()
        return out[0], out[1], int(used), int(total), int(pair.model.last_max_degree)
    finally:
        pair.model.close()


def _check(hip_lib, model_dir, tag, options=None, slots=64):
    c = _case(model_dir, tag)
    first, second, used, total, maxdeg = _twice(hip_lib, c, options or {})
    gen = util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], ["Cu"], options={"path": "generic"})
    assert gen["info"]["path"] == "generic_f32"
    err = float(np.abs(first["forces"] - c["ref"]["forces"]).max())
    dgen = float(np.abs(first["forces"] - gen["forces"]).max())
    nbit = int((first["eatom"] != second["eatom"]).sum())
    print(f"{tag}: {len(c['pos'])} atoms, degrees {c['deg'].min()}..{c['deg'].max()}, {used} edges in {total // slots} tiles of {slots} slots; max|dF| vs f64 oracle {err:.3e}, "
          f"vs path=generic {dgen:.3e} (max|F| {np.abs(c['ref']['forces']).max():.3f}); per-atom energies that differ between two evaluations: {nbit}")
    assert used == int(c["deg"].sum()) and total % slots == 0 and maxdeg == int(c["deg"].max())
    util.assert_close_to(first, c["ref"], pc.TOL["float32"], what=tag)
    assert err < pc.NORTH_STAR_DF
    assert dgen < GENERIC_DF
    np.testing.assert_allclose(first["eatom"], gen["eatom"], atol=pc.TOL["float32"], rtol=pc.TOL["float32"])
    assert nbit == 0
    assert np.abs(second["forces"] - first["forces"]).max() <= 1e-9 * max(np.abs(first["forces"]).max(), 1e-30)      # (float64 atomics in arrival order: tests/test_gpu_soak.py)
    return c, total // slots


def test_list_of_one_tile(hip_lib, model_dir):
    c, tiles = _check(hip_lib, model_dir, "one_tile")
    assert tiles == 1 and (c["deg"] == 5).all()


def test_last_chunk_shorter_than_a_claim(hip_lib, model_dir, monkeypatch):
    monkeypatch.setenv("AHIP_TCHUNK", "4")
    c, tiles = _check(hip_lib, model_dir, "chunk_tail")
    assert (c["deg"] == 6).all() and tiles == 5 and tiles % 4 != 0


def test_cluster_with_a_lone_atom_and_a_one_centre_last_tile(hip_lib, model_dir):
    c, tiles = _check(hip_lib, model_dir, "cluster_tail")
    assert c["deg"][0] == 0 and (c["deg"][1:] == 5).all()
    assert tiles == 2                                  # six centres (the lone atom and five of the cluster), then one centre with 5 edges
    assert np.abs(c["ref"]["forces"][0]).max() == 0.0  # the lone atom feels no force


def test_tile_of_exactly_64_edges(hip_lib, model_dir):
    c, tiles = _check(hip_lib, model_dir, "full_tile")
    assert (c["deg"] == 32).all() and tiles == 14      # 13 tiles of two centres = 64 edges, one of a single centre


def test_idle_wave_and_more_tiles_than_workgroups(hip_lib, model_dir):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    grid = 2 * ncu - 128
    c, tiles = _check(hip_lib, model_dir, "fcc42_wrap", {"reserve_wgs": "128"})
    print(f"fcc42_wrap: {tiles} tiles on {grid} workgroups of {ncu} CUs")
    assert (c["deg"] == 42).all() and tiles == len(c["pos"])      # one centre per tile: slots 42..63, i.e. the whole fourth wave, hold no edge
    assert tiles > grid > 0, (tiles, grid)


def test_eight_wave_shape(hip_lib, model_dir):
    c, tiles = _check(hip_lib, model_dir, "eight_wave", slots=128)
    assert (c["deg"] == 78).all() and tiles == len(c["pos"])
