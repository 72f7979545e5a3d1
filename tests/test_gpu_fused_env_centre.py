"""GPU tests of k_fused's environment backward once per centre (csrc/fused.hip; option env_backward = auto | centre | edge).

On the f16x2 instances of the 4-wave shape a tile of up to 3 centres evaluates the transposed environment linear on the centres' reduced gradients (12 columns on one
wave) instead of on every edge; tiles of 4..6 centres, the 8-wave shape and every other arithmetic keep the per-edge linear, which `edge` forces for every tile.  The two
forms differ in rounding order only, so every case holds each setting against the float64 oracle with the bars of the existing fused tests: max|dF| below
parity_cases.F32EQ_DF, energies and virial util.assert_close_to(.., 5e-4), path fused_f16x2 (the two shapes without the form: unchanged results, and parity_cases.NORTH_STAR_DF as in
their existing tests).  Every figure is printed before it is asserted.

Geometries (jittered, fixed seeds; the float64 oracle runs once per (geometry, model) and is shared):
  Si64        the 64-atom Si golden, r_max 5: 28 edges per centre, two centres per tile
  Si216       diamond Si, 3 x 3 x 3 cells, r_max 5: the same tiles, more than one workgroup's worth
  Li3PO4      the 128-atom gamma-Li3PO4 golden, three model types whose energy scales lie in different binades (8, 1/4, 1/64): one centre per tile, centres with
              33..48 edges leave the tile's fourth wave idle, and the backward scale of a centre's type is not that of its neighbours'
  Si64_r4     diamond Si, 2 x 2 x 2 cells, r_max 4: 16 edges per centre, four centres per tile: `auto` takes the per-edge linear
  mixed       a diamond slab (28 edges per centre in the bulk) followed in the list by a simple-cubic slab (6 edges per centre, six centres per tile), 600 atoms: both forms in one launch
  Si1728      diamond Si, 6 x 6 x 6 cells: 864 tiles on 2 CUs - 128 workgroups (reserve_wgs = 128)
  fcc78       fcc out to the fifth shell, 78 neighbours: the 8-wave shape, which has no per-centre form

Measured on the MI355X (max|dF| against the float64 oracle, eV/A; per centre / per edge): Si64 with 1, 2, 3 layers 2.4e-6 / 2.5e-6, 7.5e-7 / 8.6e-7, 7.1e-7 / 6.8e-7; latent MLP
depth 1 and 3: 2.2e-6 / 2.3e-6, 3.8e-7 / 4.0e-7; Si216 9.9e-7 / 1.1e-6; Li3PO4 with 2 and 3 layers 5.2e-7 / 4.7e-7, 6.7e-7 / 6.5e-7; mixed 1.5e-6 / 1.5e-6; Si64 at r_max 4 1.2e-6
under every setting; Si1728 1.2e-6, no per-atom energy differs between two launches; 8-wave shape 9.0e-7 and fused_arith=f32 1.6e-6 under both settings."""
import numpy as np
import pytest
import torch

import atomic_virial_ref as av
import parity_cases as pc
import util
from oracle import allegro_torch
from pair_allegro_amd import lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

pytestmark = pytest.mark.gpu

MODES = ["auto", "centre", "edge"]
LI_SCALES = [8.0, 0.25, 0.015625]
_cases = {}


def _geometry(tag):
    """cell, positions, symbols, model type names, r_max"""
    if tag == "Si64":
        g = util.load_golden("Si64_r5")
        return g["cell"], g["pos"], g["symbols"], ["Si"], 5.0
    if tag in ("Si216", "Si1728", "Si64_r4"):
        n = {"Si216": 3, "Si1728": 6, "Si64_r4": 2}[tag]
        cell, pos, _ = lmp_like.diamond_si(n, jitter=0.02 if tag == "Si64_r4" else 0.05, seed=n)      # (r_max 4 lies 0.16 A beyond the second shell)
        return cell, pos, ["Si"] * len(pos), ["Si"], 4.0 if tag == "Si64_r4" else 5.0
    if tag == "Li3PO4":
        g = util.load_golden("Li3PO4_128_r5")
        return g["cell"], g["pos"], g["symbols"], ["Li", "P", "O"], 5.0
    if tag == "mixed":
        # diamond cells 0..2 in z, then a simple-cubic slab of spacing L / 4 = 4.07 A (second shell at 5.76 A), 7 A of vacuum on either side of it
        _, dia, _ = lmp_like.diamond_si(3, jitter=0.0)
        L = 3 * 5.431
        a = L / 4.0
        sc = np.array([[i, j, k] for k in range(24) for j in range(4) for i in range(4)], dtype=float) * a + [0.5, 0.5, L + 7.0]
        pos = np.concatenate([dia + [0.3, 0.3, 0.3], sc])
        pos = pos + np.random.RandomState(17).normal(0.0, 0.04, size=pos.shape)
        cell = np.diag([L, L, L + 7.0 + 24 * a + 7.0 - a])
        return cell, pos, ["Si"] * len(pos), ["Si"], 5.0
    if tag == "fcc78":
        fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
        cells = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=float)
        pos = (cells[:, None, :] + fcc[None, :, :]).reshape(-1, 3) * 3.7
        pos = pos + np.random.RandomState(9).uniform(-0.05, 0.05, size=pos.shape) + 0.25
        return np.eye(3) * 7.4, pos, ["Cu"] * len(pos), ["Cu"], 6.1
    raise KeyError(tag)


def _case(model_dir, tag, **over):
    """Geometry, model file and float64 oracle result of model S with `over` on geometry `tag`: built once, shared, never changed."""
    key = (tag, tuple(sorted(over.items())))
    if key not in _cases:
        cell, pos, symbols, tn, r_max = _geometry(tag)
        cell, pos = np.asarray(cell, dtype=float), np.asarray(pos, dtype=float)
        deg = np.bincount(util.glue.brute_force_edges(cell, pos, r_max)[0], minlength=len(pos))
        cfg = model_file.model_S(**dict(dict(type_names=tn, r_max=r_max, avg_num_neighbors=float(deg.mean())), **over))
        w = model_file.init_weights(cfg)
        if tag == "Li3PO4":
            w["scale"] = np.array(LI_SCALES)
        name = "envc_" + tag + "".join(f"_{k}{v}" for k, v in sorted(over.items()))
        path = f"{model_dir}/{name}.nequip.pth"
        allegro_torch.export_nequip_pth(path, cfg, w)
        names = sorted(set(symbols))
        types = np.array([names.index(s) + 1 for s in symbols], dtype=np.int32)
        ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, names)
        _cases[key] = dict(tag=tag, cfg=cfg, w=w, path=path, cell=cell, pos=pos, types=types, names=names, ref=ref, deg=deg)
    return _cases[key]


def _held(hip_lib, c, mode, what, extra=None, path="fused_f16x2"):
    """One evaluation under env_backward = mode, held against the float64 oracle."""
    res = util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"], options=dict(extra or {}, env_backward=mode))
    err = float(np.abs(res["forces"] - c["ref"]["forces"]).max())
    print(f"{what}, env_backward={mode}: {res['info']['path']}, {len(c['pos'])} atoms, degrees {c['deg'].min()}..{c['deg'].max()}, max|dF| vs f64 oracle {err:.3e} "
          f"(max|F| {np.abs(c['ref']['forces']).max():.3f}), |dE| {abs(res['pe'] - float(c['ref']['pe'])):.3e}")
    assert res["info"]["path"] == path, res["info"]
    util.assert_close_to(res, c["ref"], 5e-4, what=f"{what} env_backward={mode}")
    assert err < pc.F32EQ_DF, (what, mode, err)
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nl", [1, 2, 3])
def test_two_centres_per_tile_every_layer_count(hip_lib, model_dir, nl, mode):
    c = _case(model_dir, "Si64", num_layers=nl)
    assert (c["deg"] > 21).all() and (c["deg"] <= 32).all()          # two centres fill a 64-slot tile, three do not fit
    _held(hip_lib, c, mode, f"Si64, {nl} layers")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("md", [1, 3])
def test_two_centres_per_tile_latent_mlp_depth(hip_lib, model_dir, md, mode):
    """The linear in front of the skipped one in the last layer (the dcat linear, which carries the stream jump) has another length at every MLP depth."""
    c = _case(model_dir, "Si64", num_layers=2, mlp_depth=md)
    _held(hip_lib, c, mode, f"Si64, 2 layers, latent MLP depth {md}")


@pytest.mark.parametrize("mode", MODES)
def test_jittered_box(hip_lib, model_dir, mode):
    c = _case(model_dir, "Si216")
    _held(hip_lib, c, mode, "Si216")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nl", [2, 3])
def test_one_centre_per_tile_idle_wave_and_centre_type_scales(hip_lib, model_dir, nl, mode):
    c = _case(model_dir, "Li3PO4", num_layers=nl)
    idle = int(((c["deg"] > 32) & (c["deg"] <= 48)).sum())
    print(f"Li3PO4: {idle} of {len(c['pos'])} centres have 33..48 edges; types {np.bincount(c['types'])[1:]}, energy scales {LI_SCALES}")
    assert idle > 0 and c["deg"].max() <= 64                                   # tiles of one centre whose fourth wave holds no edge
    assert len(c["names"]) == 3 and len(set(np.frexp(LI_SCALES)[1])) == 3        # three binades: three backward scales
    _held(hip_lib, c, mode, f"Li3PO4, {nl} layers")


@pytest.mark.parametrize("mode", MODES)
def test_four_centres_per_tile_takes_the_per_edge_linear(hip_lib, model_dir, mode):
    c = _case(model_dir, "Si64_r4")
    assert (c["deg"] == 16).all()                                      # four centres = 64 edges: no tile of this list has fewer than 4 centres
    _held(hip_lib, c, mode, "Si64 at r_max 4")


@pytest.mark.parametrize("mode", MODES)
def test_both_forms_in_one_launch(hip_lib, model_dir, mode):
    c = _case(model_dir, "mixed")
    nd = 216
    dense, sparse = c["deg"][:nd], c["deg"][nd:]
    bulk = int((dense >= 22).sum())
    print(f"mixed: diamond slab degrees {dense.min()}..{dense.max()} ({bulk} centres with >= 22 edges, at most two of which fit a tile), "
          f"simple-cubic slab degrees {sparse.min()}..{sparse.max()}")
    assert bulk >= 16 and (dense[8 * 1:8 * 2] >= 22).all() and sparse.max() <= 10 and len(sparse) == 384          # (cell (0, 0, 1): eight consecutive centres of the bulk)
    _held(hip_lib, c, mode, "mixed")
    # the tiles of the launch: some hold more than 3 centres (there are fewer tiles than a third of the centres), and consecutive centres of >= 22 edges go two to a tile
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"], "Si"], ntypes=1)
    pair.model.set_option("env_backward", mode)
    pair.init_style()
    try:
        rs = lmp_like.build_rank_system(c["cell"], c["pos"], c["types"], pair.init_one(1, 1) + 1.0)
        pair.compute(atom_from_rank_system(rs, 1), list_from_rank_system(rs))
        used, total = pair.model.tile_occupancy()
    finally:
        pair.model.close()
    tiles = total // 64
    print(f"mixed: {used} edges in {tiles} tiles")
    assert used == int(c["deg"].sum()) and total % 64 == 0
    assert 3 * tiles < len(c["pos"]), (tiles, len(c["pos"]))


def test_more_tiles_than_workgroups(hip_lib, model_dir):
    """Every workgroup runs several tiles, each behind a tile whose waves 1..3 skipped two linears: a weight ring left out of phase shows from the second tile on.  Two
    consecutive launches of one model object: per-atom energies bit for bit (summed in slot order inside a workgroup), forces within 1e-9 of max|F| (float64 atomics in
    arrival order; tests/test_gpu_soak.py), and the first within the bars of the oracle."""
    c = _case(model_dir, "Si1728")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    grid = 2 * ncu - 128
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"], "Si"], ntypes=1)
    pair.model.set_option("reserve_wgs", "128")
    pair.model.set_option("env_backward", "auto")
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
    finally:
        pair.model.close()
    first, second = out
    tiles = total // 64
    err = float(np.abs(first["forces"] - c["ref"]["forces"]).max())
    nbit = int((first["eatom"] != second["eatom"]).sum())
    print(f"Si1728: {used} edges in {tiles} tiles on {grid} workgroups of {ncu} CUs; max|dF| vs f64 oracle {err:.3e}; per-atom energies that differ between two launches: {nbit}; "
          f"max|dF| between them {np.abs(second['forces'] - first['forces']).max():.3e}")
    assert tiles > 2 * grid > 0, (tiles, grid)
    util.assert_close_to(first, c["ref"], 5e-4, what="Si1728")
    assert err < pc.F32EQ_DF
    assert nbit == 0
    assert np.abs(second["forces"] - first["forces"]).max() <= 1e-9 * np.abs(first["forces"]).max()


@pytest.mark.parametrize("mode", ["auto", "edge"])
def test_atomic_virial_instance(hip_lib, model_dir, mode):
    """The VAR_VA twin of the two-layer instance: output atomic_virial against the float64 oracle's W, bars of tests/test_gpu_atomic_virial.py (2e-5 of max|W|; the
    symmetrised sum of W against the virial at 1e-6 of the row scale)."""
    c = _case(model_dir, "Si64", num_layers=2)
    path = f"{model_dir}/envc_av_Si64.ahip"
    model_file.save_ahip(path, c["cfg"], c["w"])
    rs = av.rank_system(c["cfg"], c["cell"], c["pos"], c["types"])
    if "W" not in c:
        c["W"] = av.oracle_w(c["cfg"], c["w"], rs, c["names"])
    res = av.run(hip_lib, path, rs, c["names"], options={"path": "fused", "fused_arith": "f16x2", "env_backward": mode})
    scale = np.abs(c["W"]).max()
    err = np.abs(res["W"] - c["W"]).max()
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    dv = np.abs(av.sym_sum(res["W"]) - res["virial"]).max()
    print(f"atomic_virial Si64 env_backward={mode}: {res['path']}, max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert res["path"] == "fused_f16x2"
    assert res["W"].shape == c["W"].shape
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)


@pytest.mark.parametrize("what,tag,extra,path", [("8-wave shape", "fcc78", {}, "fused_f16x2"), ("fused_arith=f32", "Si64", {"path": "fused", "fused_arith": "f32"}, "fused_f32")])
def test_instances_without_the_form_do_not_change(hip_lib, model_dir, what, tag, extra, path):
    """The 8-wave shape and the float32 arithmetic have no per-centre form: the option changes nothing -- per-atom energies bit for bit, forces within 1e-9 of max|F|."""
    c = _case(model_dir, tag, num_layers=2)
    if tag == "fcc78":
        assert (c["deg"] == 78).all()
    runs = {}
    for mode in ("centre", "edge"):
        res = util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"], options=dict(extra, env_backward=mode))
        err = float(np.abs(res["forces"] - c["ref"]["forces"]).max())
        print(f"{what}, env_backward={mode}: {res['info']['path']}, max degree {res['info']['max_degree']}, max|dF| vs f64 oracle {err:.3e}")
        assert res["info"]["path"] == path
        util.assert_close_to(res, c["ref"], 5e-4, what=what)
        assert err < pc.NORTH_STAR_DF                                  # (the bar of the existing tests of these two shapes: tests/test_gpu_fused_queue.py, tests/test_gpu_soak.py)
        runs[mode] = res
    assert int((runs["centre"]["eatom"] != runs["edge"]["eatom"]).sum()) == 0
    assert np.abs(runs["centre"]["forces"] - runs["edge"]["forces"]).max() <= 1e-9 * np.abs(runs["edge"]["forces"]).max()


def test_unknown_value_is_an_argument_error(hip_lib, model_dir):
    c = _case(model_dir, "Si64", num_layers=2)
    with pytest.raises(Exception, match="env_backward"):
        util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"], options={"env_backward": "atom"})
