"""Output "atomic_virial" (per-atom virial, [nall][9]) on the CPU emulation of the layer-at-a-time kernels, float64: against the oracle's
edge gradients, against the `virial` output (sum rule), against finite differences of the per-atom energies (the neighbour convention
itself), through `compute allegro/atom` on rank grids, and no change anywhere without the request."""
import numpy as np
import pytest

import atomic_virial_ref as av
import util
from pair_allegro_amd import capi, lmp_like, model_file
from pair_allegro_amd.compute import ComputeAllegro
from pair_allegro_amd.pair import LammpsError, PairAllegro, atom_from_rank_system, list_from_rank_system

CASES = ("Cu2AgO4_r5", "Si64_r5")
SMALL = dict(num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8, avg_num_neighbors=30.0)


def _model(model_dir, kind, g, dtype="float64"):
    names = sorted(set(g["symbols"]))
    factory = model_file.model_S if kind == "S" else model_file.model_L
    cfg = factory(type_names=names, model_dtype=dtype, **SMALL)
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/av_{kind}_{g['tag']}_{dtype}.ahip"
    model_file.save_ahip(path, cfg, w)
    return cfg, w, path, names


def _types(g, names):
    return np.array([names.index(s) + 1 for s in g["symbols"]], dtype=np.int32)


@pytest.mark.parametrize("kind", ["S", "L2"])
@pytest.mark.parametrize("case", CASES)
def test_atomic_virial_oracle_parity_and_sum_rule(emu_lib, model_dir, case, kind):
    g = util.load_golden(case)
    cfg, w, path, names = _model(model_dir, kind, g)
    assert cfg["l_max"] == (1 if kind == "S" else 2)
    rs = av.rank_system(cfg, g["cell"], g["pos"], _types(g, names))
    ref = av.oracle_w(cfg, w, rs, names)
    res = av.run(emu_lib, path, rs, names)
    assert res["path"] == "generic_f64"
    assert res["W"].shape == (rs.nall, 9)
    scale = np.abs(ref).max()
    assert scale > 0
    err = np.abs(res["W"] - ref).max(axis=1)
    assert err.max() <= 1e-10 * scale, (np.argmax(err), err.max(), scale)
    # sum rule: symmetrised sum over all rows (ghosts included) = the virial output of the same call
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    assert np.abs(av.sym_sum(res["W"]) - res["virial"]).max() <= 1e-12 * rowscale


def test_atomic_virial_finite_difference(emu_lib, model_dir):
    """Independent of the oracle: W_k[:, b] = -sum_{i != k} d_ik dE_i/dx_k[b] with d_ik the minimum image x_k - x_i (the box of 10.862 A
    exceeds 2 r_max: one image per pair), dE_i/dx_k from central differences of the per-atom energies."""
    g = util.load_golden("Si64_r5")
    cfg, w, path, names = _model(model_dir, "S", g)
    types = _types(g, names)
    L = np.diag(g["cell"])
    assert np.allclose(g["cell"], np.diag(L)) and L.min() > 2 * cfg["r_max"]
    pos = np.asarray(g["pos"], dtype=np.float64)
    n = len(pos)

    def eatom_by_tag(p):
        rs = av.rank_system(cfg, g["cell"], p, types)
        r = av.run(emu_lib, path, rs, names, register=False)
        e = np.zeros(n)
        e[rs.tag[: rs.nlocal] - 1] = r["eatom"]
        return e

    rs = av.rank_system(cfg, g["cell"], pos, types)
    res = av.run(emu_lib, path, rs, names)
    wf = np.zeros((n, 9))
    np.add.at(wf, rs.tag - 1, res["W"])                     # ghost rows onto their owners
    h = 1e-4
    for k in (0, 37):
        want = np.zeros((3, 3))
        for b in range(3):
            pp, pm = pos.copy(), pos.copy()
            pp[k, b] += h
            pm[k, b] -= h
            de = (eatom_by_tag(pp) - eatom_by_tag(pm)) / (2 * h)     # dE_i / dx_k[b] for every i
            d = pos[k] - pos
            d -= L * np.round(d / L)
            de[k] = 0.0
            want[:, b] = -(d * de[:, None]).sum(axis=0)
        got = wf[k].reshape(3, 3)
        assert np.abs(want).max() > 1e-3
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (k, got, want)


def _fold(lib, path, g, types, names, grid):
    """`compute av all allegro/atom atomic_virial 9 1` on every rank of the grid, reverse-communicated by tag."""
    n = len(g["pos"])
    out = np.zeros((n, 9))
    for r in lmp_like.grid_ranks(grid):
        pair = PairAllegro(me=0, nprocs=1, lib=lib, quiet=True)
        pair.settings([])
        pair.coeff(["*", "*", path] + list(names), ntypes=len(names))
        c = ComputeAllegro(["av", "all", "allegro/atom", "atomic_virial", "9", "1"], pair)
        pair.init_style()
        rs = lmp_like.build_rank_system(g["cell"], g["pos"], types, pair.init_one(1, 1) + av.SKIN, grid=grid, rank=r)
        atom = atom_from_rank_system(rs, len(names))
        pair.compute(atom, list_from_rank_system(rs))
        arr = c.compute_peratom(rs.nlocal, rs.nall)
        if rs.nlocal:
            buf = c.pack_reverse_comm(rs.nghost, rs.nlocal)
            np.add.at(out, rs.tag[: rs.nlocal] - 1, arr[: rs.nlocal])
            np.add.at(out, rs.tag[rs.nlocal:] - 1, buf.reshape(-1, 9))
        pair.model.close()
    return out


def test_atomic_virial_compute_on_rank_grids(emu_lib, model_dir):
    g = util.load_golden("Cu2AgO4_r5")
    cfg, w, path, names = _model(model_dir, "L2", g)
    types = _types(g, names)
    rs = av.rank_system(cfg, g["cell"], g["pos"], types)
    ref = np.zeros((len(g["pos"]), 9))
    np.add.at(ref, rs.tag - 1, av.oracle_w(cfg, w, rs, names))
    one = _fold(emu_lib, path, g, types, names, (1, 1, 1))
    scale = np.abs(ref).max()
    assert np.abs(one - ref).max() <= 1e-10 * scale
    for grid in ((2, 1, 1), (2, 2, 1)):
        assert np.abs(_fold(emu_lib, path, g, types, names, grid) - one).max() <= 1e-10 * scale, grid


def test_atomic_virial_absent_without_request(emu_lib, model_dir):
    g = util.load_golden("Cu2AgO4_r5")
    cfg, w, path, names = _model(model_dir, "S", g)
    rs = av.rank_system(cfg, g["cell"], g["pos"], _types(g, names))
    with_w = av.run(emu_lib, path, rs, names)
    without = av.run(emu_lib, path, rs, names, register=False)
    for q in ("f", "eatom", "virial"):
        np.testing.assert_allclose(with_w[q], without[q], rtol=1e-12, atol=1e-12 * np.abs(without[q]).max())
    np.testing.assert_allclose(with_w["pe"], without["pe"], rtol=1e-12)
    # not registered: not stored (the library's StateError through the pair style)
    pair = PairAllegro(me=0, nprocs=1, lib=emu_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", path] + list(names), ntypes=len(names))
    pair.init_style()
    pair.compute(atom_from_rank_system(rs, len(names)), list_from_rank_system(rs))
    with pytest.raises(LammpsError, match="output 'atomic_virial' is not stored"):
        pair.custom_output("atomic_virial")
    with pytest.raises(capi.AhipError):
        pair.model.output_get("atomic_virial")
    pair.model.close()
