"""Fused kernels for models of more than 16 types, on the MI355X: the fused side runs on the model restricted to its active types (tests/active_types_cases.py: a
20-type model with O, Cu and Ag at 7, 18 and 19, and its 3-type slice written as a file of its own, the "twin").  The 20-type file and the twin hand the kernels
the same bytes, so they are compared by the criterion of tests/test_gpu_soak.py (per-atom energies bit for bit, forces to 1e-9 of max|F|, energy to 1e-12): a
difference means a wrong slot, not rounding.  Against the float64 oracle the bars are those of tests/fused_shape_cases.py."""
import numpy as np
import pytest

import active_types_cases as atc
import atomic_virial_ref as av
import dense_centres_cases as dc
import fused_shape_cases as fsc
import parity_cases as pc
import util
from pair_allegro_amd import capi, lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

pytestmark = pytest.mark.gpu

KERNELS3 = ["k_fused", "k_fused_lx", "k_fused_lx2"]
NEW_REASON = "at most 16 active model types (17 of the model's 20 are mapped)"


def _pair20(model_dir, kernel, **kw):
    return atc.pair20(model_dir, kernel, num_layers=2, **kw)


def _host_eval(m, cfg, rs, names):
    """One ahip_compute on an open model; per-global-atom forces and energies like util.run_pair."""
    mapper, cm = util.type_mapper_and_cutoffs(cfg, names)
    m.neigh_update_csr(rs.nall, rs.ilist, rs.offsets, rs.flat)
    f = np.zeros_like(rs.x)
    ea = np.zeros(rs.nall)
    eng, vir = m.compute(rs.nlocal, rs.nghost, rs.x, rs.type, mapper, cm, f, ea)
    n = int(rs.tag.max())
    forces = np.zeros((n, 3))
    np.add.at(forces, rs.tag - 1, f)
    eatom = np.zeros(n)
    eatom[rs.tag[: rs.nlocal] - 1] = ea[: rs.nlocal]
    return dict(forces=forces, eatom=eatom, pe=eng, virial=vir, info=dict(path=m.last_path), active=m.get_active_types())


def _rank_system(c, types=None, skin=1.0):
    return lmp_like.build_rank_system(c["cell"], c["pos"], c["types"] if types is None else types, c["cfg"]["r_max"] + skin)


# ---- 1: twin equality, the test that fails without the feature (the 20-type file takes generic_f32 there) ----
@pytest.mark.parametrize("kernel", KERNELS3)
def test_20_type_model_runs_fused_and_equals_its_slice(hip_lib, model_dir, kernel):
    full, twin = _pair20(model_dir, kernel)
    fsc.assert_bars(hip_lib, full, twin, f"20 types, 3 active, {kernel}")
    assert twin["fused"]["info"]["path"] == "fused_f16x2"
    atc.assert_same_run(full["fused"], twin["fused"], f"{kernel}: 20-type file vs its slice")
    # the layer-at-a-time kernels see the model as loaded
    util.assert_close_to(full["generic"], full["ref"], 5e-4, what="path=generic, 20 types")


# ---- 2: pair_coeff names in another order, one of them twice ----
@pytest.mark.parametrize("kernel", ["k_fused", "k_fused_lx2"])
def test_mapper_order_and_duplicates(hip_lib, model_dir, kernel):
    full, twin = _pair20(model_dir, kernel)
    fsc.measure(hip_lib, full)
    names4 = ["O", "Ag", "Cu", "O"]
    _cell, _pos, symbols, *_ = fsc.geometry("Cu2AgO4")
    types4, seen_o = [], 0
    for s in symbols:                          # the O atoms alternate between LAMMPS types 1 and 4
        if s == "O":
            types4.append(1 if seen_o % 2 == 0 else 4)
            seen_o += 1
        else:
            types4.append(names4.index(s) + 1)
    types4 = np.array(types4, dtype=np.int32)
    assert set(types4) == {1, 2, 3, 4}
    res = util.run_pair(hip_lib, full["path"], full["cell"], full["pos"], types4, names4)
    assert res["info"]["path"] == "fused_f16x2"
    atc.assert_same_run(res, full["fused"], f"{kernel}: pair_coeff O Ag Cu O")


# ---- 3: sixteen active types run fused (slot 15 in use), seventeen do not ----
def test_sixteen_active_types_fused_seventeen_generic(hip_lib, model_dir):
    _cell, pos, *_ = fsc.geometry("CuPd256")
    names16, names17 = atc.NAMES20[4:20], atc.NAMES20[3:20]
    sym16 = [names16[i % 16] for i in range(len(pos))]
    full, twin = atc.pair20(model_dir, "k_fused", tag="CuPd256", names=names16, symbols=sym16, with_ref=False, key_extra="rr16")
    m = capi.Model(full["path"], 0, hip_lib)
    a = _host_eval(m, full["cfg"], _rank_system(full), names16)
    m.close()
    assert a["info"]["path"] == "fused_f16x2" and a["active"] == list(range(4, 20))      # Ag = model type 19 = slot 15
    assert (full["types"] == 16).any()
    b = util.run_pair(hip_lib, twin["path"], twin["cell"], twin["pos"], twin["types"], names16)
    assert b["info"]["path"] == "fused_f16x2"
    atc.assert_same_run(a, b, "16 active types of 20 vs the 16-type slice")
    # seventeen mapped names: the layer-at-a-time kernels, and path=fused says why
    sym17 = [names17[i % 17] for i in range(len(pos))]
    types17 = np.array([names17.index(s) + 1 for s in sym17], dtype=np.int32)
    m = capi.Model(full["path"], 0, hip_lib)
    rs17 = _rank_system(full, types17)
    c = _host_eval(m, full["cfg"], rs17, names17)
    assert c["info"]["path"] == "generic_f32" and c["active"] == list(range(3, 20))
    m.set_option("path", "fused")
    with pytest.raises(capi.AhipError) as e:
        _host_eval(m, full["cfg"], rs17, names17)
    assert e.value.code == capi.AHIP_ERR_UNSUPPORTED and NEW_REASON in e.value.msg, e.value.msg
    m.close()


# ---- 4: compact slots on the fused kernel and full types on the layer-at-a-time kernels in one call ----
def test_dense_centres_split_with_20_types(hip_lib, model_dir):
    names = ["Cu", "Ag"]                       # Cu: the bulk at 54 edges, Ag: four centres at 134 (tests/dense_centres_cases.py: S_light4)
    cell, pos, types = dc.fcc(dc.HEAVY)
    T = len(atc.NAMES20)
    pcut = np.full((T, T), dc.R54)
    pcut[atc.NAMES20.index("Ag"), :] = dc.R134
    cfg = model_file.model_S(type_names=list(atc.NAMES20), r_max=dc.R134, per_edge_type_cutoff=pcut.tolist(), avg_num_neighbors=56.0)
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/at_dense20.ahip"
    model_file.save_ahip(path, cfg, w)
    ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, names, skin=1.0)
    res = util.run_pair(hip_lib, path, cell, pos, types, names, options={"dense_centres": "split"})
    gen = util.run_pair(hip_lib, path, cell, pos, types, names, options={"path": "generic"})
    assert res["info"]["path"] in pc.FUSED_F32EQ and gen["info"]["path"] == "generic_f32"
    assert res["info"]["max_degree"] > 128
    m = capi.Model(path, 0, hip_lib)
    m.set_option("dense_centres", "split")
    one = _host_eval(m, cfg, lmp_like.build_rank_system(cell, pos, types, cfg["r_max"] + 1.0), names)
    assert one["active"] == [18, 19] and m.last_heavy_centres[0] == len(dc.HEAVY)
    m.close()
    tol = pc.TOL["float32"]
    util.assert_close_to(res, ref, tol, what="split, 20 types vs the float64 oracle")
    assert np.abs(res["forces"] - ref["forces"]).max() < pc.NORTH_STAR_DF
    util.assert_close_to(res, gen, tol, what="split, 20 types vs path=generic")


# ---- 5: the other writers of fused-side types ----
@pytest.mark.parametrize("kernel,options,skin", [
    ("k_fused", {"tile_pack": "separate"}, 1.0),                       # k_pack_small / k_centre_info write the centre records
    ("k_fused_lx", {"tile_pack": "separate"}, 1.0),
    ("k_fused", {}, 2.6),                                              # list rows above 128 entries, degrees <= 64: two-pass edge build, k_edge_types
    ("k_fused_lx2", {}, 2.6),
    ("k_fused", {"fused_tb": "mlp", "fused_arith": "f32"}, 1.0),       # the o_pair table of the two-body MLP
])
def test_other_writers_equal_the_slice(hip_lib, model_dir, kernel, options, skin):
    full, twin = _pair20(model_dir, kernel)
    a = util.run_pair(hip_lib, full["path"], full["cell"], full["pos"], full["types"], full["names"], skin=skin, options=options)
    b = util.run_pair(hip_lib, twin["path"], twin["cell"], twin["pos"], twin["types"], twin["names"], skin=skin, options=options)
    want = "fused_f32" if options.get("fused_arith") == "f32" else "fused_f16x2"
    assert a["info"]["path"] == want and b["info"]["path"] == want
    if skin > 1.0:
        rs = _rank_system(full, skin=skin)
        assert int(rs.numneigh.max()) > 128 and a["info"]["max_degree"] <= 64
    atc.assert_same_run(a, b, f"{kernel} {options} skin {skin}")
    util.assert_close_to(a, full["ref"], 5e-4, what=f"{kernel} {options}")


def test_centre_records_of_the_multi_workgroup_packing(hip_lib, model_dir):
    """More than 32 768 centres with tile_pack=separate: the centre records come from k_centre_info instead of the single-workgroup packing kernel.  A jittered
    simple-cubic lattice (6 neighbours per atom) of one element of the 20; no oracle at this size, the slice is the yardstick."""
    n, a0 = 33, 4.0
    pos = np.array([[i, j, k] for i in range(n) for j in range(n) for k in range(n)], dtype=float) * a0
    pos = pos + np.random.RandomState(7).uniform(-0.1, 0.1, size=pos.shape) + 0.5
    cell, types = np.eye(3) * n * a0, np.ones(len(pos), dtype=np.int32)
    assert len(pos) > 32768
    cfg = model_file.model_S(type_names=list(atc.NAMES20), avg_num_neighbors=6.0, r_max=5.0, num_layers=2)
    w = model_file.init_weights(cfg)
    cfg1, w1 = model_file.subset_types(cfg, w, ["Cu"])
    runs = []
    for tag, (c, ww) in (("full", (cfg, w)), ("twin", (cfg1, w1))):
        path = f"{model_dir}/at_sc33_{tag}.ahip"
        model_file.save_ahip(path, c, ww)
        runs.append(util.run_pair(hip_lib, path, cell, pos, types, ["Cu"], options={"tile_pack": "separate"}))
    assert runs[0]["info"]["path"] == "fused_f16x2" == runs[1]["info"]["path"]
    atc.assert_same_run(runs[0], runs[1], "35 937 centres, tile_pack=separate")


# ---- 6: per-pair cutoffs ----
@pytest.mark.parametrize("kernel", ["k_fused", "k_fused_lx"])
def test_per_pair_cutoffs_of_the_active_pairs(hip_lib, model_dir, kernel):
    T = len(atc.NAMES20)
    pcut = np.full((T, T), 5.0)
    for k, (a, b) in enumerate((a, b) for a in atc.ACTIVE3 for b in atc.ACTIVE3):
        pcut[a, b] = 4.95 - 0.06 * k          # nine different values, 4.47 .. 4.95
    # (rows and columns of the other types keep 5.0: a slot that read them would be seen)
    full, twin = _pair20(model_dir, kernel, per_edge_type_cutoff=pcut.tolist(), key_extra="pcut")
    assert np.asarray(twin["cfg"]["per_edge_type_cutoff"]).shape == (3, 3) and len(set(np.asarray(twin["cfg"]["per_edge_type_cutoff"]).reshape(-1))) == 9
    a = fsc.run(hip_lib, full)
    b = fsc.run(hip_lib, twin)
    assert a["info"]["path"] == "fused_f16x2" and b["info"]["path"] == "fused_f16x2"
    util.assert_close_to(a, full["ref"], 5e-4, what=f"per-pair cutoffs {kernel}")
    assert np.abs(a["forces"] - full["ref"]["forces"]).max() < pc.NORTH_STAR_DF
    atc.assert_same_run(a, b, f"per-pair cutoffs {kernel}")


# ---- 7: the set changes under one model object ----
def test_set_change_on_one_model(hip_lib, model_dir):
    full, _twin = _pair20(model_dir, "k_fused")
    cfg, w = full["cfg"], full["w"]
    other = ["Na", "Mg", "Al"]                 # the same atoms as other elements: model types 10, 11, 12
    ref2 = util.oracle_run(dict(cfg, model_dtype="float64"), w, full["cell"], full["pos"], full["types"], other)
    rs = _rank_system(full)
    m = capi.Model(full["path"], 0, hip_lib)
    r1 = _host_eval(m, cfg, rs, atc.PAIR_NAMES)
    r2 = _host_eval(m, cfg, rs, other)
    r3 = _host_eval(m, cfg, rs, atc.PAIR_NAMES)
    m.close()
    assert [r["info"]["path"] for r in (r1, r2, r3)] == ["fused_f16x2"] * 3
    assert r1["active"] == atc.ACTIVE3 == r3["active"] and r2["active"] == [10, 11, 12]
    assert (r1["eatom"] == r3["eatom"]).all() and abs(r1["pe"] - r3["pe"]) <= 1e-12 * abs(r1["pe"])
    assert np.abs(r1["forces"] - r3["forces"]).max() <= 1e-9 * np.abs(r1["forces"]).max()
    util.assert_close_to(r1, full["ref"], 5e-4, what="first set")
    util.assert_close_to(r2, ref2, 5e-4, what="second set")
    assert np.abs(r2["forces"] - ref2["forces"]).max() < pc.NORTH_STAR_DF
    assert np.abs(r2["forces"] - r1["forces"]).max() > 1e-3          # it IS another model


# ---- 8: the device-resident path ----
def test_device_path_and_inactive_type_report(hip_lib, model_dir):
    import torch
    full, _twin = _pair20(model_dir, "k_fused")
    fsc.measure(hip_lib, full)
    cfg, rs = full["cfg"], _rank_system(full)
    mapper, _cm = util.type_mapper_and_cutoffs(cfg, atc.PAIR_NAMES)
    dev = torch.device("cuda", 0)
    m = capi.Model(full["path"], 0, hip_lib)
    m.neigh_update_csr(rs.nall, rs.ilist, rs.offsets, rs.flat)
    x = torch.tensor(rs.x, device=dev)
    lt = torch.tensor(rs.type, dtype=torch.int32, device=dev)
    mt = torch.zeros(rs.nall, dtype=torch.int32, device=dev)
    m.map_types_dev(rs.nall, lt.data_ptr(), mapper, mt.data_ptr())
    assert (mt.cpu().numpy() == mapper[rs.type - 1]).all()           # full model types: 7, 18, 19
    f = torch.zeros_like(x)
    ea = torch.zeros(rs.nall, dtype=torch.float64, device=dev)
    ev = torch.zeros(7, dtype=torch.float64, device=dev)
    m.compute_dev(rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), ea.data_ptr(), ev.data_ptr())
    torch.cuda.synchronize()
    assert m.last_path == "fused_f16x2" and m.get_active_types() == atc.ACTIVE3
    forces = np.zeros((len(full["pos"]), 3))
    np.add.at(forces, rs.tag - 1, f.cpu().numpy())
    host = full["fused"]
    assert np.abs(forces - host["forces"]).max() <= 1e-9 * np.abs(host["forces"]).max()
    assert (ea.cpu().numpy()[: rs.nlocal] == host["eatom"][rs.tag[: rs.nlocal] - 1]).all()
    # an explicit set that leaves out a type in use: the evaluation completes (the atom takes slot 0, every index in range), the next accessor reports it.  Once.
    m.set_active_types([7, 18])
    f.zero_()
    m.compute_dev(rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), ea.data_ptr(), ev.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f).all())
    with pytest.raises(capi.AhipError) as e:
        m.get_active_types()
    assert e.value.code == capi.AHIP_ERR_ARG and "model type 19" in e.value.msg and "Ag" in e.value.msg, e.value.msg
    assert m.get_active_types() == [7, 18]                            # reported once
    m.close()


# ---- 9: registered outputs ----
@pytest.mark.parametrize("kernel", ["k_fused", "k_fused_lx2"])
def test_atomic_virial_and_atomic_energy_with_20_types(hip_lib, model_dir, kernel):
    full, _twin = _pair20(model_dir, kernel)
    cfg, w, names = full["cfg"], full["w"], atc.PAIR_NAMES
    rs = av.rank_system(cfg, full["cell"], full["pos"], full["types"])
    ref = av.oracle_w(cfg, w, rs, names)
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", full["path"]] + names, ntypes=len(names))
    pair.add_custom_output("atomic_virial")
    pair.add_custom_output("atomic_energy")
    pair.init_style()
    atom = atom_from_rank_system(rs, len(names))
    pair.compute(atom, list_from_rank_system(rs))
    assert pair.model.last_path == "fused_f16x2" and pair.model.get_active_types() == atc.ACTIVE3
    W = pair.custom_output("atomic_virial").reshape(-1, 9)
    ae = pair.custom_output("atomic_energy").reshape(-1)
    virial = pair.virial.copy()
    eatom = pair.eatom[: rs.nlocal].copy()
    pair.model.close()
    # the bars of tests/test_gpu_atomic_virial.py (f16x2: 2e-5 of max|W|; symmetric sum against the virial: 1e-6 of the row scale)
    assert W.shape == ref.shape
    assert np.abs(W - ref).max() <= 2e-5 * np.abs(ref).max()
    assert np.abs(av.sym_sum(W) - virial).max() <= 1e-6 * np.abs(W).max(axis=1).sum()
    # atomic_energy: the centres' energies, and for the ghost rows the shift of their FULL model type
    assert ae.shape == (rs.nall,) and rs.nghost > 0
    assert (ae[: rs.nlocal] == eatom).all()
    mapper, _cm = util.type_mapper_and_cutoffs(cfg, names)
    assert (ae[rs.nlocal:] == np.asarray(w["shift"])[mapper[rs.type[rs.nlocal:] - 1]]).all()
    np.testing.assert_allclose(eatom, full["ref"]["eatom"][rs.tag[: rs.nlocal] - 1], atol=5e-4, rtol=5e-4)


# ---- 10: the opt-in for a model of at most 16 types ----
def test_explicit_subset_of_a_3_type_model(hip_lib, model_dir):
    _full, twin = _pair20(model_dir, "k_fused")
    cfg = twin["cfg"]
    assert cfg["type_names"] == ["O", "Cu", "Ag"]
    names = ["Ag", "O"]                        # every Cu atom relabelled Ag: model types 0 and 2 in use
    _cell, _pos, symbols, *_ = fsc.geometry("Cu2AgO4")
    types = np.array([names.index("Ag" if s == "Cu" else s) + 1 for s in symbols], dtype=np.int32)
    rs = _rank_system(twin, types)
    m = capi.Model(twin["path"], 0, hip_lib)
    plain = _host_eval(m, cfg, rs, names)
    m.close()
    m = capi.Model(twin["path"], 0, hip_lib)
    m.set_active_types([2, 0])
    sub = _host_eval(m, cfg, rs, names)
    m.close()
    assert plain["active"] == [] and sub["active"] == [0, 2]
    assert plain["info"]["path"] == "fused_f16x2" == sub["info"]["path"]
    atc.assert_same_run(sub, plain, "3-type model, explicit set {0, 2}")


# ---- 11: NVE helpers with a 20-type mass table ----
def test_nve_with_20_types(hip_lib, model_dir):
    import torch
    full, _twin = _pair20(model_dir, "k_fused")
    m = capi.Model(full["path"], 0, hip_lib)
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(11)
    n, nall, dt, ftm2v = 1000, 1100, 0.002, 1.0 / 1.0364269e-4
    mass = 1.0 + 3.7 * np.arange(20, dtype=np.float64)
    mt = (np.arange(nall) * 7 % 20).astype(np.int32)
    x0, v0, f0 = rng.normal(size=(nall, 3)), rng.normal(size=(nall, 3)), rng.normal(size=(nall, 3))
    vv = v0[:n] + ((0.5 * dt * ftm2v) * (1.0 / mass[mt[:n]]))[:, None] * f0[:n]
    for mode in (0, 1, "first"):
        x, v, f = (torch.tensor(a, device=dev) for a in (x0, v0, f0))
        mtd = torch.tensor(mt, device=dev)
        if mode == "first":
            m.nve_first_dev(n, nall, x.data_ptr(), v.data_ptr(), f.data_ptr(), mtd.data_ptr(), mass, dt, ftm2v)
        else:
            m.nve_dev(mode, n, x.data_ptr(), v.data_ptr(), f.data_ptr(), mtd.data_ptr(), mass, dt, ftm2v)
        torch.cuda.synchronize()
        xh, vh, fh = x.cpu().numpy(), v.cpu().numpy(), f.cpu().numpy()
        np.testing.assert_allclose(vh[:n], vv, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(xh[:n], x0[:n] if mode == 1 else x0[:n] + dt * vv, rtol=1e-13, atol=1e-13)
        assert (vh[n:] == v0[n:]).all() and (xh[n:] == x0[n:]).all()
        assert (fh == 0).all() if mode == "first" else (fh == f0).all()
    m.close()
