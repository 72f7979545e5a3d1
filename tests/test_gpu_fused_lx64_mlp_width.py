"""GPU tests of the MLP-width-128 instances of k_fused_lx2 (template parameter WH = 4: csrc/fused_lx2.hip, object fused_lx2_m.o) behind option lx64_mlp_width=auto: a model
of 33..64 tensor features (l_max = 2, or l_max = 1 lifted) with 65 <= mlp_width <= 128 runs fused, zero-padded to hidden width 128, on the f16x2 arithmetic with read-out
depth 1.  Without the option -- the default, "64" -- such a model runs on the layer-at-a-time float32 kernels (`generic_f32`), as tests/test_gpu_fused_mlp_width.py pins.

Every model here is evaluated with {"lx64_mlp_width": "auto"}.  Geometries are those of tests/fused_shape_cases.py; the float64 oracle runs once per model and is shared.
`twin` is the mlp_width = 64 model of the same kernel, depths and geometry.  The bars are those of fused_shape_cases.assert_bars, restated here because that helper asserts on
the default-options run: path fused_f16x2; energies and virial util.assert_close_to(.., 5e-4); max|dF| against the float64 oracle below parity_cases.NORTH_STAR_DF and below
max(3 e_generic, 1e-5), e_generic being the error of path=generic on the same file -- or twice the twin's measured error where the twin itself misses that bar.
Every figure is printed before it is asserted.
Measured on the MI355X (max|dF|, eV/A): the nine plain width-128 instances on Cu2AgO4 5.3e-7 .. 1.8e-6, their width-64 twins 3.7e-7 .. 1.2e-6 (always inside max(3 e_generic, 1e-5),
so the fall-back bar is not in use), the layer-at-a-time float32 kernels 1.2e-6 .. 4.2e-6; widths 65 / 72 / 96 / 100 5.6e-7 .. 1.0e-6; lifted l_max = 1 models 3.4e-7 / 9.1e-7;
256-atom box 1.8e-6, 6-neighbour lattice 5.4e-7; atomic_virial max|dW| 4.1e-7 at max|W| 1.19; fused_arith=auto keeps f16x2 at 1.97e-6 max|F| from the float32 pass."""
import numpy as np
import pytest
import torch

import atomic_virial_ref as av
import fused_shape_cases as fsc
import parity_cases as pc
import util
from pair_allegro_amd import capi, model_file
from pair_allegro_amd.pair import atom_from_rank_system, list_from_rank_system

pytestmark = pytest.mark.gpu

OPT = {"lx64_mlp_width": "auto"}
K = "k_fused_lx2"


def _pair(model_dir, tag, kernel=K, width=128, **over):
    """The model of MLP width `width` and its mlp_width = 64 twin (same kernel, other widths, depths, layers, geometry)."""
    over.setdefault("readout_depth", 1)
    return fsc.model(model_dir, tag, kernel, **dict(over, mlp_width=width)), fsc.model(model_dir, tag, kernel, **over)


def _measure(hip_lib, c):
    """With the option, and path=generic with it, on the same file, both against the float64 oracle; once per model (keys of their own: fsc.measure's are the default run's)."""
    if "lx64" not in c:
        c["lx64"] = fsc.run(hip_lib, c, OPT)
        c["lx64_generic"] = fsc.run(hip_lib, c, dict(OPT, path="generic"))
        c["lx64_err"] = float(np.abs(c["lx64"]["forces"] - c["ref"]["forces"]).max())
        c["lx64_egen"] = float(np.abs(c["lx64_generic"]["forces"] - c["ref"]["forces"]).max())
    return c


def _assert_bars(hip_lib, c, twin, what):
    _measure(hip_lib, c)
    _measure(hip_lib, twin)
    print(f"{what}: max|dF| vs f64 oracle fused {c['lx64_err']:.3e}, layer-at-a-time f32 {c['lx64_egen']:.3e}; twin: fused {twin['lx64_err']:.3e}, "
          f"layer-at-a-time f32 {twin['lx64_egen']:.3e}; paths {c['lx64']['info']['path']} / {twin['lx64']['info']['path']}")
    assert c["lx64"]["info"]["path"] == "fused_f16x2", c["lx64"]["info"]
    assert c["lx64_generic"]["info"]["path"] == "generic_f32" and twin["lx64"]["info"]["path"] == "fused_f16x2", twin["lx64"]["info"]
    util.assert_close_to(c["lx64"], c["ref"], 5e-4, what=what)
    assert c["lx64_err"] < pc.NORTH_STAR_DF
    bar = max(3.0 * c["lx64_egen"], 1e-5)
    if twin["lx64_err"] >= max(3.0 * twin["lx64_egen"], 1e-5):
        bar = 2.0 * twin["lx64_err"]
    assert c["lx64_err"] < bar, (what, c["lx64_err"], bar)
    return c


@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("md", [1, 2, 3])
def test_every_instance_ragged_tiles(hip_lib, model_dir, md, nl):
    """1: every compiled WH = 4 instance (1..3 layers x latent MLP depth 1..3; the per-atom-virial twins: case 7) on Cu2AgO4, 7 atoms, degrees 36..39."""
    c, twin = _pair(model_dir, "Cu2AgO4", num_layers=nl, mlp_depth=md)
    _assert_bars(hip_lib, c, twin, f"Cu2AgO4 k_fused_lx2 {nl} layers MLP depth {md} MLP width 128")


@pytest.mark.parametrize("width", [65, 72, 96])
def test_padding_inside_the_width(hip_lib, model_dir, width):
    """2: 65 (one feature in the fifth hidden tile), 72 (a half-filled tile), 96 (the second hand-over round all padding for one wave half)."""
    c, twin = _pair(model_dir, "Cu2AgO4", width=width, num_layers=2)
    _assert_bars(hip_lib, c, twin, f"Cu2AgO4 k_fused_lx2 MLP width {width}")


def test_all_paddings_at_once(hip_lib, model_dir):
    """3: S 48, U 48, read-out width 24 with MLP width 100."""
    over = dict(fsc.NARROW, num_tensor_features=48, mlp_width=64)
    c, twin = _pair(model_dir, "Cu2AgO4", width=100, **over)
    assert c["cfg"]["mlp_width"] == 100 and twin["cfg"]["mlp_width"] == 64 and c["cfg"]["num_scalar_features"] == 48 and c["cfg"]["num_tensor_features"] == 48
    _assert_bars(hip_lib, c, twin, "Cu2AgO4 k_fused_lx2 narrow model, MLP width 100")


@pytest.mark.parametrize("U", [48, 64])
def test_lifted_l1_model(hip_lib, model_dir, U):
    """4: l_max = 1 with 48 / 64 tensor features, lifted to l_max = 2."""
    c, twin = _pair(model_dir, "Cu2AgO4", "l1", num_tensor_features=U, num_layers=2)
    assert c["cfg"]["l_max"] == 1
    _assert_bars(hip_lib, c, twin, f"Cu2AgO4 l_max 1, {U} tensor features, MLP width 128")


@pytest.mark.parametrize("tag,over", [("CuPd256", dict(num_layers=3)), ("sc27", {})], ids=["CuPd256", "sc27"])
def test_full_tiles(hip_lib, model_dir, tag, over):
    """5: three layers on the 256-atom box (degree 42: every wave pair carries edges), and the 6-neighbour lattice (four centres per tile: the per-centre reduction with MAXA
    centres)."""
    c, twin = _pair(model_dir, tag, **over)
    _assert_bars(hip_lib, c, twin, f"{tag} k_fused_lx2 MLP width 128")
    print(f"{tag}: max degree {c['lx64']['info']['max_degree']}")
    if tag == "CuPd256":
        assert c["lx64"]["info"]["max_degree"] > 32
    else:
        assert c["lx64"]["info"]["max_degree"] <= 16


def test_more_tiles_than_workgroups(hip_lib, model_dir):
    """6: reserve_wgs=128 leaves CUs - 64 workgroups for the 256 tiles of the 256-atom box: a workgroup consumes the longer weight stream more than once.  Against
    reserve_wgs=0: per-atom energies bit for bit, forces within 1e-9 of max|F| (float64 atomics in arrival order)."""
    c = fsc.model(model_dir, "CuPd256", K, mlp_width=128, readout_depth=1, num_layers=3)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    grid = ncu - 64
    pair, rs, f1, e1, pe1 = fsc.one_evaluation(hip_lib, c, dict(OPT, reserve_wgs="128"))
    try:
        assert pair.model.last_path == "fused_f16x2"
        used, total = pair.model.tile_occupancy()
        tiles = total // 64
        print(f"k_fused_lx2 MLP width 128 on CuPd256: {tiles} tiles ({used} edges) on {grid} workgroups of {ncu} CUs")
        assert total % 64 == 0 and tiles > grid > 0, (tiles, grid)
    finally:
        pair.model.close()
    pair, _, f0, e0, pe0 = fsc.one_evaluation(hip_lib, c, dict(OPT, reserve_wgs="0"), rs=rs)
    try:
        assert pair.model.last_path == "fused_f16x2"
    finally:
        pair.model.close()
    print(f"per-atom energies that differ {int((e1 != e0).sum())}, max|dF| {np.abs(f1 - f0).max():.3e} (max|F| {np.abs(f0).max():.3e})")
    assert int((e1 != e0).sum()) == 0
    assert np.abs(f1 - f0).max() <= 1e-9 * np.abs(f0).max()
    assert abs(pe1 - pe0) <= 1e-12 * abs(pe0)
    forces = np.zeros((len(c["pos"]), 3))
    np.add.at(forces, rs.tag - 1, f1)
    assert np.abs(forces - c["ref"]["forces"]).max() < pc.NORTH_STAR_DF


AV_NAMES = ["Ag", "Cu", "O"]


def test_atomic_virial_twin(hip_lib, model_dir):
    """7: the VAR_VA twins: output atomic_virial against the float64 oracle's W, bars of test_gpu_atomic_virial.py (2e-5 of max|W|; the symmetrised sum of W against the
    virial at 1e-6 of the row scale)."""
    g = util.load_golden("Cu2AgO4_r5")
    base, over = fsc.KERNELS[K]
    cfg = base(**dict(over, type_names=AV_NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), mlp_width=128))
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/lx64_w128_av.ahip"
    model_file.save_ahip(path, cfg, w)
    types = np.array([AV_NAMES.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    rs = av.rank_system(cfg, g["cell"], g["pos"], types)
    ref = av.oracle_w(cfg, w, rs, AV_NAMES)
    res = av.run(hip_lib, path, rs, AV_NAMES, options=dict(OPT, path="fused", fused_arith="f16x2"))
    assert res["path"] == "fused_f16x2"
    assert res["W"].shape == ref.shape
    scale = np.abs(ref).max()
    err = np.abs(res["W"] - ref).max()
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    dv = np.abs(av.sym_sum(res["W"]) - res["virial"]).max()
    print(f"atomic_virial k_fused_lx2 MLP width 128: max|dW| {err:.3e} (max|W| {scale:.3e}), |sym_sum(W) - virial| {dv:.3e} (row scale {rowscale:.3e})")
    assert err <= 2e-5 * scale, (err, scale)
    assert dv <= 1e-6 * rowscale, (dv, rowscale)


def test_arithmetic(hip_lib, model_dir, monkeypatch):
    """8: f16x2 only.  fused_arith=f32 sends the model to the layer-at-a-time kernels and path=fused then names the rule; fused_arith=auto with its first-evaluation
    self-check on (whose float32 pass runs on the layer-at-a-time kernels) ends on f16x2 and says so."""
    monkeypatch.delenv("AHIP_NO_ARITH_SELFCHECK", raising=False)
    c = fsc.model(model_dir, "Cu2AgO4", K, mlp_width=128, readout_depth=1, num_layers=3)
    exact = fsc.run(hip_lib, c, dict(OPT, fused_arith="f32"))
    assert exact["info"]["path"] == "generic_f32"
    util.assert_close_to(exact, c["ref"], 5e-4, what="MLP width 128, fused_arith=f32")
    with pytest.raises(Exception, match="fused path unavailable.*MLP width 65..128 runs on the f16x2 arithmetic only on the wide fused kernels"):
        fsc.run(hip_lib, c, dict(OPT, path="fused", fused_arith="f32"))
    auto = fsc.run(hip_lib, c, dict(OPT, fused_arith="auto"))
    print(f"fused_arith=auto: {auto['info']['path']}; {auto['info']['arith_note']}")
    assert auto["info"]["path"] == "fused_f16x2"
    assert "f16x2 kept" in auto["info"]["arith_note"], auto["info"]["arith_note"]
    util.assert_close_to(auto, c["ref"], 5e-4, what="MLP width 128, fused_arith=auto")


def _evaluate(pair, rs, c):
    atom = atom_from_rank_system(rs, len(c["names"]))
    pair.compute(atom, list_from_rank_system(rs))
    n = len(c["pos"])
    forces = np.zeros((n, 3))
    np.add.at(forces, rs.tag - 1, atom.f)
    eatom = np.zeros(n)
    eatom[rs.tag[: rs.nlocal] - 1] = pair.eatom[: rs.nlocal]
    return dict(forces=forces, eatom=eatom, pe=float(pair.eng_vdwl), virial=np.array(pair.virial, dtype=float), path=pair.model.last_path)


def test_option_on_one_model_object(hip_lib, model_dir):
    """9a: "64" -> "auto" -> "64" on one model object: layer-at-a-time, fused, layer-at-a-time again (the prepared state is dropped with the option), each within 5e-4."""
    c = fsc.model(model_dir, "Cu2AgO4", K, mlp_width=128, readout_depth=1, num_layers=2)
    pair, rs, _, _, _ = fsc.one_evaluation(hip_lib, c, {"lx64_mlp_width": "64"})
    try:
        assert pair.model.last_path == "generic_f32"
        runs = []
        for v in ("64", "auto", "64"):
            pair.model.set_option("lx64_mlp_width", v)
            runs.append(_evaluate(pair, rs, c))
            print(f"lx64_mlp_width={v}: {runs[-1]['path']}, max|dF| vs f64 oracle {np.abs(runs[-1]['forces'] - c['ref']['forces']).max():.3e}")
        assert [r["path"] for r in runs] == ["generic_f32", "fused_f16x2", "generic_f32"]
        for r in runs:
            util.assert_close_to(r, c["ref"], 5e-4, what="64 -> auto -> 64")
    finally:
        pair.model.close()


def test_option_values(hip_lib, model_dir):
    """9b: anything but 64 | auto is an error that names the accepted values."""
    c = fsc.model(model_dir, "Cu2AgO4", K, mlp_width=128, readout_depth=1, num_layers=2)
    m = capi.Model(c["path"], 0, hip_lib)
    try:
        with pytest.raises(Exception, match=r"64\|auto"):
            m.set_option("lx64_mlp_width", "128")
        m.set_option("lx64_mlp_width", "auto")
        m.set_option("lx64_mlp_width", "64")
    finally:
        m.close()


@pytest.mark.parametrize("kernel,width", [("k_fused_lx", 128), ("k_fused_lx2", 64)])
def test_option_changes_nothing_elsewhere(hip_lib, model_dir, kernel, width):
    """9c: a k_fused_lx model of width 128 and a k_fused_lx2 model of width 64: per-atom energies bit for bit with and without the option."""
    c = fsc.model(model_dir, "Cu2AgO4", kernel, mlp_width=width, readout_depth=1, num_layers=2)
    on, off = fsc.run(hip_lib, c, OPT), fsc.run(hip_lib, c)
    print(f"{kernel} MLP width {width}: {on['info']['path']} / {off['info']['path']}, per-atom energies that differ {int((on['eatom'] != off['eatom']).sum())}")
    assert on["info"]["path"] == off["info"]["path"] == "fused_f16x2"
    assert np.array_equal(on["eatom"], off["eatom"])
    assert np.abs(on["forces"] - off["forces"]).max() <= 1e-9 * np.abs(off["forces"]).max()


@pytest.mark.parametrize("what,over,reason", [
    ("read-out depth 2", dict(mlp_width=128, readout_depth=2), "MLP width 65..128 runs with read-out depth 1 only"),
    ("read-out width 64", dict(mlp_width=128, readout_depth=1, readout_width=64), "read-out width 33..64 has no fused instance with MLP width 65..128"),
    ("MLP width 129", dict(mlp_width=129, readout_depth=1), "MLP width 128"),
])
def test_limits_beside_it_stay_refused_with_the_option(hip_lib, model_dir, what, over, reason):
    """10: layer-at-a-time float32 kernels, within 5e-4 of the oracle; path=fused fails naming the limit."""
    d = fsc.model(model_dir, "Cu2AgO4", K, num_layers=2, **over)
    res = fsc.run(hip_lib, d, OPT)
    print(f"k_fused_lx2 {what}, with the option: {res['info']['path']}, max|dF| vs f64 oracle {np.abs(res['forces'] - d['ref']['forces']).max():.3e}")
    assert res["info"]["path"] == "generic_f32"
    util.assert_close_to(res, d["ref"], 5e-4, what=what)
    with pytest.raises(Exception, match="fused path unavailable.*" + reason):
        fsc.run(hip_lib, d, dict(OPT, path="fused"))


def test_dense_list(hip_lib, model_dir):
    """11: fcc Cu at r_max 6.1 (78 neighbours, above the 64-slot tile): with the option the model runs as it does without it, on the layer-at-a-time kernels; no error."""
    c = fsc.model(model_dir, "Cu108", K, mlp_width=128, readout_depth=1)
    on, off = fsc.run(hip_lib, c, OPT), fsc.run(hip_lib, c)
    print(f"Cu108 k_fused_lx2 MLP width 128: with the option {on['info']['path']}, without {off['info']['path']}, max degree {on['info']['max_degree']}")
    assert 64 < on["info"]["max_degree"] <= 128
    assert on["info"]["path"] == off["info"]["path"] == "generic_f32"
    util.assert_close_to(on, c["ref"], 5e-4, what="MLP width 128, dense list, with the option")
    util.assert_close_to(off, c["ref"], 5e-4, what="MLP width 128, dense list, without the option")
