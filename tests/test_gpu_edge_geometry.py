"""Adversarial geometry on every kernel path (k_fused, k_fused_lx, k_fused_lx2, the layer-at-a-time float32 kernels), on the float32 instance
and with the default arithmetic, against the float64 oracle: perfect lattices (ties in edge order, net forces zero in exact arithmetic),
a symmetric cluster without ghosts, a neighbour shell exactly at the cutoff and one float64 ulp either side of it, bonds along the axes and
collinear chains (spherical-harmonic components exactly 0), bonds of 0.1 r_max and r_max (1 - 1e-6).  Where net forces vanish the bar is
relative to the oracle's largest per-edge gradient."""
import numpy as np
import pytest

import parity_cases as pc
import path_parity as pp
import util
from pair_allegro_amd import lmp_like, model_file

pytestmark = pytest.mark.gpu

R_MAX = 5.0
BOX = 40.0                       # clusters: no periodic image within r_max + skin, i.e. no ghosts


def _fcc(n, a):
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    return np.eye(3) * (n * a), ((g[:, None, :] + basis[None]).reshape(-1, 3) * a)


def _geometries():
    out = {}
    cell, pos, _ = lmp_like.diamond_si(2, jitter=0.0)
    out["diamond_si_perfect"] = (cell, pos, ["Si"] * len(pos))
    cell, pos = _fcc(3, 3.61)
    out["fcc_cu_perfect"] = (cell, pos, ["Cu"] * len(pos))
    c = np.full(3, BOX / 2)
    nn = np.array([v for v in np.ndindex(3, 3, 3) if sorted(np.abs(np.array(v) - 1).tolist()) == [0, 1, 1]]) - 1      # 12 fcc nearest neighbours
    out["cuboctahedron_no_ghosts"] = (np.eye(3) * BOX, np.concatenate([c[None], c + 1.8 * nn]), ["Cu"] * 13)
    cell, pos = np.eye(3) * 10.4, np.array(list(np.ndindex(4, 4, 4)), dtype=np.float64) * 2.6
    out["simple_cubic_axis_bonds"] = (cell, pos, ["Cu"] * len(pos))
    chain = [c + [2.3 * k, 0, 0] for k in range(-2, 3)] + [c + [0, 6.0, 2.4 * k] for k in range(-2, 3)] + \
            [c + [-7.0, -3.0, 0] + 1.7 * k * np.ones(3) / np.sqrt(3) for k in range(4)]
    sym = ["Cu"] * 5 + ["O"] * 5 + ["Cu", "O", "Cu", "O"]
    out["collinear_chains"] = (np.eye(3) * BOX, np.array(chain), sym)
    ext = [c, c + [0.1 * R_MAX, 0, 0], c + [0, R_MAX * (1 - 1e-6), 0], c + [0.1 * R_MAX, 0, -R_MAX * (1 - 1e-6)],
           c + [-2.0, -2.5, 0.3]]
    out["bond_length_extremes"] = (np.eye(3) * BOX, np.array(ext), ["Cu", "O", "Cu", "O", "O"])
    # centre on exact binary coordinates; neighbours at the signed permutations of (3, 4, 0) (|d|^2 = r_max^2 = 25 exactly in float64): three
    # of them exactly there, five with the coordinate of 4 one ulp farther out (just outside), five one ulp farther in (just inside)
    c0 = np.array([16.0, 16.0, 16.0])
    dirs = [np.array(v, dtype=np.float64) for v in sorted({(s1 * a, s2 * b, 0.0) for a, b in ((3, 4), (4, 3)) for s1 in (1, -1) for s2 in (1, -1)})]
    dirs += [np.roll(v, 1) for v in dirs] + [np.roll(v, 2) for v in dirs]
    shell = [c0]
    for n, d in enumerate(dirs[:13]):
        p = c0 + d
        if n >= 3:
            ax = int(np.argmax(np.abs(d)))
            p[ax] = np.nextafter(p[ax], c0[ax] + 2.0 * d[ax] if n < 8 else c0[ax])
        shell.append(p)
    out["shell_at_the_cutoff"] = (np.eye(3) * 32.0, np.array(shell), ["Cu"] * len(shell))
    return out


GEOMETRIES = _geometries()
MODELS = {
    "k_fused": dict(),
    "k_fused_lx": dict(l_max=2, num_tensor_features=32),
    "k_fused_lx2": dict(l_max=2, num_tensor_features=64),
    "layer_kernels": dict(),
}
_models = {}


def _model(model_dir, kind, names):
    key = (kind, tuple(names))
    if key not in _models:
        over = dict(MODELS[kind], type_names=list(names), avg_num_neighbors=20.0)
        cfg = model_file.model_L(**over) if over.get("l_max") == 2 else model_file.model_S(**over)
        w = model_file.init_weights(cfg)
        path = f"{model_dir}/geom_{kind}_{'_'.join(names)}.ahip"
        model_file.save_ahip(path, cfg, w)
        _models[key] = (cfg, w, path)
    return _models[key]


@pytest.mark.parametrize("kind,arith", [(k, a) for k in MODELS for a in ("f32", "auto") if not (k == "layer_kernels" and a == "auto")])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_adversarial_geometry(hip_lib, model_dir, geom, kind, arith):
    """arith auto on a fused kernel must stay on f16x2: the first-evaluation self-check compares with the float32 instance relative to max|F|,
    which is rounding noise on a perfect lattice."""
    cell, pos, symbols = GEOMETRIES[geom]
    names = sorted(set(symbols))
    types = np.array([names.index(s) + 1 for s in symbols], dtype=np.int32)
    cfg, w, path = _model(model_dir, kind, names)
    if kind == "layer_kernels":
        opts = {"path": "generic"}
    else:
        opts = {"path": "fused"} if arith == "auto" else {"path": "fused", "fused_arith": "f32"}
    ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, names)
    res = util.run_pair(hip_lib, path, cell, pos, types, names, options=opts)
    expect = "generic_f32" if kind == "layer_kernels" else (pc.FUSED_DEFAULT if arith == "auto" else "fused_f32")
    assert res["info"]["path"] == expect, res["info"]
    # the edge list is bit-identical to the host glue's rsq <= cut^2 (same pairs, same float32 vectors)
    rs = ref["rs"]
    ref_ei = ref["inputs"]["edge_index"]
    mine = sorted(zip(res["edges"][0].tolist(), res["edges"][1].tolist(), np.round(res["edges"][2], 6).tolist()))
    d_ref = np.linalg.norm(rs.x[ref_ei[1]] - rs.x[ref_ei[0]], axis=1)
    theirs = sorted(zip((rs.tag[ref_ei[0]] - 1).tolist(), (rs.tag[ref_ei[1]] - 1).tolist(), np.round(d_ref, 6).tolist()))
    assert [(a, b) for a, b, _ in mine] == [(a, b) for a, b, _ in theirs]
    np.testing.assert_allclose([d for *_, d in mine], [d for *_, d in theirs], rtol=0, atol=2e-6)
    _, gref = pp.oracle_edge_gradients(cfg, w, rs, names)
    gmax = np.abs(gref).max()
    df = np.abs(res["forces"] - ref["forces"]).max()
    de = np.abs(res["eatom"] - ref["eatom"]).max()
    e_model = ref["eatom"] - np.asarray(w["shift"])[types - 1]                 # what the model adds to the per-type shift
    allowed_e = pp.BAR["float32"] * np.abs(e_model).max() + pp.ROUNDING["float32"] * np.abs(ref["eatom"]).max()
    print(f"\n{geom} {kind} {arith} ({res['info']['path']}): max|dF| / (1e-4 max|g_ref|) {df / (1e-4 * gmax):.3f}, "
          f"max|dE_i| / bar {de / allowed_e:.3f} ({len(ref_ei[0])} edges)")
    assert df <= pp.BAR["float32"] * gmax, (df, gmax)
    assert de <= allowed_e, (de, allowed_e)
