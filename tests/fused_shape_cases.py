"""Shared pieces of the GPU tests of the fused kernels' newer shapes (tests/test_gpu_fused_readout_depth.py, tests/test_gpu_lmax1_wide_channels.py): the geometries, one
model file + float64 oracle per (geometry, model), the measurement against the layer-at-a-time kernels and the error bars of tests/test_gpu_fused_lx_depth.py."""
import numpy as np

import parity_cases as pc
import util
from oracle import allegro_torch
from pair_allegro_amd import lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

# the three fused kernels by the model that selects them: base config and overrides
KERNELS = {
    "k_fused": (model_file.model_S, {}),
    "k_fused_lx": (model_file.model_L, {"num_tensor_features": 32}),
    "k_fused_lx2": (model_file.model_L, {"num_tensor_features": 64}),
    "l1": (model_file.model_S, {}),          # l_max = 1 at the caller's num_tensor_features: k_fused up to 32, k_fused_lx2 (lifted to l_max = 2) from 33 to 64
}
NARROW = dict(num_scalar_features=48, num_tensor_features=16, mlp_width=40, readout_width=24)

_geoms = {}
_runs = {}          # (geometry, kernel, frozen overrides) -> the file, the float64 oracle, the default (fused) run and the layer-at-a-time run


def geometry(tag):
    """cell, positions, symbols, model type names, r_max, average neighbour count."""
    if tag in _geoms:
        return _geoms[tag]
    if tag == "Cu2AgO4":                  # 7 atoms, 3 types, triclinic, degrees 36..39
        g = util.load_golden("Cu2AgO4_r5")
        out = (g["cell"], g["pos"], g["symbols"], ["Cu", "Ag", "O"], 5.0, float(g["nedges"]) / len(g["pos"]))
    elif tag in ("CuPd256", "CuPd512"):   # the 256-atom CuPd box relabelled O / H (degree 42), and the same doubled along x
        g = util.load_golden("CuPd-cubic-big_r5")
        cell, pos = np.array(g["cell"], dtype=float), np.array(g["pos"], dtype=float)
        symbols = ["O" if s == "Cu" else "H" for s in g["symbols"]]
        nb = float(len(util.glue.brute_force_edges(cell, pos, 5.0)[0])) / len(pos)
        if tag == "CuPd512":
            a = cell[0] if cell.ndim == 2 else np.array([cell[0], 0.0, 0.0])
            pos = np.concatenate([pos, pos + a])
            symbols = symbols + symbols
            cell = cell.copy()
            cell[0] = 2.0 * cell[0]      # first lattice vector (or first box length)
        out = (cell, pos, symbols, ["O", "H"], 5.0, nb)
    elif tag == "sc27":                   # jittered simple-cubic lattice, a = 4: 6 neighbours per atom, so a 64-slot tile holds as many centres as the kernel allows
        n, a0 = 3, 4.0
        pos = np.array([[i, j, k] for i in range(n) for j in range(n) for k in range(n)], dtype=float) * a0
        pos = pos + np.random.RandomState(7).uniform(-0.1, 0.1, size=pos.shape) + 0.5
        out = (np.eye(3) * n * a0, pos, ["Cu"] * len(pos), ["Cu"], 5.0, 6.0)
    elif tag == "Cu108":                  # jittered fcc Cu, r_max 6.1: 78 neighbours per atom
        g = util.load_golden("Cu-cubic_r15")
        reps = 3
        cell = g["cell"] * reps
        shifts = np.array([[i, j, k] for i in range(reps) for j in range(reps) for k in range(reps)], dtype=float)
        pos = np.concatenate([g["pos"] + s @ g["cell"] for s in shifts])
        pos = pos + np.random.RandomState(3).uniform(-0.05, 0.05, size=pos.shape)
        nb = float(len(util.glue.brute_force_edges(cell, pos, 6.1)[0])) / len(pos)
        out = (cell, pos, ["Cu"] * len(pos), ["Cu"], 6.1, nb)
    else:
        raise KeyError(tag)
    _geoms[tag] = out
    return out


def model(model_dir, tag, kernel, edit=None, edit_name="", **over):
    """The model file of KERNELS[kernel] with `over` on geometry `tag` and its float64 oracle result, built once.  `edit(w)` may change the initial weights in place."""
    key = (tag, kernel, edit_name, tuple(sorted(over.items())))
    if key not in _runs:
        cell, pos, symbols, tn, r_max, nb = geometry(tag)
        base, kover = KERNELS[kernel]
        cfg = base(**dict(dict(kover, type_names=tn, avg_num_neighbors=nb, r_max=r_max), **over))
        w = model_file.init_weights(cfg)
        if edit is not None:
            edit(w)
        name = "fsc_" + tag + "_" + kernel + edit_name + "_" + "_".join(f"{k}{v}" for k, v in sorted(over.items()))
        path = f"{model_dir}/{name}.nequip.pth"
        allegro_torch.export_nequip_pth(path, cfg, w)
        names = sorted(set(symbols))
        types = np.array([names.index(s) + 1 for s in symbols], dtype=np.int32)
        ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, cell, pos, types, names)
        _runs[key] = dict(cfg=cfg, w=w, path=path, types=types, names=names, ref=ref, cell=cell, pos=pos)
    return _runs[key]


def run(hip_lib, c, options=None):
    return util.run_pair(hip_lib, c["path"], c["cell"], c["pos"], c["types"], c["names"], options=options)


def measure(hip_lib, c):
    """Default options (the fused kernel where the model has one) and path=generic on the same file, both against the float64 oracle; once per model."""
    if "fused" not in c:
        c["fused"] = run(hip_lib, c)
        c["generic"] = run(hip_lib, c, {"path": "generic"})
        c["err"] = float(np.abs(c["fused"]["forces"] - c["ref"]["forces"]).max())
        c["egen"] = float(np.abs(c["generic"]["forces"] - c["ref"]["forces"]).max())
    return c


def assert_bars(hip_lib, c, twin, what):
    """The bars of tests/test_gpu_fused_lx_depth.py: _assert_bars for model `c`, with `twin` the existing instance of the same shape measured beside it:
    fused_f16x2 under default options; energies and virial within 5e-4 of the float64 oracle; max|dF| below NORTH_STAR_DF and below max(3 e_generic, 1e-5), e_generic being
    the error of the layer-at-a-time float32 kernels on the same file -- or, where the twin itself misses that second bar, below twice the twin's measured error."""
    measure(hip_lib, c)
    measure(hip_lib, twin)
    print(f"{what}: max|dF| vs f64 oracle fused {c['err']:.3e}, layer-at-a-time f32 {c['egen']:.3e}; twin: fused {twin['err']:.3e}, layer-at-a-time f32 {twin['egen']:.3e}")
    assert c["fused"]["info"]["path"] == "fused_f16x2", c["fused"]["info"]
    assert c["generic"]["info"]["path"] == "generic_f32" and twin["fused"]["info"]["path"] == "fused_f16x2", twin["fused"]["info"]
    util.assert_close_to(c["fused"], c["ref"], 5e-4, what=what)
    assert c["err"] < pc.NORTH_STAR_DF
    bar = max(3.0 * c["egen"], 1e-5)
    if twin["err"] >= max(3.0 * twin["egen"], 1e-5):
        bar = 2.0 * twin["err"]
    assert c["err"] < bar, (what, c["err"], bar)
    return c


def one_evaluation(hip_lib, c, options=None, rs=None):
    """One evaluation through a model object that stays open for the caller's questions: (pair, rank system, forces [nall][3], per-atom energies, energy)."""
    pair = PairAllegro(me=0, nprocs=1, lib=hip_lib, quiet=True)
    pair.settings([])
    pair.coeff(["*", "*", c["path"]] + list(c["names"]), ntypes=len(c["names"]))
    for k, v in (options or {}).items():
        pair.model.set_option(k, v)
    pair.init_style()
    if rs is None:
        rs = lmp_like.build_rank_system(c["cell"], c["pos"], c["types"], pair.init_one(1, 1) + 1.0)
    atom = atom_from_rank_system(rs, len(c["names"]))
    pair.compute(atom, list_from_rank_system(rs))
    return pair, rs, atom.f.copy(), pair.eatom[: rs.nlocal].copy(), float(pair.eng_vdwl)
