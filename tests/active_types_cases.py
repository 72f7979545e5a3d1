"""Models with more types than the fused kernels hold (tests/test_active_types.py, tests/test_gpu_active_types.py): a 20-type model whose simulation names three of
them, and its twin -- the 3-type slice written by model_file.subset_types as a file of its own.  Geometries and bars come from tests/fused_shape_cases.py."""
import numpy as np

import fused_shape_cases as fsc
import util
from oracle import allegro_torch
from pair_allegro_amd import model_file

# 20 model types; the elements of the Cu2AgO4 golden sit at 7 (O), 18 (Cu) and 19 (Ag)
NAMES20 = ["H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar", "Cu", "Ag"]
ACTIVE3 = [7, 18, 19]
PAIR_NAMES = ["Ag", "Cu", "O"]            # the pair_coeff line of the tests: LAMMPS types 1, 2, 3

_built = {}


def config20(tag, kernel, **over):
    """(cfg, w, cell, pos, symbols): the 20-type model of fsc.KERNELS[kernel] on geometry `tag`."""
    cell, pos, symbols, _tn, r_max, nb = fsc.geometry(tag)
    base, kover = fsc.KERNELS[kernel]
    cfg = base(**dict(dict(kover, type_names=list(NAMES20), avg_num_neighbors=nb, r_max=r_max), **over))
    return cfg, model_file.init_weights(cfg), cell, pos, symbols


def pair20(model_dir, kernel, tag="Cu2AgO4", names=PAIR_NAMES, symbols=None, with_ref=True, key_extra="", **over):
    """(full, twin): the 20-type model file and the file of its slice at `names`, each a dict like those of fsc.model (path, cell, pos, types, names, ref: the float64
    oracle of THAT file), so that fsc.measure / fsc.assert_bars take them.  symbols: per-atom element names when the geometry's own are not wanted."""
    key = (kernel, tag, tuple(names), key_extra, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _built:
        cfg, w, cell, pos, sym0 = config20(tag, kernel, **over)
        symbols = list(sym0) if symbols is None else list(symbols)
        types = np.array([list(names).index(s) + 1 for s in symbols], dtype=np.int32)
        cfg3, w3 = model_file.subset_types(cfg, w, names)
        out = []
        for which, (c, ww) in (("full", (cfg, w)), ("twin", (cfg3, w3))):
            name = f"at_{which}_{kernel}_{tag}_{len(_built)}"
            path = f"{model_dir}/{name}.nequip.pth"
            allegro_torch.export_nequip_pth(path, c, ww)
            ref = util.oracle_run(dict(c, model_dtype="float64"), ww, cell, pos, types, list(names)) if with_ref else None
            out.append(dict(cfg=c, w=ww, path=path, types=types, names=list(names), ref=ref, cell=cell, pos=pos))
        _built[key] = tuple(out)
    return _built[key]


def assert_same_run(a, b, what=""):
    """The criterion of tests/test_gpu_soak.py between two runs that hand the kernels the same bytes: per-atom energies bit for bit (their summation order is fixed),
    forces within 1e-9 of max|F| (float64 atomics in arrival order), energy within 1e-12 relative.  A difference means a wrong slot, not rounding."""
    fscale = float(np.abs(b["forces"]).max())
    df = float(np.abs(a["forces"] - b["forces"]).max())
    ne = int((a["eatom"] != b["eatom"]).sum())
    print(f"{what}: max|dF| / max|F| = {df / fscale:.3e}, per-atom energies that differ: {ne}, dE = {abs(a['pe'] - b['pe']):.3e}")
    assert ne == 0, f"{what}: {ne} per-atom energies differ"
    assert df <= 1e-9 * fscale, f"{what}: forces differ by {df / fscale:.3e} of max|F|"
    assert abs(a["pe"] - b["pe"]) <= 1e-12 * abs(b["pe"]), what
