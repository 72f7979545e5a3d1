"""Path-difference parity on the CPU (tests/path_parity.py): every tensor-product path of l_max 1, 2 and 3 models, isolated as
Delta = F(row p boosted) - F(row p zero), through the emulated layer-at-a-time kernels in float64 and float32 against the float64 oracle;
and the power of that bar: one wrong Clebsch-Gordan entry, one flipped sign, two swapped m components of the ORACLE's table move Delta
by at least 5x the bar, so the GPU version of the harness (tests/test_gpu_path_parity.py) sees a kernel with such a defect."""
import numpy as np
import pytest

import path_parity as pp
import util
from pair_allegro_amd import model_file

_cases = {}


def _case(model_dir, lmax):
    """Cu2AgO4 (3 types, triclinic, ragged degrees), small widths (S 32, U 16, MLP 32, read-out 16): l_max 1 and 3 with 2 layers, 2 with 3."""
    if lmax not in _cases:
        g = util.load_golden("Cu2AgO4_r5")
        cfg = dict(model_file.DEFAULT_CFG, type_names=["Ag", "Cu", "O"], l_max=lmax, num_layers=3 if lmax == 2 else 2, num_scalar_features=32,
                   num_tensor_features=16, mlp_width=32, readout_width=16, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]))
        _cases[lmax] = pp.PathCase(model_dir, f"emu_paths_l{lmax}", cfg, g["cell"], g["pos"], g["symbols"])
    return _cases[lmax]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lmax", [1, 2, 3])
def test_every_path_on_the_emulated_layer_kernels(emu_lib, model_dir, lmax, dtype):
    case = _case(model_dir, lmax)
    worst = 0.0
    for k, p, lll in pp.paths(case.cfg):
        worst = max(worst, case.check(emu_lib, k, p, dtype, "generic_f64" if dtype == "float64" else "generic_f32"))
    print(f"l_max {lmax} {dtype}: worst path-difference error / bar {worst:.3f}")


def _power_sample(cfg):
    every = pp.paths(cfg)
    if cfg["l_max"] < 3:
        return every
    return every[::3] + [e for e in every if e[0] == cfg["num_layers"]]      # l_max 3: a third of layer 1 (all l3) and the scalar paths


@pytest.mark.parametrize("lmax", [1, 2, 3])
def test_path_parity_has_the_power_to_see_one_wrong_coefficient(model_dir, lmax):
    case = _case(model_dir, lmax)
    for k, p, lll in _power_sample(case.cfg):
        _, ref, size = case.boost(k, p)
        for what, edit in pp.ctab_mutations(*lll, p):
            mutated = case.oracle_delta(k, p, edit)
            moved = max(np.abs(mutated[q] - ref[q]).max() / (pp.BAR["float32"] * np.abs(ref[q]).max() + pp.ROUNDING["float32"] * size[q])
                        for q in pp.QUANTITIES)
            assert moved >= 5.0, f"l_max {lmax} layer {k} path {p} {lll}: mutation {what} moves Delta by only {moved:.2f}x the float32 bar"
