"""GPU: ahip_compute_cells on the MI355X.  The eight structures of batch_cases.py in one call, float32 full-width model S (six types) so that the fused kernel
runs: against the float64 torch oracle of every structure alone, against single ahip_compute_cell calls of the same library, the ghost contract and the
no-cross-talk check on the device, run-to-run identity of the energies, the layer-at-a-time path, and a 20-type model whose active set is the union of the
types present.
k_cells_reduce runs here as the device runs it -- 256 threads striding over the rows, then the tree in LDS; big-257 has more rows than threads -- which the
CPU emulation cannot do: it launches threads one after the other, so its build of the kernel is a single thread per structure without the tree."""
import numpy as np
import pytest
import torch

import batch_cases as bc
import cell_cases as cc
import parity_cases as pc
import util
from pair_allegro_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(hip_lib, model_dir):
    path, cfg, w = bc.model(model_dir, "float32", small=False)
    m = capi.Model(path, 0, hip_lib)
    structs = bc.structures()
    res, call = bc.run_batch(m, structs, cfg["type_names"], skin=1.0)
    yield dict(path=path, cfg=cfg, w=w, m=m, structs=structs, res=res, call=call)
    m.close()


def _tol(name):
    """against the float64 oracle only; two evaluations of the same library are compared at pc.TOL["float32"] as it is"""
    return pc.TOL["float32"] * (23 if name.startswith("aspirin") else 1)          # the factor test_gpu_cell.py grants the molecule (kcal/mol-scale forces)


def test_batch_equals_the_oracle(case):
    assert case["call"]["path"].startswith("fused_"), case["call"]["path"]
    refs = bc.references(case["cfg"], case["w"])
    for name, out, ref in zip(bc.NAMES, case["res"], refs):
        df = float(np.abs(out["forces"] - ref["forces"]).max()) if len(ref["forces"]) else 0.0
        print(f"{name}: n={len(ref['forces'])} max|dF|={df:.3e} |dE|={abs(out['pe'] - ref['pe']):.3e} max|dV|={np.abs(out['virial'] - ref['virial']).max():.3e}")
        util.assert_close_to(out, ref, _tol(name), what=f"{name} in the batch")
        if not name.startswith("aspirin"):
            assert df < pc.NORTH_STAR_DF
    assert case["res"][1]["pe"] == 0.0 and not case["res"][1]["virial"].any()


def test_batch_equals_single_calls(case):
    m, names = case["m"], case["cfg"]["type_names"]
    rs, ei = bc.row_structure(case["call"]), case["call"]["edges"][0]
    for k, (name, (cell, pos, sym, pbc)) in enumerate(zip(bc.NAMES, case["structs"])):
        mt = np.array([names.index(s) for s in sym], dtype=np.int32)
        pe, f, ea, vir = m.compute_cell(pos, mt, cell, pbc, skin=1.0)
        nedges = m.get_edges()[0].shape[1] if len(pos) else 0
        assert m.last_path.startswith("fused_") or len(pos) == 0
        util.assert_close_to(case["res"][k], dict(forces=f, eatom=ea, pe=pe, virial=vir), pc.TOL["float32"], what=f"{name}: batch against its single call")
        assert int((rs[ei[0]] == k).sum()) == nedges, name


def test_ghost_contract_and_no_cross_talk(case, hip_lib, model_dir):
    border = cc.border_model(hip_lib, model_dir, "float32")
    bc.check_ghost_contract(case["call"], case["structs"], torch.device("cuda", 0), border, bc.R_MAX + 1.0)
    border.close()
    counts = bc.check_no_cross_talk(case["call"], case["structs"], bc.R_MAX)
    assert counts[0] == counts[7] > 0 and counts[1] == 0 and counts[5] == 0


def test_same_batch_twice_is_bit_identical(case):
    """per-atom energies are deterministic in the kernels and the per-structure reduction has a fixed order"""
    _, a = bc.run_batch(case["m"], case["structs"], case["cfg"]["type_names"], skin=1.0)
    _, b = bc.run_batch(case["m"], case["structs"], case["cfg"]["type_names"], skin=1.0)
    for call in (a, b):
        assert np.array_equal(call["eng"], case["call"]["eng"]) and np.array_equal(call["eatom"], case["call"]["eatom"])
        assert np.array_equal(call["ghosts"], case["call"]["ghosts"]) and np.array_equal(call["rows"], case["call"]["rows"])


def test_generic_path_same_batch(case, hip_lib):
    """the row-sum virial does not depend on the kernel path"""
    m = capi.Model(case["path"], 0, hip_lib)
    m.set_option("path", "generic")
    res, call = bc.run_batch(m, case["structs"], case["cfg"]["type_names"], skin=1.0)
    assert call["path"].startswith("generic"), call["path"]
    refs = bc.references(case["cfg"], case["w"])
    for name, out, ref, fused in zip(bc.NAMES, res, refs, case["res"]):
        util.assert_close_to(out, ref, _tol(name), what=f"{name} generic path")
        util.assert_close_to(out, fused, pc.TOL["float32"], what=f"{name} generic against fused")
    m.close()


def test_twenty_types_union_of_the_types_present(hip_lib, model_dir):
    names = ["Cu", "Ag", "O"] + [f"X{k}" for k in range(17)]
    names = names[3:10] + ["Cu"] + names[10:15] + ["Ag"] + names[15:] + ["O"]          # the three types in use are spread over the 20
    path, cfg, w = bc.model(model_dir, "float32", small=False, type_names=names)
    structs = [bc.structures()[k] for k in (0, 1, 2, 4)]                               # Cu alone, empty, Cu2AgO4, its slab
    m = capi.Model(path, 0, hip_lib)
    res, call = bc.run_batch(m, structs, names, skin=1.0)
    assert call["path"].startswith("fused_"), call["path"]
    g = capi.Model(path, 0, hip_lib)
    g.set_option("path", "generic")
    ref, gcall = bc.run_batch(g, structs, names, skin=1.0)
    assert gcall["path"].startswith("generic")
    for k, (out, r) in enumerate(zip(res, ref)):
        util.assert_close_to(out, r, pc.TOL["float32"], what=f"20 types, structure {k}")
    m.close(); g.close()
