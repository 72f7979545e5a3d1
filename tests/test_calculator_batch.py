"""ahip_compute_cells / Calculator.compute_many on the CPU emulation, float64: the eight structures of batch_cases.py in one call against the torch oracle of
every structure alone, with the bars of test_calculator.py (forces and per-atom energies atol 1e-9, energy rtol 1e-10, virial atol 1e-8).
The emulation launches threads one after the other, so its k_cells_reduce is one thread per structure without the LDS tree; the strided accumulation and the
tree of the device build are covered by test_gpu_cell_batch.py alone."""
import numpy as np
import pytest
import torch

import batch_cases as bc
import cell_cases as cc
from pair_allegro_amd import capi
from pair_allegro_amd.calculator import Calculator

DEV = torch.device("cpu")


def _check(out, ref, what=""):
    np.testing.assert_allclose(out["forces"], ref["forces"], rtol=0, atol=1e-9, err_msg=f"forces {what}")
    np.testing.assert_allclose(out["pe"], ref["pe"], rtol=1e-10, err_msg=f"energy {what}")
    np.testing.assert_allclose(out["virial"], ref["virial"], rtol=0, atol=1e-8, err_msg=f"virial {what}")
    np.testing.assert_allclose(out["eatom"], ref["eatom"], rtol=0, atol=1e-9, err_msg=f"eatom {what}")


@pytest.fixture(scope="module")
def case(emu_lib, model_dir):
    path, cfg, w = bc.model(model_dir, "float64", small=True)
    m = capi.Model(path, 0, emu_lib)
    structs = bc.structures()
    res, call = bc.run_batch(m, structs, cfg["type_names"])
    yield dict(path=path, cfg=cfg, w=w, m=m, structs=structs, res=res, call=call, refs=bc.references(cfg, w))
    m.close()


def test_every_structure_equals_its_oracle(case):
    assert case["call"]["path"] == "generic_f64"
    for name, out, ref in zip(bc.NAMES, case["res"], case["refs"]):
        _check(out, ref, name)
    empty, atom = case["res"][1], case["res"][5]
    assert empty["pe"] == 0.0 and not empty["virial"].any() and len(empty["forces"]) == 0
    assert atom["pe"] == float(case["w"]["shift"][0]) and not atom["forces"].any() and not atom["virial"].any()


def test_order_and_batch_size_do_not_matter(case):
    m, names = case["m"], case["cfg"]["type_names"]
    rev, _ = bc.run_batch(m, case["structs"][::-1], names)
    for name, out, ref in zip(bc.NAMES[::-1], rev, case["refs"][::-1]):
        _check(out, ref, name + " (reversed batch)")
    for k in (2, 3, 1):                                                # a batch of one: triclinic, the molecule outside its cell, the empty structure
        one, call = bc.run_batch(m, [case["structs"][k]], names)
        _check(one[0], case["refs"][k], bc.NAMES[k] + " (batch of one)")
        assert len(call["ghosts"]) == 1
    # the slab and the triclinic cell with every atom up to 1000 lattice vectors away along the periodic axes: the slab's extent along its open axis is
    # that of the wrapped atoms, and the neighbours in the batch are not disturbed
    rng = np.random.RandomState(12)
    far = []
    for k in (4, 2):
        cell, pos, sym, pbc = case["structs"][k]
        far.append((cell, pos + (rng.randint(-1000, 1001, size=pos.shape) * np.asarray(pbc)) @ cell, sym, pbc))
    out, call = bc.run_batch(m, [case["structs"][0], far[0], far[1], case["structs"][7]], names)
    for o, k in zip(out, (0, 4, 2, 7)):
        np.testing.assert_allclose(o["forces"], case["refs"][k]["forces"], rtol=0, atol=1e-8, err_msg=bc.NAMES[k] + " (far images)")   # (positions of 5e3 A carry 1e-12 A)
        np.testing.assert_allclose(o["pe"], case["refs"][k]["pe"], rtol=1e-9)
    assert np.array_equal(call["ghosts"], case["call"]["ghosts"][[0, 4, 2, 7]])
    none, call = bc.run_batch(m, [], names)                            # nstruct == 0
    assert none == [] and len(call["ghosts"]) == 0
    skin, _ = bc.run_batch(m, case["structs"], names, skin=0.7)        # the skin only inflates the shells and the list
    for name, out, ref in zip(bc.NAMES, skin, case["refs"]):
        _check(out, ref, name + " (skin 0.7)")


def test_ghost_contract(case, emu_lib, model_dir):
    border = cc.border_model(emu_lib, model_dir)
    bc.check_ghost_contract(case["call"], case["structs"], DEV, border, bc.R_MAX)
    g = case["call"]["ghosts"]
    assert g[0] == g[7] > 0 and g[1] == 0 and g[3] == 0 and g[5] == 3 and 0 < g[4] < g[2]          # (the lone atom sits near three faces of its cell)
    border.close()


def test_no_cross_talk(case):
    counts = bc.check_no_cross_talk(case["call"], case["structs"], bc.R_MAX)
    assert counts[0] == counts[7] > 0 and counts[1] == 0 and counts[5] == 0


def test_sums_equal_single_calls(case):
    m, names = case["m"], case["cfg"]["type_names"]
    e_sum, v_sum = 0.0, np.zeros(6)
    for k, (cell, pos, sym, pbc) in enumerate(case["structs"]):
        mt = np.array([names.index(s) for s in sym], dtype=np.int32)
        pe, f, ea, vir = m.compute_cell(pos, mt, cell, pbc)
        e_sum += pe
        v_sum += vir
        _check(case["res"][k], dict(forces=f, eatom=ea, pe=pe, virial=vir), bc.NAMES[k] + " (single call)")
    np.testing.assert_allclose(case["call"]["eng"].sum(), e_sum, rtol=1e-10)
    np.testing.assert_allclose(case["call"]["virial"].sum(axis=0), v_sum, rtol=0, atol=1e-8)


def test_compute_many(case, emu_lib):
    calc = Calculator(case["path"], lib=emu_lib)
    one = calc.compute_many(case["structs"])
    many = calc.compute_many(case["structs"], max_atoms=100)
    assert [r["info"]["batch"] for r in one] == [0] * 8
    assert [r["info"]["batch"] for r in many] == [0, 0, 0, 0, 0, 0, 1, 2]         # 4+0+7+21+7+1 = 40 atoms, then the 257 alone, then 4
    for name, a, b, ref, st in zip(bc.NAMES, one, many, case["refs"], case["structs"]):
        for r in (a, b):
            _check(dict(forces=r["forces"], eatom=r["atomic_energy"], pe=r["energy"], virial=r["virial"]), ref, name)
            assert (r["stress"] is None) == (not all(st[3])) and r["info"]["path"] == "generic_f64"
        assert a["info"]["nghost"] == b["info"]["nghost"]
    V = abs(np.linalg.det(case["structs"][2][0]))
    v = one[2]["virial"]
    np.testing.assert_allclose(one[2]["stress"] * V, -np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]]), rtol=0, atol=1e-12)
    # three-tuples default to a fully periodic cell; the single-structure method agrees
    single = calc.compute(*case["structs"][2][:3])
    np.testing.assert_allclose(calc.compute_many([case["structs"][2][:3]])[0]["forces"], single["forces"], rtol=0, atol=1e-9)
    bad = list(case["structs"])
    bad[4] = (bad[4][0], bad[4][1], ["Xx"] + bad[4][2][1:], bad[4][3])
    with pytest.raises(ValueError, match=r"structure 4.*Xx"):
        calc.compute_many(bad)
    assert calc.compute_many([]) == []
    calc.close()


def test_uneven_batch_is_split(case, emu_lib):
    """one huge open cell among small ones: three structures take 2 x 2 x 1 uniform slots of its extent (1283 + 5 A: 515 x 515 x 257 bins > 2^26); the library says
    "split the batch", compute_many halves (alone it needs 257^3 bins)"""
    far = (np.eye(3) * 10.0, np.array([[0.0, 0.0, 0.0], [1283.0, 1283.0, 1283.0]]), ["Cu", "Cu"], (0, 0, 0))
    structs = [far, case["structs"][0], case["structs"][2]]
    m, names = case["m"], case["cfg"]["type_names"]
    with pytest.raises(capi.AhipError, match="split the batch") as e:
        bc.run_batch(m, structs, names)
    assert e.value.code == capi.AHIP_ERR_ARG
    calc = Calculator(case["path"], lib=emu_lib)
    out = calc.compute_many(structs)
    assert [r["info"]["batch"] for r in out] == [0, 1, 1]
    for k, j in ((1, 0), (2, 2)):
        np.testing.assert_allclose(out[k]["forces"], case["refs"][j]["forces"], rtol=0, atol=1e-9)
    sh = float(case["w"]["shift"][0])
    np.testing.assert_allclose(out[0]["energy"], 2 * sh, rtol=1e-10)
    calc.close()


def test_errors_leave_f_untouched(case, emu_lib):
    m, names = case["m"], case["cfg"]["type_names"]
    first, x, mt, cells, pbc = bc.pack(case["structs"], names)
    _, before = bc.run_batch(m, case["structs"], names)

    def refused(match, **over):
        a = dict(first=first, x=x, mtype=mt, cells=cells, pbc=pbc)
        a.update(over)
        f = np.full((len(x), 3), cc.SENTINEL)
        with pytest.raises(capi.AhipError, match=match) as e:
            m.compute_cells(a["first"], a["x"], a["mtype"], a["cells"], a["pbc"], f=f)
        assert e.value.code == capi.AHIP_ERR_ARG
        assert np.all(f == cc.SENTINEL), "f was written"

    singular = cells.copy(); singular[2, 2] = singular[2, 0] + singular[2, 1]
    refused(r"structure 2\b.*singular", cells=singular)
    nan = cells.copy(); nan[6, 1, 1] = np.nan
    refused(r"structure 6\b.*non-finite", cells=nan)
    for badtype in (-1, len(names)):
        mt2 = mt.copy(); mt2[first[3] + 5] = badtype
        refused(r"structure 3, atom 5 has model type", mtype=mt2)
    down = first.copy(); down[4] = down[3] - 1                         # first[-1] stays: the arrays keep their length
    refused(r"non-decreasing.*structure 3\b", first=down)
    xbad = x.copy(); xbad[first[6] + 2, 1] = np.inf
    refused(r"structure 6, atom 2.*not finite", x=xbad)
    thin = cells.copy(); thin[0] *= 1e-4                               # 4 atoms x (2 ceil(5 / 3.61e-4) + 1)^3 images: beyond 32 bits
    refused(r"structure 0\b.*2\^31", cells=thin)
    # a call refused for its arguments leaves the accessors on the last successful batch
    np.testing.assert_array_equal(m.last_cells_ghosts(), before["ghosts"])
    np.testing.assert_array_equal(m.last_cell_rows(), before["rows"])
    # the model still evaluates afterwards
    res, _ = bc.run_batch(m, case["structs"], names)
    _check(res[2], case["refs"][2], "after the refused calls")
    calc = Calculator(case["path"], lib=emu_lib)
    with pytest.raises(ValueError, match="Xx"):
        calc.compute_many([(np.eye(3) * 9.0, np.zeros((1, 3)), ["Xx"])])
    calc.close()
