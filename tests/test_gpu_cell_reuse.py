"""GPU: ahip_compute_cell_reuse.  The row-refresh kernel (csrc/neigh.hip: k_cell_refresh) and the hold in float64 against a fresh ahip_compute_cell on a second
handle at every step of the CPU tests' trajectories, plus 257 atoms (a block boundary) and a cell of one atom; the float32 golden models on the fused kernels
against those float64 results; and everything that must end a hold."""
import numpy as np
import pytest

import cell_reuse_cases as rc
import parity_cases as pc
import util
from pair_allegro_amd import capi

pytestmark = pytest.mark.gpu
F64_SPECS = rc.SEQUENCES + [rc.BIG_WALK, rc.BLOCK_WALK, rc.ONE_WALK]
F32_SPECS = [rc.SEQUENCES[0], rc.SEQUENCES[1], rc.SEQUENCES[3], rc.BIG_WALK]
_ref = {}


def _golden(geom, model_dir):
    g = util.load_golden(rc.GOLDEN_OF.get(geom, geom) + "_r5")
    path, cfg, _ = util.golden_model(g, model_dir, "float32")
    _, _, sym = rc.geometry(geom)
    return path, cfg, np.array([cfg["type_names"].index(s) for s in sym], dtype=np.int32)


def _reference(hip_lib, model_dir, spec):
    """the trajectory, its expected flags and, per step, a fresh ahip_compute_cell in float64 on a handle of its own: computed once, shared, never modified"""
    if spec[0] not in _ref:
        path, cfg, mt = _golden(spec[1], model_dir)
        fresh = capi.Model(path, 0, hip_lib)
        fresh.set_option("precision", "float64")
        steps, flags = rc.sequence(spec, rc.largest_cutoff(fresh) + rc.SKIN)
        res = [rc.as_result(fresh, fresh.compute_cell(pos, mt, cell, spec[2], rc.SKIN)) for cell, pos in steps]
        assert fresh.last_path == "generic_f64"
        fresh.close()
        _ref[spec[0]] = (steps, flags, res)
    return _ref[spec[0]]


@pytest.mark.parametrize("spec", F64_SPECS, ids=[s[0] for s in F64_SPECS])
def test_float64_trajectory_equals_fresh_calls(hip_lib, model_dir, spec):
    steps, flags, ref = _reference(hip_lib, model_dir, spec)
    path, cfg, mt = _golden(spec[1], model_dir)
    model = capi.Model(path, 0, hip_lib)
    model.set_option("precision", "float64")
    got, worst = [], 0.0
    for (cell, pos), want in zip(steps, ref):
        out = model.compute_cell_reuse(pos, mt, cell, spec[2], rc.SKIN)
        got.append(out[4])
        res = rc.as_result(model, out)
        worst = max(worst, float(np.abs(res["forces"] - want["forces"]).max()))
        rc.check_tight(res, want)
        rc.check_edges(res, cell, pos, spec[2], cfg["r_max"])
    print(f"{spec[0]}: rebuilt {''.join(str(int(f)) for f in got)} rows={len(res['rows'])} max|dF| against fresh calls {worst:.3e}")
    assert got == flags
    assert model.cell_reuse_stats() == (len(steps), sum(flags))
    model.close()


@pytest.mark.parametrize("spec", F32_SPECS, ids=[s[0] for s in F32_SPECS])
def test_float32_golden_models_on_the_fused_kernels(hip_lib, model_dir, spec):
    """the bars of test_gpu_cell.py::test_compute_cell_equals_the_golden, against the float64 evaluation of the same step"""
    steps, flags, ref = _reference(hip_lib, model_dir, spec)
    path, cfg, mt = _golden(spec[1], model_dir)
    model = capi.Model(path, 0, hip_lib)
    tol = pc.TOL["float32"] * (23 if spec[1] == "aspirin" else 1)
    got, worst = [], 0.0
    for k, ((cell, pos), want) in enumerate(zip(steps, ref)):
        out = model.compute_cell_reuse(pos, mt, cell, spec[2], rc.SKIN)
        got.append(out[4])
        res = rc.as_result(model, out)
        df = float(np.abs(res["forces"] - want["forces"]).max())
        worst = max(worst, df)
        assert model.last_path.startswith("fused_"), (k, model.last_path)
        util.assert_close_to(res, want, tol, what=f"{spec[0]} step {k}")
        if spec[1] != "aspirin":
            assert df < pc.NORTH_STAR_DF, (k, df)
        assert len(res["edges"][0]) == len(want["edges"][0])
    print(f"{spec[0]}: path={model.last_path} rebuilt {''.join(str(int(f)) for f in got)} max|dF| against float64 {worst:.3e}")
    assert got == flags
    model.close()


def test_what_ends_a_hold(hip_lib, model_dir):
    path, cfg, mt = _golden("Cu2AgO4", model_dir)
    cell, pos, _ = rc.geometry("Cu2AgO4")
    model, fresh = capi.Model(path, 0, hip_lib), capi.Model(path, 0, hip_lib)
    tol = pc.TOL["float32"]

    def check(res, cell, pos, mt, pbc):
        want = rc.as_result(fresh, fresh.compute_cell(pos, mt, cell, pbc, rc.SKIN))
        util.assert_close_to(res, want, tol, what="against a fresh ahip_compute_cell")
        assert sorted(zip(*[e.tolist() for e in res["edges"][:2]])) == sorted(zip(*[e.tolist() for e in want["edges"][:2]]))

    rc.check_invalidation(model, mt, cell, pos, check)
    assert model.last_path.startswith("fused_")
    model.close(); fresh.close()
