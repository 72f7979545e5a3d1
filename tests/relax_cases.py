"""FIRE relaxations (ahip_relax_cell), shared by the CPU-emulation tests (test_relax.py) and the GPU tests (test_gpu_relax.py): the algorithm of
include/allegro_hip.h in numpy over a force callback, with ASE's direct |dr|, the cases from fixed seeds whose every decision has a margin, and the checks of
one run."""
import numpy as np

import cell_reuse_cases as rc

SKIN = rc.SKIN
MARGIN = rc.MARGIN
SIGMA = 0.05                # jitter of the start, per coordinate [A]
FIRE = dict(dt_start=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)
# (name, geometry, pbc, fmax, max_steps, seed).  The random-weight models of every geometry but Cu-cubic do not converge: they wander, which is what exercises
# the rebuilds, so those run fmax = 0 for a fixed number of moves.  The seeds were chosen so that `fire` finds its asserts satisfied on the small float64 models of
# rc.small_case (CPU tests) and on the golden models (GPU tests) alike; the golden Cu-cubic model needs 59 moves to converge, the small one 21.
CASES = [
    ("Cu-cubic-relax", "Cu-cubic", (1, 1, 1), 0.02, 100, 3),
    ("Cu2AgO4-relax", "Cu2AgO4", (1, 1, 1), 0.0, 30, 4),
    ("Cu2AgO4-slab-relax", "Cu2AgO4", (1, 1, 0), 0.0, 30, 2),
    ("aspirin-relax", "aspirin", (0, 0, 0), 0.0, 30, 2),
]
BIG = ("CuPd-cubic-big-relax", "CuPd-cubic-big", (1, 1, 1), 0.0, 30, 1)
# the GPU tests add: 257 atoms (a thread block boundary and a partial wave in the row kernels) and a cell of one atom
BLOCK = ("CuPd-257-relax", "CuPd-257", (1, 1, 1), 0.0, 12, 1)
ONE = ("Cu-one-relax", "Cu-one", (1, 1, 1), 0.02, 100, 1)
SLAB = CASES[2]
FIXED = ("aspirin-fixed-relax", "aspirin", (0, 0, 0), 0.0, 30, 2)      # run with every third atom fixed


def start(spec):
    """cell, jittered start positions, symbols"""
    cell, pos, sym = rc.geometry(spec[1])
    return cell, pos + np.random.RandomState(spec[5]).normal(0.0, SIGMA, size=pos.shape), sym


def left_cell(cell, pos, pbc):
    """atoms whose fractional coordinate on a periodic axis is outside [0, 1)"""
    s = pos @ np.linalg.inv(cell)
    p = np.asarray(pbc, dtype=bool)
    return np.nonzero((((s < 0) | (s >= 1)) & p).any(axis=1))[0]


def fire(force, x0, fmax, max_steps, skin=SKIN, fixed=None, **par):
    """The algorithm of include/allegro_hip.h.  `force(x)` -> forces [n][3] at positions x (ghost forces folded home).  Rebuild rule: 2 U > skin against the
    positions of the last rebuild.  Asserts that every decision -- the sign of vf, max|F| against fmax, 2 U against skin -- has a relative margin of MARGIN.
    Returns dict(positions, forces, steps, converged, rebuilds, fmax, margin, margins): margin is the smallest one met, margins the smallest per decision."""
    par = dict(FIRE, **par)
    free = np.ones(len(x0), dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool)
    x, v = np.array(x0, dtype=np.float64), np.zeros_like(x0, dtype=np.float64)
    dt, alpha, npos, steps, rebuilds, worst = par["dt_start"], par["alpha_start"], 0, 0, 1, {}
    xhold = x.copy()

    def masked(x):
        raw = np.asarray(force(x), dtype=np.float64)
        return raw, raw * free[:, None]

    def margin(what, value):
        assert value >= MARGIN, f"move {steps}: a rounding could decide {what} (margin {value:.2e})"
        worst[what] = min(worst.get(what, np.inf), value)

    def largest(F):
        fm = float(np.linalg.norm(F, axis=1).max()) if len(F) else 0.0
        if fmax > 0 and len(F):
            margin("convergence", abs(fm - fmax) / fmax)
        return fm

    raw, F = masked(x)
    while steps < max_steps:
        U = float(np.linalg.norm(x - xhold, axis=1).max()) if len(x) else 0.0
        assert np.isfinite(U)
        margin("the rebuild", abs(2 * U - skin) / skin)
        if 2 * U > skin:                      # the forces of a rebuild are those of the same positions
            rebuilds += 1
            xhold = x.copy()
        vf, ff, vv = float(np.vdot(v, F)), float(np.vdot(F, F)), float(np.vdot(v, v))
        assert np.isfinite([vf, ff, vv]).all()
        if largest(F) <= fmax:
            break
        if vv > 0:
            margin("the sign of v.F", abs(vf) / np.sqrt(ff * vv))
        if vf > 0:
            c1, c2 = 1.0 - alpha, alpha * np.sqrt(vv / ff)
            if npos > par["n_min"]:
                dt = min(dt * par["f_inc"], par["dt_max"])
                alpha *= par["f_alpha"]
            npos += 1
        else:
            c1 = c2 = 0.0
            alpha, dt, npos = par["alpha_start"], dt * par["f_dec"], 0
        v = c1 * v + (c2 + dt) * F
        dr = dt * v
        norm = float(np.sqrt(np.vdot(dr, dr)))
        x = x + min(1.0, par["max_step"] / norm) * dr if norm > 0 else x
        steps += 1
        raw, F = masked(x)
    fm = largest(F)
    return dict(positions=x, forces=raw, steps=steps, converged=fm <= fmax, rebuilds=rebuilds, fmax=fm, margin=min(worst.values()), margins=worst)


def reference(spec, compute, fixed=None, **par):
    """`fire` of one case over compute(x) -> (energy, forces, eatom, virial) of a fresh evaluation; keeps the outputs of the last one.  The slab case must
    have an atom that has left the cell, so that a wrapped result cannot pass."""
    cell, x0, _ = start(spec)
    last = {}

    def force(x):
        out = compute(x)
        last.update(pe=out[0], forces=out[1], eatom=out[2], virial=out[3])
        return out[1]

    ref = fire(force, x0, spec[3], spec[4], fixed=fixed, **par)
    ref.update(pe=last["pe"], eatom=last["eatom"], virial=last["virial"])
    if spec[0] == SLAB[0]:
        assert len(left_cell(cell, ref["positions"], spec[2])) >= 1, "no atom of the slab case has left the cell"
    return ref


def expected_evaluations(info, max_steps):
    """check_every = 1: one evaluation at the start and one behind every move; a rebuild discards the evaluation in front of it and makes one of its own; the
    decision that finds the forces converged has one more behind it (the host enqueues the evaluation with the move, before it reads the state)"""
    stopped_converged = info["steps"] < max_steps
    return info["steps"] + 1 + 2 * (info["rebuilds"] - 1) + (1 if stopped_converged else 0)


def as_result(model, out):
    """(positions, energy, forces, eatom, virial, info) of relax_cell in the shape of rc.as_result"""
    rows = model.last_cell_rows()
    ei, rij = model.get_edges()
    return dict(positions=out[0], pe=out[1], forces=out[2], eatom=out[3], virial=out[4], info=out[5], edges=(ei[0], rows[ei[1]], rij), rows=rows)


def check_run(res, ref, pos_tol=1e-9, check=rc.check_tight):
    info = res["info"]
    assert (info["steps"], info["rebuilds"], info["converged"]) == (ref["steps"], ref["rebuilds"], ref["converged"]), (info, ref["steps"], ref["rebuilds"])
    np.testing.assert_allclose(res["positions"], ref["positions"], rtol=0, atol=pos_tol)
    check(res, ref)
    np.testing.assert_allclose(info["fmax"], ref["fmax"], rtol=0, atol=1e-9)


def check_hold(model, res, mt, cell, pbc, check=rc.check_tight, skin=SKIN):
    """after a success the model holds the list as ahip_compute_cell_reuse would: the next call at the returned positions reuses it"""
    out = model.compute_cell_reuse(res["positions"], mt, cell, pbc, skin)
    assert not out[4], "the hold of the relaxation was not used"
    check(dict(pe=out[0], forces=out[1], eatom=out[2], virial=out[3]), res)
