"""Variable-cell FIRE relaxations (ahip_relax_vcell), shared by the CPU-emulation tests (test_relax_vcell.py) and the GPU tests (test_gpu_relax_vcell.py): the
algorithm of include/allegro_hip.h in numpy over a callback compute(x, cell), with the rebuild rule and U as ahip_compute_cell_reuse defines them, the case
tables, and the checks of one run.

The random-weight models have no equilibrium volume: without an external pressure they expand until the atoms leave each other's cutoff.  Every case therefore
carries a pressure under which the reference alone stays within 0.8 <= det D <= 1.25 and finds a margin on every decision; the small float64 models of
rc.small_case (CPU tests) and the golden models (GPU tests) need different ones, so there are two tables."""
import numpy as np

import cell_reuse_cases as rc
import relax_cases as xc

SKIN = rc.SKIN
MARGIN = rc.MARGIN
SIGMA = xc.SIGMA
FIRE = xc.FIRE
FULL = (1, 1, 1)
DET_WINDOW = (0.8, 1.25)
ALL_STRAINS = (1, 1, 1, 1, 1, 1)


def case(name, geom, pressure, fmax, smax, max_steps, seed, **par):
    return dict(name=name, geom=geom, pressure=pressure, fmax=fmax, smax=smax, max_steps=max_steps, seed=seed, par=par)


# The small float64 models (CPU emulation).  Pressures in eV/A^3, found by running `reference` alone.
SMALL = {
    "cubic": case("Cu-cubic-vcell", "Cu-cubic", 0.35, 0.02, 1e-3, 100, 3),
    "hydrostatic": case("Cu-cubic-vcell-hydrostatic", "Cu-cubic", 0.35, 0.02, 1e-3, 100, 3, hydrostatic=True),
    "triclinic": case("Cu2AgO4-vcell", "Cu2AgO4", 0.15, 0.0, 0.0, 30, 4),
    "big": case("CuPd-cubic-big-vcell", "CuPd-cubic-big", 0.2, 0.0, 0.0, 24, 1),
}
# The golden models (GPU); 257 atoms cross a thread-block boundary and leave a partial wave in the row kernels; one atom with c = 1 feels no force, so the
# cell term sum_d M_d g_d alone decides its rebuilds.
GOLDEN = {
    "cubic": case("Cu-cubic-vcell", "Cu-cubic", 0.10, 0.02, 1e-3, 150, 3),
    "hydrostatic": case("Cu-cubic-vcell-hydrostatic", "Cu-cubic", 0.10, 0.02, 1e-3, 150, 3, hydrostatic=True),
    "triclinic": case("Cu2AgO4-vcell", "Cu2AgO4", -0.075, 0.0, 0.0, 30, 4),
    "big": case("CuPd-cubic-big-vcell", "CuPd-cubic-big", 0.02, 0.0, 0.0, 30, 1, cell_factor=32.0),
    "block": case("CuPd-257-vcell", "CuPd-257", 0.01, 0.0, 0.0, 12, 1, cell_factor=8.0),
    "one": case("Cu-one-vcell", "Cu-one", 0.005, 0.0, 0.0, 12, 1, cell_factor=1.0),
}


def start(spec):
    """cell, jittered start positions, symbols"""
    cell, pos, sym = rc.geometry(spec["geom"])
    return cell, pos + np.random.RandomState(spec["seed"]).normal(0.0, SIGMA, size=pos.shape), sym


def sym3(v):
    return np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]], dtype=np.float64)


def w_ext(virial, cell, pressure=0.0, hydrostatic=False, mask=ALL_STRAINS):
    """(W_ext, V) of include/allegro_hip.h"""
    V = abs(np.linalg.det(cell))
    W = sym3(virial) - pressure * V * np.eye(3)
    if hydrostatic:
        W = np.trace(W) / 3.0 * np.eye(3)
    return W * sym3(np.asarray(mask, dtype=bool).astype(np.float64)), V


def fire(compute, cell0, x0, rcut, fmax, smax, max_steps, pressure=0.0, skin=SKIN, fixed=None, hydrostatic=False, mask=ALL_STRAINS, cell_factor=None,
         window=DET_WINDOW, **par):
    """The algorithm of include/allegro_hip.h.  `compute(x, cell)` -> (energy, forces, eatom, virial) of a fresh evaluation; `rcut`: the largest cutoff of the
    model.  Asserts a relative margin of MARGIN on every decision -- the sign of v.G, max |F| against fmax, max |W_ext| / V against smax, and both inequalities
    of the reuse criterion -- and det D within `window` throughout.  Returns dict(positions, cell, D, q, forces, pe, eatom, virial, steps, converged, rebuilds,
    last_check_rebuilt, fmax, smax, margin, margins, det_range)."""
    par = dict(FIRE, **par)
    n = len(x0)
    free = np.ones(n, dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool)
    c = float(cell_factor) if cell_factor else float(n)
    A0 = np.array(cell0, dtype=np.float64)
    D, vD = np.eye(3), np.zeros((3, 3))
    q, v = np.array(x0, dtype=np.float64), np.zeros((n, 3))
    dt, alpha, npos, steps, rebuilds, worst = par["dt_start"], par["alpha_start"], 0, 0, 1, {}
    dets = [1.0]

    def margin(what, value):
        assert value >= MARGIN, f"move {steps}: a rounding could decide {what} (margin {value:.2e})"
        worst[what] = min(worst.get(what, np.inf), value)

    def config():
        return q @ D.T, A0 @ D.T

    def evaluate():
        x, A = config()
        return compute(x, A)

    def take_hold():
        x, A = config()
        h0 = rc.heights(A)
        return dict(cell=A.copy(), x=rc.wrap(A, x, FULL), M=np.ceil((rcut + skin) / h0) + 1, hmin=h0.min())

    def reuse(hold):
        """the criterion of ahip_compute_cell_reuse for the current configuration against the hold"""
        x, A = config()
        u = x - hold["x"]
        k = np.floor(u @ np.linalg.inv(A) + 0.5)
        U = float(np.linalg.norm(u - k @ A, axis=1).max())
        assert np.isfinite(U)
        g = np.linalg.norm(A - hold["cell"], axis=1)
        lhs = 2 * U + float((hold["M"] * g).sum())
        margin("2 U + sum M g against the skin", abs(lhs - skin) / skin)
        margin("sum g against the smallest height", abs(g.sum() - hold["hmin"]) / hold["hmin"])
        return lhs <= skin and g.sum() <= hold["hmin"]

    def measures(out):
        """(largest Cartesian force on a free atom, max |W_ext| / V, W_ext), with their margins"""
        W, V = w_ext(out[3], config()[1], pressure, hydrostatic, mask)
        F = np.asarray(out[1], dtype=np.float64) * free[:, None]
        fm, sm = float(np.linalg.norm(F, axis=1).max()), float(np.abs(W).max() / V)
        assert np.isfinite([fm, sm, V]).all()
        if fmax > 0:
            margin("max |F| against fmax", abs(fm - fmax) / fmax)
        if smax > 0:
            margin("max |W_ext| / V against smax", abs(sm - smax) / smax)
        return fm, sm, W

    hold = take_hold()
    out = evaluate()
    last_check_rebuilt = False
    while True:
        last_check_rebuilt = False
        if steps == 0 and max_steps == 0:
            break
        if not reuse(hold):                   # the forces of a rebuild are those of the same configuration
            rebuilds += 1
            hold = take_hold()
            last_check_rebuilt = steps == max_steps
        detD = float(np.linalg.det(D))
        assert window[0] <= detD <= window[1], f"move {steps}: det D = {detD:.4f} has left {window}"
        fm, sm, W = measures(out)
        if (fm <= fmax and sm <= smax) or steps == max_steps:
            break
        F = np.asarray(out[1], dtype=np.float64) * free[:, None]
        G, GD = F @ D, W @ np.linalg.inv(D).T / c
        vf = float(np.vdot(v, G) + np.vdot(vD, GD))
        ff = float(np.vdot(G, G) + np.vdot(GD, GD))
        vv = float(np.vdot(v, v) + np.vdot(vD, vD))
        assert np.isfinite([vf, ff, vv]).all()
        if vv > 0:
            margin("the sign of v.G", abs(vf) / np.sqrt(ff * vv))
        if vf > 0:
            c1, c2 = 1.0 - alpha, alpha * np.sqrt(vv / ff)
            if npos > par["n_min"]:
                dt = min(dt * par["f_inc"], par["dt_max"])
                alpha *= par["f_alpha"]
            npos += 1
        else:
            c1 = c2 = 0.0
            alpha, dt, npos = par["alpha_start"], dt * par["f_dec"], 0
        v, vD = c1 * v + (c2 + dt) * G, c1 * vD + (c2 + dt) * GD
        norm = dt * float(np.sqrt(np.vdot(v, v) + np.vdot(vD, vD)))          # ASE's |dr| over all natoms + 3 rows
        s = min(1.0, par["max_step"] / norm) if norm > 0 else 1.0
        q, D = q + s * dt * v, D + s * dt * vD / c
        dets.append(float(np.linalg.det(D)))
        steps += 1
        out = evaluate()
    x, A = config()
    if max_steps == 0:
        fm, sm, _ = measures(out)
    return dict(positions=x, cell=A, D=D, q=q, pe=out[0], forces=np.asarray(out[1]), eatom=out[2], virial=np.asarray(out[3]), steps=steps,
                converged=bool(fm <= fmax and sm <= smax), rebuilds=rebuilds, last_check_rebuilt=last_check_rebuilt, fmax=fm, smax=sm,
                margin=min(worst.values()) if worst else np.inf, margins=worst, det_range=(min(dets), max(dets)))


def reference(spec, compute, rcut, **over):
    """`fire` of one case over compute(x, cell)"""
    cell, x0, _ = start(spec)
    kw = dict(spec["par"], **over)
    return fire(compute, cell, x0, rcut, spec["fmax"], spec["smax"], spec["max_steps"], pressure=spec["pressure"], **kw)


def run(model, spec, mt, check_every=4, **over):
    """the case through ahip_relax_vcell, in the shape of rc.as_result plus positions, cell and info"""
    cell, x0, _ = start(spec)
    kw = dict(dict(fmax=spec["fmax"], smax=spec["smax"], max_steps=spec["max_steps"], pressure=spec["pressure"], check_every=check_every), **spec["par"])
    kw.update(over)
    return as_result(model, model.relax_vcell(x0, mt, cell, FULL, SKIN, **kw))


def as_result(model, out):
    rows = model.last_cell_rows()
    ei, rij = model.get_edges()
    return dict(positions=out[0], pe=out[1], forces=out[2], eatom=out[3], virial=out[4], info=out[5], cell=out[6], edges=(ei[0], rows[ei[1]], rij), rows=rows)


def expected_evaluations(info, ref, max_steps):
    """The rule of relax_cases.expected_evaluations at check_every = 1; a rebuild that the check of the last configuration asks for (no move is left) has no
    discarded evaluation behind it."""
    return xc.expected_evaluations(info, max_steps) - (1 if ref["last_check_rebuilt"] else 0)


def check_run(res, ref, pos_tol=1e-9, check=rc.check_tight):
    """moves, rebuilds and the converged flag equal; positions and the nine cell entries to pos_tol; energy, forces and virial by `check`"""
    info = res["info"]
    assert (info["steps"], info["rebuilds"], info["converged"]) == (ref["steps"], ref["rebuilds"], ref["converged"]), (info, ref["steps"], ref["rebuilds"])
    np.testing.assert_allclose(res["positions"], ref["positions"], rtol=0, atol=pos_tol)
    np.testing.assert_allclose(res["cell"], ref["cell"], rtol=0, atol=pos_tol)
    check(res, ref)
    np.testing.assert_allclose(info["fmax"], ref["fmax"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(info["smax"], ref["smax"], rtol=0, atol=1e-9)


def check_hold(model, res, mt, check=rc.check_tight, skin=SKIN):
    """after a success the model holds the list of the last rebuild: the next reuse call at the returned positions and cell runs on it"""
    out = model.compute_cell_reuse(res["positions"], mt, res["cell"], FULL, skin)
    assert not out[4], "the hold of the relaxation was not used"
    check(dict(pe=out[0], forces=out[1], eatom=out[2], virial=out[3]), res)
