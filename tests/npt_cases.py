"""MD at constant pressure in one call (ahip_npt_cell), shared by the CPU-emulation tests (test_npt_onecall.py) and the GPU tests (test_gpu_npt_onecall.py): the
algorithm of include/allegro_hip.h in numpy over a callback compute(x, cell) -- the BAOAB of md_onecall_cases inside the isotropic stochastic cell rescaling,
with the rebuild rule and U as ahip_compute_cell_reuse defines them -- the case tables, and the checks of one run.

The random-weight models have no equilibrium volume, so every case carries its own P0 near the virial pressure of its start; the small float64 models of
rc.small_case (CPU tests) and the golden models (GPU tests) have different virial pressures, so there are two tables.  The barostat is fast (tau_p = 0.03 ps):
in a few dozen steps the cell must really move, which is what exercises the cell term of the rebuild rule."""
import numpy as np

import cell_reuse_cases as rc
import md_onecall_cases as mc
from pair_allegro_amd.units import FTM2V, KB, MVV2E

SKIN = mc.SKIN              # 0.3 A
MARGIN = rc.MARGIN
DT = mc.DT                  # 0.002 ps
BETA = 1.6                  # A^3 / eV
TAU_P = 0.03                # ps
FULL = (1, 1, 1)
GAMMA = mc.GAMMA
BATH = mc.BATH
SEED = 20261021
VARIANTS = [("berendsen", 0.0, 0.0), ("npt", GAMMA, KB * BATH)]      # (name, gamma, kT)
V_WINDOW = (0.9, 1.1)       # V / V0 throughout
V_MOVES = 0.005             # max |V / V0 - 1| at least
NOISE_ATOM = 0xFFFFFFFF


def case(spec, p0, seed=SEED):
    return dict(name=spec[0].replace("-md", "-npt"), spec=spec, p0=p0, seed=seed, steps=spec[3])


# P0 in eV/A^3: the virial pressure of the start rounded to 0.01, found by running `reference` alone
SMALL = {
    "cubic": case(mc.CASES[0], 0.40),
    "triclinic": case(mc.CASES[1], 0.17),
    "big": case(mc.BIG, 0.13),
}
# The golden models (GPU), by `reference` over a float64 ahip_compute_cell; 257 atoms cross a thread-block boundary and leave a partial wave in the row kernels;
# with one atom the cell term sum_d M_d g_d alone decides the rebuilds.  Start pressures 0.122, -0.053, 0.031, 0.017 and 0.013 eV/A^3: P0 is near them, but far
# enough that the cell really moves (at 0.03 the 256-atom cell stays within 0.15 % of V0), and where the default seed left a decision of the "npt" variant
# without its margin, another seed.
GOLDEN = {
    "cubic": case(mc.CASES[0], 0.12, seed=20261024),
    "triclinic": case(mc.CASES[1], -0.06, seed=20261024),
    "big": case(mc.BIG, 0.0, seed=20261024),
    "block": case(mc.BLOCK, 0.02),
    "one": case(mc.ONE, 0.02),
}


def xi_v(seed, step):
    """xi_V of include/allegro_hip.h: the first component of xi at the atom word 0xFFFFFFFF"""
    key = (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    w = mc.philox4x32_10((NOISE_ATOM, int(step) & 0xffffffff, (int(step) >> 32) & 0xffffffff, 0), key)
    u1 = (float((int(w[0]) << 21) | (int(w[1]) >> 11)) + 0.5) * 2.0 ** -53
    u2 = (float((int(w[2]) << 21) | (int(w[3]) >> 11)) + 0.5) * 2.0 ** -53
    return float(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))


def start_pressure(compute, spec):
    """P of configuration 0"""
    cell, x0, v0, mass, _ = mc.start(spec)
    out = compute(x0, cell)
    ke = 0.5 * MVV2E * float((mass[:, None] * v0 * v0).sum())
    return (2.0 * ke + float(np.sum(out[3][:3]))) / (3.0 * abs(np.linalg.det(cell)))


def npt(compute, cell0, x0, v0, mass, nsteps, rcut, p0, beta=BETA, tau_p=TAU_P, dt=DT, skin=SKIN, gamma=0.0, kT=0.0, seed=0, step0=0, fixed=None, sample_every=1,
        frame_every=0, ftm2v=FTM2V, mvv2e=MVV2E, window=V_WINDOW):
    """The algorithm of include/allegro_hip.h.  `compute(x, cell)` -> (energy, forces, eatom, virial [6]) of a fresh evaluation; `rcut`: the largest cutoff of
    the model.  Asserts a relative margin of MARGIN on both inequalities of every rebuild decision and V / V0 within `window` throughout.  Returns dict(positions,
    velocities, cell, pe, forces, eatom, virial, thermo [.][10], frames, frame_cells, steps, rebuilds, final_rebuilt, margin, v_range, path, cells)."""
    n_at = len(x0)
    free = np.ones(n_at, dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool)
    fr = free[:, None].astype(np.float64)
    m = np.asarray(mass, dtype=np.float64)[:, None]
    hdtf, c1 = 0.5 * dt * ftm2v, np.exp(-gamma * dt)
    c2 = np.sqrt(1.0 - c1 * c1)
    noise = np.sqrt(2.0 * kT * beta * dt / tau_p)
    A = np.array(cell0, dtype=np.float64)
    V0 = abs(np.linalg.det(A))
    x, w = np.array(x0, dtype=np.float64), np.array(v0, dtype=np.float64)

    def take_hold():
        h0 = rc.heights(A)
        return dict(cell=A.copy(), x=rc.wrap(A, x, FULL), M=np.ceil((rcut + skin) / h0) + 1, hmin=h0.min())

    worst = {}

    def margin(what, value, n):
        assert value >= MARGIN, f"step {n}: a rounding could decide {what} (margin {value:.2e})"
        worst[what] = min(worst.get(what, np.inf), value)

    def reuse(hold, n):
        u = x - hold["x"]
        k = np.floor(u @ np.linalg.inv(A) + 0.5)
        U = float(np.linalg.norm(u - k @ A, axis=1).max())
        assert np.isfinite(U)
        g = np.linalg.norm(A - hold["cell"], axis=1)
        lhs = 2 * U + float((hold["M"] * g).sum())
        margin("2 U + sum M g against the skin", abs(lhs - skin) / skin, n)
        margin("sum g against the smallest height", abs(g.sum() - hold["hmin"]) / hold["hmin"], n)
        return lhs <= skin and g.sum() <= hold["hmin"]

    hold = take_hold()
    out = compute(x, A)
    rebuilds, final_rebuilt = 1, False
    thermo, frames, fcells, path, cells, ratios = [], [], [], [], [], []
    for n in range(nsteps + 1):
        F = np.asarray(out[1], dtype=np.float64)
        if not reuse(hold, n):                # the forces of a rebuild are those of the same configuration
            rebuilds += 1
            hold = take_hold()
            final_rebuilt = n == nsteps
        v = (w + (hdtf * F / m if n > 0 else 0.0)) * fr
        V = abs(np.linalg.det(A))
        ke = 0.5 * mvv2e * float((m * v * v).sum())
        W = np.asarray(out[3], dtype=np.float64)
        P = (2.0 * ke + W[0] + W[1] + W[2]) / (3.0 * V)
        assert np.isfinite(out[0]) and np.isfinite(F).all() and np.isfinite(v).all() and np.isfinite(P) and V > 0
        ratios.append(V / V0)
        assert window[0] <= V / V0 <= window[1], f"step {n}: V / V0 = {V / V0:.4f} has left {window}"
        if n % sample_every == 0:
            thermo.append(np.concatenate([[out[0], ke], W, [V, P]]))
        if frame_every and n % frame_every == 0:
            frames.append(x.copy())
            fcells.append(A.copy())
        path.append(x.copy())
        cells.append(A.copy())
        if n == nsteps:
            break
        de = -(beta / tau_p) * (p0 - P) * dt
        if noise > 0:
            de += noise / np.sqrt(V) * xi_v(seed, step0 + n)
        mu = float(np.exp(de / 3.0))
        vp = v + hdtf * F / m
        xh = x + 0.5 * dt * vp
        wd = c1 * vp + c2 * np.sqrt(kT / (m * mvv2e)) * mc.xi(seed, n_at, step0 + n) if gamma > 0 else vp
        x = mu * np.where(free[:, None], xh + 0.5 * dt * wd, x)
        w = wd * fr / mu
        A = mu * A
        out = compute(x, A)
    return dict(positions=x, velocities=v, cell=A, pe=out[0], forces=np.asarray(out[1]), eatom=out[2], virial=np.asarray(out[3]), thermo=np.array(thermo),
                frames=np.array(frames) if frame_every else None, frame_cells=np.array(fcells) if frame_every else None, steps=nsteps, rebuilds=rebuilds,
                final_rebuilt=final_rebuilt, margin=min(worst.values()), margins=worst, v_range=(min(ratios), max(ratios)), path=path, cells=cells)


def reference(case_, variant, compute, rcut, **kw):
    """`npt` of one case and variant, with the conditions the reference alone must meet: the volume stays within V_WINDOW and really moves, at least 3 rebuilds
    (2 for one atom), and the margin at every decision (asserted inside `npt`)."""
    spec = case_["spec"]
    cell, x0, v0, mass, _ = mc.start(spec)
    kw = dict(dict(gamma=variant[1], kT=variant[2], seed=case_["seed"]), **kw)
    ref = npt(compute, cell, x0, v0, mass, case_["steps"], rcut, case_["p0"], **kw)
    lo, hi = ref["v_range"]
    assert max(abs(lo - 1.0), abs(hi - 1.0)) >= V_MOVES, f"{case_['name']}: the cell hardly moves (V / V0 in {ref['v_range']})"
    need = 3 if len(x0) > 1 else 2
    assert ref["rebuilds"] >= need, f"{case_['name']}: only {ref['rebuilds']} rebuilds"
    assert ref["margin"] >= MARGIN
    return ref


def expected_evaluations(ref):
    return mc.expected_evaluations(ref)


def run(model, case_, variant, mt, **over):
    """the case through ahip_npt_cell, in the shape of rc.as_result plus positions, velocities, cell, thermo, frames, frame_cells and info"""
    spec = case_["spec"]
    cell, x0, v0, mass, _ = mc.start(spec)
    kw = dict(dict(nsteps=case_["steps"], dt=DT, gamma=variant[1], kT=variant[2], seed=case_["seed"], pressure=case_["p0"], compressibility=BETA, tau_p=TAU_P), **over)
    return as_result(model, model.npt_cell(kw.pop("x", x0), kw.pop("v", v0), mt, mass, kw.pop("cell", cell), FULL, SKIN, **kw))


def as_result(model, out):
    rows = model.last_cell_rows()
    ei, rij = model.get_edges()
    return dict(positions=out[0], velocities=out[1], pe=out[2], forces=out[3], eatom=out[4], virial=out[5], thermo=out[6], frames=out[7], info=out[8], cell=out[9],
                frame_cells=out[10], edges=(ei[0], rows[ei[1]], rij), rows=rows)


def check_thermo(got, want):
    """pe, ke and the virial at the bars of md_onecall_cases.check_thermo; V and P at rtol 1e-10"""
    assert got.shape == want.shape, (got.shape, want.shape)
    mc.check_thermo(got[:, :8], want[:, :8])
    np.testing.assert_allclose(got[:, 8:], want[:, 8:], rtol=1e-10, atol=0)


def check_run(res, ref, dt=DT, pos_tol=1e-9, check=rc.check_tight):
    info = res["info"]
    assert (info["steps"], info["rebuilds"]) == (ref["steps"], ref["rebuilds"]), (info, ref["steps"], ref["rebuilds"])
    np.testing.assert_allclose(res["positions"], ref["positions"], rtol=0, atol=pos_tol)
    np.testing.assert_allclose(res["cell"], ref["cell"], rtol=0, atol=pos_tol)
    np.testing.assert_allclose(res["velocities"], ref["velocities"], rtol=0, atol=pos_tol / dt)
    check(res, ref)
    check_thermo(res["thermo"], ref["thermo"])
    if ref["frames"] is not None:
        np.testing.assert_allclose(res["frames"], ref["frames"], rtol=0, atol=pos_tol)
        np.testing.assert_allclose(res["frame_cells"], ref["frame_cells"], rtol=0, atol=pos_tol)


def check_hold(model, res, mt, check=rc.check_tight, skin=SKIN):
    """after a success the model holds the list of the last rebuild: the next reuse call at the returned positions and cell runs on it"""
    out = model.compute_cell_reuse(res["positions"], mt, res["cell"], FULL, skin)
    assert not out[4], "the hold of the run was not used"
    check(dict(pe=out[0], forces=out[1], eatom=out[2], virial=out[3]), res)
