"""MD in one call (ahip_md_cell), shared by the CPU-emulation tests (test_md_onecall.py) and the GPU tests (test_gpu_md_onecall.py): the algorithm of
include/allegro_hip.h in numpy over a force callback -- BAOAB with the rebuild rule 2 U > skin against the positions of the last rebuild -- a numpy
Philox4x32-10 checked against the published Random123 vectors, the cases from fixed seeds whose every rebuild decision has a margin, and the checks of one run."""
import numpy as np

import cell_reuse_cases as rc
from pair_allegro_amd.units import FTM2V, KB, MVV2E, masses_of, maxwell_boltzmann

SKIN = 0.3
MARGIN = rc.MARGIN
DT = 0.002                  # ps
SIGMA = 0.05                # jitter of the start, per coordinate [A]
GAMMA = 5.0                 # 1 / ps, the Langevin variant of every case
BATH = 300.0                # K
VARIANTS = [("nve", 0.0), ("langevin", GAMMA)]
# (name, geometry, pbc, steps, temperature of the start velocities [K], seed).  The starts are hot: the atoms cross half the skin several times in a few dozen
# steps, which is what exercises the rebuilds.  The seeds were chosen so that `baoab` finds its asserts satisfied, for both variants, on the small float64 models
# of rc.small_case (CPU tests) and on the golden models (GPU tests) alike.
CASES = [
    ("Cu-cubic-md", "Cu-cubic", (1, 1, 1), 32, 3000.0, 1),
    ("Cu2AgO4-md", "Cu2AgO4", (1, 1, 1), 32, 1000.0, 1),
    ("Cu2AgO4-slab-md", "Cu2AgO4", (1, 1, 0), 32, 800.0, 1),
    ("aspirin-md", "aspirin", (0, 0, 0), 24, 40.0, 1),
]
BIG = ("CuPd-cubic-big-md", "CuPd-cubic-big", (1, 1, 1), 24, 1200.0, 1)
# the GPU tests add: 257 atoms (a thread block boundary and a partial wave in the row kernels) and a cell of one atom
BLOCK = ("CuPd-257-md", "CuPd-257", (1, 1, 1), 24, 1200.0, 1)
ONE = ("Cu-one-md", "Cu-one", (1, 1, 1), 40, 1500.0, 4)
SLAB = CASES[2]
SEED = 20261021             # the noise key of every Langevin run

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two; returns the four output words as uint64 arrays holding 32-bit values"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff) for v in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)]
    lo32, s32 = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & lo32, (p0 >> s32) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(W0)) & lo32, (k[1] + np.uint64(W1)) & lo32]
    return c


for _c, _k, _want in KNOWN_ANSWERS:
    assert tuple(int(v) for v in philox4x32_10(_c, _k)) == _want, "the numpy Philox4x32-10 misses a Random123 known answer"


def xi(seed, natoms, step):
    """the noise of include/allegro_hip.h for atoms 0 .. natoms-1 at one step: [natoms][3]"""
    atoms = np.arange(natoms, dtype=np.uint64)
    key = (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    z = []
    for j in (0, 1):
        w = philox4x32_10((atoms, np.full(natoms, int(step) & 0xffffffff, dtype=np.uint64), np.full(natoms, (int(step) >> 32) & 0xffffffff, dtype=np.uint64),
                           np.full(natoms, j, dtype=np.uint64)), key)
        u1 = (((w[0] << np.uint64(21)) | (w[1] >> np.uint64(11))).astype(np.float64) + 0.5) * 2.0 ** -53
        u2 = (((w[2] << np.uint64(21)) | (w[3] >> np.uint64(11))).astype(np.float64) + 0.5) * 2.0 ** -53
        rad = np.sqrt(-2.0 * np.log(u1))
        z.append((rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)))
    return np.stack([z[0][0], z[0][1], z[1][0]], axis=1)


def start(spec):
    """cell, jittered start positions, Maxwell-Boltzmann start velocities, masses, symbols"""
    cell, pos, sym = rc.geometry(spec[1])
    mass = masses_of(sym)
    rng = np.random.RandomState(spec[5])
    x0 = pos + rng.normal(0.0, SIGMA, size=pos.shape)
    v0 = maxwell_boltzmann(len(pos), mass, spec[4], spec[5] + 1000)
    if len(pos) == 1:                         # (zero total momentum would leave one atom at rest)
        v0 = np.sqrt(KB * spec[4] / (mass * MVV2E))[:, None] * rng.normal(size=(1, 3))
    return cell, x0, v0, mass, sym


def left_cell(cell, pos, pbc):
    """atoms whose fractional coordinate on a periodic axis is outside [0, 1)"""
    s = pos @ np.linalg.inv(cell)
    p = np.asarray(pbc, dtype=bool)
    return np.nonzero((((s < 0) | (s >= 1)) & p).any(axis=1))[0]


def baoab(compute, x0, v0, mass, nsteps, dt=DT, skin=SKIN, gamma=0.0, kT=0.0, seed=0, step0=0, fixed=None, sample_every=1, frame_every=0, ftm2v=FTM2V,
          mvv2e=MVV2E):
    """The algorithm of include/allegro_hip.h.  `compute(x)` -> (energy, forces [n][3], eatom, virial [6]) of a fresh evaluation at positions x.  Asserts that
    every decision 2 U against skin has a relative margin of MARGIN.  Returns dict(positions, velocities, pe, forces, eatom, virial, thermo [.][8], frames,
    steps, rebuilds, final_rebuilt, margin, path: the positions of every configuration)."""
    n_at = len(x0)
    free = np.ones(n_at, dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool)
    fr = free[:, None].astype(np.float64)
    m = np.asarray(mass, dtype=np.float64)[:, None]
    hdtf, c1 = 0.5 * dt * ftm2v, np.exp(-gamma * dt)
    c2 = np.sqrt(1.0 - c1 * c1)
    x, w = np.array(x0, dtype=np.float64), np.array(v0, dtype=np.float64)
    out = compute(x)
    xhold, rebuilds, worst, final_rebuilt = x.copy(), 1, np.inf, False
    thermo, frames, path = [], [], []
    for n in range(nsteps + 1):
        F = np.asarray(out[1], dtype=np.float64)
        U = float(np.linalg.norm(x - xhold, axis=1).max()) if n_at else 0.0
        assert np.isfinite(U)
        margin = abs(2 * U - skin) / skin
        assert margin >= MARGIN, f"step {n}: a rounding could decide the rebuild (margin {margin:.2e})"
        worst = min(worst, margin)
        if 2 * U > skin:                      # the forces of a rebuild are those of the same positions
            rebuilds += 1
            xhold = x.copy()
            final_rebuilt = n == nsteps
        v = (w + (hdtf * F / m if n > 0 else 0.0)) * fr
        assert np.isfinite(out[0]) and np.isfinite(F).all() and np.isfinite(v).all()
        if n % sample_every == 0:
            thermo.append(np.concatenate([[out[0], 0.5 * mvv2e * float((m * v * v).sum())], np.asarray(out[3], dtype=np.float64)]))
        if frame_every and n % frame_every == 0:
            frames.append(x.copy())
        path.append(x.copy())
        if n == nsteps:
            break
        vp = v + hdtf * F / m
        xh = x + 0.5 * dt * vp
        wn = (c1 * vp + c2 * np.sqrt(kT / (m * mvv2e)) * xi(seed, n_at, step0 + n) if gamma > 0 else vp) * fr
        x = np.where(free[:, None], xh + 0.5 * dt * wn, x)
        w = wn
        out = compute(x)
    return dict(positions=x, velocities=v, pe=out[0], forces=np.asarray(out[1]), eatom=out[2], virial=np.asarray(out[3]), thermo=np.array(thermo),
                frames=np.array(frames) if frame_every else None, steps=nsteps, rebuilds=rebuilds, final_rebuilt=final_rebuilt, margin=worst, path=path)


def reference(spec, gamma, compute, **kw):
    """`baoab` of one case and variant.  Every multi-atom case must count at least 2 rebuilds after the first; the slab case must have an atom that has left the
    cell, so that a wrapped result cannot pass."""
    cell, x0, v0, mass, _ = start(spec)
    kw = dict(dict(gamma=gamma, kT=KB * BATH, seed=SEED), **kw)
    ref = baoab(compute, x0, v0, mass, spec[3], **kw)
    if len(x0) > 1:
        assert ref["rebuilds"] >= 3, f"{spec[0]}: only {ref['rebuilds']} rebuilds"
    if spec[0] == SLAB[0]:
        assert len(left_cell(cell, ref["positions"], spec[2])) >= 1, "no atom of the slab case has left the cell"
    return ref


def expected_evaluations(ref):
    """check_every = 1: one evaluation at the start and one behind every step; a rebuild discards the evaluation in front of it and makes one of its own, but
    the final check has no evaluation behind it to discard"""
    return ref["steps"] + 1 + 2 * (ref["rebuilds"] - 1) - (1 if ref["final_rebuilt"] else 0)


def as_result(model, out):
    """(x, v, energy, forces, eatom, virial, thermo, frames, info) of md_cell in the shape of rc.as_result"""
    rows = model.last_cell_rows()
    ei, rij = model.get_edges()
    return dict(positions=out[0], velocities=out[1], pe=out[2], forces=out[3], eatom=out[4], virial=out[5], thermo=out[6], frames=out[7], info=out[8],
                edges=(ei[0], rows[ei[1]], rij), rows=rows)


def check_thermo(got, want):
    """pe and the virial at rc.check_tight's bars, ke at the energy's"""
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-10)
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(got[:, 2:], want[:, 2:], rtol=0, atol=1e-8)


def check_run(res, ref, dt=DT, pos_tol=1e-9, check=rc.check_tight):
    info = res["info"]
    assert (info["steps"], info["rebuilds"]) == (ref["steps"], ref["rebuilds"]), (info, ref["steps"], ref["rebuilds"])
    np.testing.assert_allclose(res["positions"], ref["positions"], rtol=0, atol=pos_tol)
    np.testing.assert_allclose(res["velocities"], ref["velocities"], rtol=0, atol=pos_tol / dt)
    check(res, ref)
    check_thermo(res["thermo"], ref["thermo"])
    if ref["frames"] is not None:
        np.testing.assert_allclose(res["frames"], ref["frames"], rtol=0, atol=pos_tol)


def check_hold(model, res, mt, cell, pbc, check=rc.check_tight, skin=SKIN):
    """after a success the model holds the list as ahip_compute_cell_reuse would: the next call at the returned positions reuses it"""
    out = model.compute_cell_reuse(res["positions"], mt, cell, pbc, skin)
    assert not out[4], "the hold of the MD run was not used"
    check(dict(pe=out[0], forces=out[1], eatom=out[2], virial=out[3]), res)
