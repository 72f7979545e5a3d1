"""Energy, forces and stress of one structure without LAMMPS: "cell, positions, species" in, one call into the library
(ahip_compute_cell: wrap, ghost images, neighbor list and model evaluation all on the device) out.

    from pair_allegro_amd.calculator import Calculator
    calc = Calculator("model.nequip.pth")
    out = calc.compute(cell, positions, symbols)          # out["energy"], out["forces"], out["stress"]
    outs = calc.compute_many([(cell, positions, symbols), ...])      # a data set: one library call for many structures (ahip_compute_cells)
    calc = Calculator("model.nequip.pth", skin=1.0, reuse=True)      # a trajectory: ghosts and neighbor list are kept from call to call (ahip_compute_cell_reuse)
    out = calc.relax(cell, positions, symbols, fmax=0.05)            # a FIRE relaxation at fixed cell in one library call (ahip_relax_cell): out["positions"]
    out = calc.relax(cell, positions, symbols, variable_cell=True, pressure=0.01)      # ... of positions and cell (ahip_relax_vcell): out["cell"] too
    out = calc.md(cell, positions, symbols, steps=1000, dt=0.001, temperature=300.0, friction=5.0)      # MD in one library call (ahip_md_cell): out["thermo"]
    out = calc.md(cell, positions, symbols, steps=1000, temperature=300.0, friction=5.0, pressure=0.0, compressibility=1.6, tau_p=1.0)     # ... at constant pressure (ahip_npt_cell): out["cell"]

Any cell works: triclinic, thinner than the cutoff (several images per direction), open axes.  No ASE import: an ASE calculator is three lines
around `compute(atoms.cell.array, atoms.positions, atoms.get_chemical_symbols(), atoms.pbc)`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import capi
from .units import FTM2V, KB, MVV2E, masses_of, maxwell_boltzmann


class Calculator:
    def __init__(self, model_path: str, device: int = 0, lib: Optional[capi.Library] = None, options: Optional[dict] = None, skin: float = 0.0,
                 reuse: bool = False):
        """`options`: library options by name (include/allegro_hip.h: ahip_set_option), e.g. {"precision": "float64"}.  `skin` >= 0 only inflates the ghost
        shell and the neighbor list; the results do not depend on it.  `reuse`: `compute` keeps ghosts and list between calls and rebuilds them only when
        atoms or cell have moved too far for the skin (needs skin > 0; MD, relaxations, variable-cell optimisers)."""
        if skin < 0:
            raise ValueError("skin must be >= 0")
        if reuse and not skin > 0:
            raise ValueError("reuse=True needs skin > 0: the skin is what the atoms may move through before the list is rebuilt")
        self.model = capi.Model(model_path, device, lib)
        for k, v in (options or {}).items():
            self.model.set_option(k, v)
        self.skin = float(skin)
        self.reuse = bool(reuse)
        self.type_names = list(self.model.type_names)

    def close(self) -> None:
        self.model.close()

    def reset(self) -> None:
        """drop the list held by reuse=True: the next `compute` rebuilds it"""
        self.model.cell_reuse_reset()

    def model_types(self, symbols: Sequence[str]) -> np.ndarray:
        """chemical symbols -> model types through the model's type_names; an unknown symbol is a ValueError that names it"""
        index = {s: k for k, s in enumerate(self.type_names)}
        unknown = sorted({str(s) for s in symbols if str(s) not in index})
        if unknown:
            raise ValueError(f"symbol(s) {', '.join(unknown)} not among the model's types {self.type_names}")
        return np.array([index[str(s)] for s in symbols], dtype=np.int32)

    def compute(self, cell, positions, symbols: Sequence[str], pbc: Sequence[bool] = (True, True, True)) -> dict:
        """One evaluation.  `cell`: 3x3, rows are lattice vectors (any orientation); `positions` [n][3], wrapped or not; `pbc`: periodic axes.

        Returns a dict: energy; forces [n][3]; atomic_energy [n]; virial [6] (xx, yy, zz, xy, xz, yz in LAMMPS order and sign); stress [3][3] =
        -virial matrix / volume = (1 / V) dE / d(strain), None unless all three axes are periodic; info: path (kernel family and arithmetic), nghost,
        nedges, row_atom (the atom index of every row -- atoms, then ghost images -- the edge accessors of the model refer to), and with reuse=True
        rebuilt (whether this call built ghosts and list).

        By default nothing is kept between calls: every call wraps, builds the ghost images and the neighbor list again, even for positions that barely moved.
        With reuse=True the model holds them (ahip_compute_cell_reuse): a call refreshes the rows on the device and rebuilds only when the largest
        displacement U since the hold and the change of the lattice vectors fail 2 U + sum_d M_d |a_d - a0_d| <= skin (include/allegro_hip.h states the
        criterion and why it is sufficient).  The cell may change between calls; a change of the species, the atom count, pbc, or any other call on the
        model that installs a list (compute_many among them) makes the next call rebuild.  The results are those of the default path."""
        cell = np.asarray(cell, dtype=np.float64)
        pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        if len(symbols) != len(pos):
            raise ValueError("positions and symbols differ in length")
        pbc = tuple(bool(p) for p in pbc)
        mt = self.model_types(symbols)
        rebuilt = None
        if self.reuse:
            energy, forces, eatom, vir, rebuilt = self.model.compute_cell_reuse(pos, mt, cell, pbc, self.skin)
        else:
            energy, forces, eatom, vir = self.model.compute_cell(pos, mt, cell, pbc, self.skin)
        rows = self.model.last_cell_rows()
        stress = None
        if all(pbc):
            vm = np.array([[vir[0], vir[3], vir[4]], [vir[3], vir[1], vir[5]], [vir[4], vir[5], vir[2]]])
            stress = -vm / abs(np.linalg.det(cell))
        info = dict(path=self.model.last_path, nghost=int(len(rows) - len(pos)), nedges=self.model.nedges(), row_atom=rows)
        if self.reuse:
            info["rebuilt"] = rebuilt
        return dict(energy=energy, forces=forces, atomic_energy=eatom, virial=vir, stress=stress, info=info)

    def relax(self, cell, positions, symbols: Sequence[str], pbc: Sequence[bool] = (True, True, True), fmax: float = 0.05, max_steps: int = 500, fixed=None,
              check_every: int = 4, variable_cell: bool = False, smax: Optional[float] = None, pressure: float = 0.0, strain_mask=None,
              hydrostatic: bool = False, cell_factor: Optional[float] = None, **fire) -> dict:
        """Relaxes the positions at fixed cell: FIRE with the optimiser's state on the device, one library call (ahip_relax_cell; include/allegro_hip.h states
        the algorithm).  Converged when the largest force on a free atom is <= `fmax` (eV/A), or stopped after `max_steps` moves.  `fixed`: a boolean mask of
        atoms that do not move.  `check_every`: moves the host enqueues between two looks at the state.  `fire`: the other fields of ahip_relax_params
        (dt_start, dt_max, max_step, n_min, f_inc, f_dec, alpha_start, f_alpha).

        Returns the dict of `compute` at the relaxed positions plus positions [n][3] (never wrapped: an atom that left the cell keeps its continuous
        coordinate); info gains steps, converged, fmax (the largest force on a free atom), evaluations and rebuilds.  Needs a calculator with skin > 0: the
        ghosts and the neighbor list are held while the atoms move, as with reuse=True.  A later `compute` of a reuse=True calculator goes on from that hold.

        `variable_cell=True` relaxes the cell with the positions (ahip_relax_vcell, all axes periodic): converged when also the largest component of
        stress + pressure is <= `smax` (eV/A^3; the library's default when None).  `pressure`: the external pressure (eV/A^3).  `strain_mask`: six flags (xx,
        yy, zz, xy, xz, yz), False = that strain component is not followed -- the way to relax a slab.  `hydrostatic`: only the volume changes.
        `cell_factor`: the weight of the strain rows among the generalised coordinates (None: the number of atoms).  The result gains cell [3][3], positions
        and stress are those in that cell, and info gains smax.  A model without an equilibrium volume needs a pressure."""
        if not self.skin > 0:
            raise ValueError("relax needs a calculator with skin > 0: the skin is what the atoms may move through before the neighbor list is rebuilt")
        cell = np.asarray(cell, dtype=np.float64)
        pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        if len(symbols) != len(pos):
            raise ValueError("positions and symbols differ in length")
        pbc = tuple(bool(p) for p in pbc)
        mt = self.model_types(symbols)
        if variable_cell:
            par = dict(fire, pressure=pressure, hydrostatic=int(bool(hydrostatic)))
            if smax is not None:
                par["smax"] = smax
            if strain_mask is not None:
                par["mask"] = strain_mask
            if cell_factor is not None:
                par["cell_factor"] = cell_factor
            x, energy, forces, eatom, vir, rinfo, cell = self.model.relax_vcell(pos, mt, cell, pbc, self.skin, fixed=fixed, fmax=fmax, max_steps=max_steps,
                                                                                check_every=check_every, **par)
        else:
            if smax is not None or pressure != 0.0 or strain_mask is not None or hydrostatic or cell_factor is not None:
                raise ValueError("smax, pressure, strain_mask, hydrostatic and cell_factor belong to variable_cell=True")
            x, energy, forces, eatom, vir, rinfo = self.model.relax_cell(pos, mt, cell, pbc, self.skin, fixed=fixed, fmax=fmax, max_steps=max_steps,
                                                                         check_every=check_every, **fire)
        rows = self.model.last_cell_rows()
        stress = None
        if all(pbc):
            vm = np.array([[vir[0], vir[3], vir[4]], [vir[3], vir[1], vir[5]], [vir[4], vir[5], vir[2]]])
            stress = -vm / abs(np.linalg.det(cell))
        info = dict(path=self.model.last_path, nghost=int(len(rows) - len(pos)), nedges=self.model.nedges(), row_atom=rows, **rinfo)
        out = dict(energy=energy, forces=forces, atomic_energy=eatom, virial=vir, stress=stress, positions=x, info=info)
        if variable_cell:
            out["cell"] = cell
        return out

    def md(self, cell, positions, symbols: Sequence[str], pbc: Sequence[bool] = (True, True, True), steps: int = 100, dt: float = 0.001, velocities=None,
           temperature: Optional[float] = None, friction: float = 0.0, seed: int = 0, step0: int = 0, masses: Optional[dict] = None, fixed=None,
           sample_every: int = 1, frame_every: int = 0, check_every: int = 4, pressure: Optional[float] = None, compressibility: Optional[float] = None,
           tau_p: Optional[float] = None) -> dict:
        """Molecular dynamics with the integrator's state on the device, one library call (ahip_md_cell; include/allegro_hip.h states the algorithm): `steps`
        steps of `dt`, NVE (velocity Verlet) when `friction` is 0, else Langevin dynamics by BAOAB at `temperature` with friction `friction`.  Metal units: A, eV,
        ps, amu, K, 1 / ps.  `velocities` [n][3] in A / ps; None draws Maxwell-Boltzmann velocities at `temperature` with zero total momentum from `seed`.
        `seed` also keys the thermostat's noise, which depends only on (seed, atom, step0 + step): a trajectory cut into calls, each started from the positions
        and velocities the last returned with `step0` advanced by its steps, is the trajectory of one call.  `masses`: symbol -> amu over the standard atomic
        weights of units.py; a symbol in neither is a ValueError.  `fixed`: a boolean mask of atoms that keep their position, have velocity 0 and are left out
        of the kinetic energy.  `sample_every` / `frame_every`: a thermo row / a frame of positions every so many steps (0: no frames), step 0 included.
        `check_every`: steps the host enqueues between two looks at the state.

        Returns the dict of `compute` at the final positions plus positions (never wrapped) and velocities [n][3]; thermo: a dict of arrays step, pe, ke,
        temperature = 2 ke / (3 N_free kB) and virial [.][6]; frames [.][n][3] or None; info gains steps, evaluations and rebuilds.  Needs a calculator with
        skin > 0, like `relax`; a later `compute` of a reuse=True calculator goes on from the hold of the run.

        `pressure` (eV/A^3) makes it MD at constant pressure (ahip_npt_cell, all axes periodic): an isotropic stochastic cell rescaling around the same
        integrator, with `compressibility` (A^3/eV; 1.6 is a solid of 100 GPa bulk modulus) and the relaxation time `tau_p` (ps), both required.  The barostat's
        noise is that of `temperature`: None or 0 gives the deterministic (Berendsen-limit) barostat; `friction` 0 keeps the particles on velocity Verlet.  The
        result gains cell [3][3] and frame_cells [.][3][3] (None without frames), thermo gains volume and pressure, positions, velocities and stress are those
        in the returned cell, and a fixed atom follows the cell affinely.  A continuation carries the cell over with positions, velocities and `step0`."""
        if not self.skin > 0:
            raise ValueError("md needs a calculator with skin > 0: the skin is what the atoms may move through before the neighbor list is rebuilt")
        if pressure is None:
            if compressibility is not None or tau_p is not None:
                raise ValueError("compressibility and tau_p belong to a run with a pressure")
        else:
            if not all(bool(p) for p in pbc):
                raise ValueError("md at a pressure needs all three axes periodic: the cell rescaling is isotropic")
            if compressibility is None or tau_p is None:
                raise ValueError("md at a pressure needs compressibility and tau_p")
        cell = np.asarray(cell, dtype=np.float64)
        pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        if len(symbols) != len(pos):
            raise ValueError("positions and symbols differ in length")
        pbc = tuple(bool(p) for p in pbc)
        mt = self.model_types(symbols)
        mass = masses_of(symbols, masses)
        if friction > 0 and temperature is None:
            raise ValueError("friction > 0 needs a temperature: the bath's")
        if velocities is None:
            if temperature is None:
                raise ValueError("give velocities, or a temperature to draw them at")
            velocities = maxwell_boltzmann(len(pos), mass, float(temperature), int(seed)) if len(pos) else np.zeros((0, 3))
        vel = np.asarray(velocities, dtype=np.float64).reshape(-1, 3)
        if len(vel) != len(pos):
            raise ValueError("positions and velocities differ in length")
        par = dict(nsteps=int(steps), dt=float(dt), gamma=float(friction), kT=KB * float(temperature or 0.0), seed=int(seed), step0=int(step0), ftm2v=FTM2V,
                   mvv2e=MVV2E, sample_every=int(sample_every), frame_every=int(frame_every), check_every=int(check_every))
        if pressure is None:
            x, v, energy, forces, eatom, vir, th, frames, minfo = self.model.md_cell(pos, vel, mt, mass, cell, pbc, self.skin, fixed=fixed, **par)
        else:
            x, v, energy, forces, eatom, vir, th, frames, minfo, cell, frame_cells = self.model.npt_cell(
                pos, vel, mt, mass, cell, pbc, self.skin, fixed=fixed, pressure=float(pressure), compressibility=float(compressibility), tau_p=float(tau_p), **par)
        nfree = len(pos) - (int(np.count_nonzero(np.asarray(fixed).astype(bool))) if fixed is not None else 0)
        thermo = dict(step=int(step0) + int(sample_every) * np.arange(len(th)), pe=th[:, 0].copy(), ke=th[:, 1].copy(),
                      temperature=2.0 * th[:, 1] / (3.0 * max(nfree, 1) * KB), virial=th[:, 2:8].copy())
        if pressure is not None:
            thermo.update(volume=th[:, 8].copy(), pressure=th[:, 9].copy())
        rows = self.model.last_cell_rows() if len(pos) else np.zeros(0, dtype=np.int64)
        stress = None
        if all(pbc):
            vm = np.array([[vir[0], vir[3], vir[4]], [vir[3], vir[1], vir[5]], [vir[4], vir[5], vir[2]]])
            stress = -vm / abs(np.linalg.det(cell))
        info = dict(path=self.model.last_path, nghost=int(len(rows) - len(pos)), nedges=self.model.nedges() if len(pos) else 0, row_atom=rows, **minfo)
        out = dict(energy=energy, forces=forces, atomic_energy=eatom, virial=vir, stress=stress, positions=x, velocities=v, thermo=thermo, frames=frames, info=info)
        if pressure is not None:
            out.update(cell=cell, frame_cells=frame_cells)
        return out

    def compute_many(self, structures: Sequence, max_atoms: int = 1 << 20) -> list:
        """A data set in as few library calls as possible (ahip_compute_cells: one upload, one ghost build, one neighbor list and one evaluation per call,
        where `compute` pays all of them per structure).  `structures`: a sequence of (cell, positions, symbols) or (cell, positions, symbols, pbc), each
        as in `compute`; an empty structure is allowed.

        Returns a list of dicts, one per structure, in order: energy, forces, atomic_energy, virial, stress (None unless all three axes are periodic) and info:
        path, nghost, batch (the index of the library call that evaluated it).  The sequence is cut into consecutive calls of at most `max_atoms` atoms (a single
        larger structure goes alone); a call the library refuses as too uneven for one neighbor grid ("split the batch") is halved and repeated.  An unknown
        symbol is a ValueError that names the structure and the symbol, before any call."""
        if max_atoms < 1:
            raise ValueError("max_atoms must be >= 1")
        items = []
        for k, st in enumerate(structures):
            if len(st) not in (3, 4):
                raise ValueError(f"structure {k}: expected (cell, positions, symbols[, pbc])")
            cell = np.asarray(st[0], dtype=np.float64)
            pos = np.asarray(st[1], dtype=np.float64).reshape(-1, 3)
            if cell.shape != (3, 3):
                raise ValueError(f"structure {k}: cell must be a 3x3 matrix of lattice vectors (rows), got shape {cell.shape}")
            if len(st[2]) != len(pos):
                raise ValueError(f"structure {k}: positions and symbols differ in length")
            pbc = tuple(bool(p) for p in (st[3] if len(st) == 4 else (True, True, True)))
            if len(pbc) != 3:
                raise ValueError(f"structure {k}: pbc must have three entries")
            try:
                mt = self.model_types(st[2])
            except ValueError as e:
                raise ValueError(f"structure {k}: {e}") from None
            items.append((cell, pos, mt, pbc))
        chunks, lo = [], 0
        while lo < len(items):                     # consecutive chunks of at most max_atoms atoms, at least one structure each
            hi, n = lo + 1, len(items[lo][1])
            while hi < len(items) and n + len(items[hi][1]) <= max_atoms:
                n += len(items[hi][1])
                hi += 1
            chunks.append((lo, hi))
            lo = hi
        results, ncall = [None] * len(items), 0
        while chunks:
            lo, hi = chunks.pop(0)
            part = items[lo:hi]
            first = np.concatenate([[0], np.cumsum([len(p[1]) for p in part])]).astype(np.int32)
            x = np.concatenate([p[1] for p in part]) if part else np.zeros((0, 3))
            mt = np.concatenate([p[2] for p in part]) if part else np.zeros(0, np.int32)
            try:
                eng, f, ea, vir = self.model.compute_cells(first, x, mt, np.stack([p[0] for p in part]), np.array([p[3] for p in part]), self.skin)
            except capi.AhipError as e:
                if e.code == capi.AHIP_ERR_ARG and "split the batch" in e.msg and hi - lo > 1:
                    mid = lo + (hi - lo) // 2
                    chunks[:0] = [(lo, mid), (mid, hi)]
                    continue
                raise
            ghosts, path = self.model.last_cells_ghosts(), self.model.last_path
            for k, (cell, pos, _, pbc) in enumerate(part):
                a, b = int(first[k]), int(first[k + 1])
                v = vir[k].copy()
                stress = None
                if all(pbc):
                    vm = np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]])
                    stress = -vm / abs(np.linalg.det(cell))
                results[lo + k] = dict(energy=float(eng[k]), forces=f[a:b].copy(), atomic_energy=ea[a:b].copy(), virial=v, stress=stress,
                                       info=dict(path=path, nghost=int(ghosts[k]), batch=ncall))
            ncall += 1
        return results
