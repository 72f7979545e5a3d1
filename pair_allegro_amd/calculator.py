"""Energy, forces and stress of one structure without LAMMPS: "cell, positions, species" in, one call into the library
(ahip_compute_cell: wrap, ghost images, neighbor list and model evaluation all on the device) out.

    from pair_allegro_amd.calculator import Calculator
    calc = Calculator("model.nequip.pth")
    out = calc.compute(cell, positions, symbols)          # out["energy"], out["forces"], out["stress"]

Any cell works: triclinic, thinner than the cutoff (several images per direction), open axes.  No ASE import: an ASE calculator is three lines
around `compute(atoms.cell.array, atoms.positions, atoms.get_chemical_symbols(), atoms.pbc)`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import capi


class Calculator:
    def __init__(self, model_path: str, device: int = 0, lib: Optional[capi.Library] = None, options: Optional[dict] = None, skin: float = 0.0):
        """`options`: library options by name (include/allegro_hip.h: ahip_set_option), e.g. {"precision": "float64"}.  `skin` >= 0 only inflates the ghost
        shell and the neighbor list; the results do not depend on it."""
        if skin < 0:
            raise ValueError("skin must be >= 0")
        self.model = capi.Model(model_path, device, lib)
        for k, v in (options or {}).items():
            self.model.set_option(k, v)
        self.skin = float(skin)
        self.type_names = list(self.model.type_names)

    def close(self) -> None:
        self.model.close()

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
        nedges, row_atom (the atom index of every row -- atoms, then ghost images -- the edge accessors of the model refer to).

        Nothing is kept between calls: every call wraps, builds the ghost images and the neighbor list again, even for positions that barely moved.
        Reusing lists across calls (a skin with a displacement check, as the MD driver does) is left to a later change."""
        cell = np.asarray(cell, dtype=np.float64)
        pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        if len(symbols) != len(pos):
            raise ValueError("positions and symbols differ in length")
        pbc = tuple(bool(p) for p in pbc)
        mt = self.model_types(symbols)
        energy, forces, eatom, vir = self.model.compute_cell(pos, mt, cell, pbc, self.skin)
        rows = self.model.last_cell_rows()
        stress = None
        if all(pbc):
            vm = np.array([[vir[0], vir[3], vir[4]], [vir[3], vir[1], vir[5]], [vir[4], vir[5], vir[2]]])
            stress = -vm / abs(np.linalg.det(cell))
        info = dict(path=self.model.last_path, nghost=int(len(rows) - len(pos)), nedges=self.model.nedges(), row_atom=rows)
        return dict(energy=energy, forces=forces, atomic_energy=eatom, virial=vir, stress=stress, info=info)
