"""Metal units (A, eV, ps, g/mol, K) as LAMMPS defines them, the Maxwell-Boltzmann draw and a small table of standard atomic weights: numpy only, so that
the LAMMPS-free route (calculator.py) needs no torch.  md.py re-exports the constants and `maxwell_boltzmann`."""
from typing import Optional, Sequence

import numpy as np

FTM2V = 1.0 / 1.0364269e-4          # metal units: (eV/A)/(g/mol) -> A/ps^2
MVV2E = 1.0364269e-4
KB = 8.617343e-5

# standard atomic weights (IUPAC 2021, abridged to what the digits below show), g/mol
ATOMIC_WEIGHTS = {
    "H": 1.008, "He": 4.002602, "Li": 6.94, "Be": 9.0121831, "B": 10.81, "C": 12.011, "N": 14.007, "O": 15.999, "F": 18.998403, "Ne": 20.1797,
    "Na": 22.98976928, "Mg": 24.305, "Al": 26.9815384, "Si": 28.085, "P": 30.973762, "S": 32.06, "Cl": 35.45, "Ar": 39.95, "K": 39.0983, "Ca": 40.078,
    "Sc": 44.955907, "Ti": 47.867, "V": 50.9415, "Cr": 51.9961, "Mn": 54.938043, "Fe": 55.845, "Co": 58.933194, "Ni": 58.6934, "Cu": 63.546, "Zn": 65.38,
    "Ga": 69.723, "Ge": 72.630, "As": 74.921595, "Se": 78.971, "Br": 79.904, "Kr": 83.798, "Rb": 85.4678, "Sr": 87.62, "Y": 88.905838, "Zr": 91.224,
    "Nb": 92.90637, "Mo": 95.95, "Ru": 101.07, "Rh": 102.90549, "Pd": 106.42, "Ag": 107.8682, "Cd": 112.414, "In": 114.818, "Sn": 118.710, "Sb": 121.760,
    "Te": 127.60, "I": 126.90447, "Xe": 131.293, "Cs": 132.90545196, "Ba": 137.327, "La": 138.90547, "Hf": 178.486, "Ta": 180.94788, "W": 183.84,
    "Re": 186.207, "Os": 190.23, "Ir": 192.217, "Pt": 195.084, "Au": 196.966570, "Hg": 200.592, "Tl": 204.38, "Pb": 207.2, "Bi": 208.98040,
}


def masses_of(symbols: Sequence[str], masses: Optional[dict] = None) -> np.ndarray:
    """per-atom masses [g/mol]: `masses` (symbol -> mass) over ATOMIC_WEIGHTS; a symbol in neither is a ValueError that names it"""
    table = dict(ATOMIC_WEIGHTS, **{str(k): float(v) for k, v in (masses or {}).items()})
    unknown = sorted({str(s) for s in symbols if str(s) not in table})
    if unknown:
        raise ValueError(f"no mass for symbol(s) {', '.join(unknown)}: pass masses={{symbol: amu}}")
    return np.array([table[str(s)] for s in symbols], dtype=np.float64)


def maxwell_boltzmann(n: int, mass: np.ndarray, temperature: float, seed: int) -> np.ndarray:
    rng = np.random.RandomState(seed)
    sigma = np.sqrt(KB * temperature / (mass * MVV2E))
    v = rng.normal(size=(n, 3)) * sigma[:, None]
    v -= (v * mass[:, None]).sum(0) / mass.sum()
    return v
