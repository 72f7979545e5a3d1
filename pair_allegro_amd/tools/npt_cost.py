"""What Calculator.md(pressure=...) (ahip_npt_cell: BAOAB inside a stochastic cell rescaling, state and cell on the device) saves over the same algorithm written
in Python over Calculator(reuse=True).compute.

   python pair_allegro_amd/tools/npt_cost.py [--steps 200] [--reps 3] [--out FILE]          (GPU box)

The 64-atom Si cell (2 x 2 x 2 diamond cells) and the 10 648-atom Si box (11 x 11 x 11), every coordinate jittered by --sigma A from a fixed seed,
Maxwell-Boltzmann velocities at --temperature, float32 model S (random weights), r_max 5 A, skin --skin, dt --dt, one GPU, one process, one library, one
calculator per route.  The random-weight model has no equilibrium volume, so P0 is the virial pressure of the start, as in tools/vcell_relax_cost.py;
--compressibility and --tau-p are the barostat's.  Two variants: the deterministic barostat over velocity Verlet (gamma = 0, kT = 0) and the stochastic one over
Langevin BAOAB (--friction, bath at --temperature).  "python": the algorithm of include/allegro_hip.h in numpy, one Calculator(reuse=True).compute per step -- an
upload, three downloads and two synchronisations per step -- with numpy's own normal deviates.  "npt": Calculator.md at each --check-every, one thermo row per
step, no frames.  Host wall clock around each run (both return host arrays, so the device is idle when they return).  One warm-up of each, then --reps alternating
repetitions; the medians are reported as microseconds per step, with the rebuilds and evaluations of each route, V / V0 at the end and, for the deterministic
variant, the largest distance between the end points."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "4095")

from pair_allegro_amd import capi, lmp_like, model_file  # noqa: E402
from pair_allegro_amd.calculator import Calculator  # noqa: E402
from pair_allegro_amd.units import FTM2V, KB, MVV2E, masses_of, maxwell_boltzmann  # noqa: E402


def pressure_of(out, cell, mass, v):
    ke = 0.5 * MVV2E * float((mass[:, None] * v * v).sum())
    return (2.0 * ke + float(out["virial"][:3].sum())) / (3.0 * abs(np.linalg.det(cell)))


def python_npt(calc, cell0, x0, v0, mass, symbols, steps, dt, gamma, kT, p0, beta, tau_p, rng):
    """the algorithm of include/allegro_hip.h, a thermo row per step; the calculator decides about its list by itself"""
    m = mass[:, None]
    hdtf, c1 = 0.5 * dt * FTM2V, np.exp(-gamma * dt)
    sig = np.sqrt(1.0 - c1 * c1) * np.sqrt(kT / (m * MVV2E))
    noise = np.sqrt(2.0 * kT * beta * dt / tau_p)
    x, w, A, rebuilds, thermo = x0.copy(), v0.copy(), cell0.copy(), 0, np.zeros((steps + 1, 10))
    out = calc.compute(A, x, symbols)
    rebuilds += out["info"]["rebuilt"]
    for n in range(steps + 1):
        a = hdtf * out["forces"] / m
        v = w + a if n > 0 else w
        V = abs(np.linalg.det(A))
        ke = 0.5 * MVV2E * float((m * v * v).sum())
        P = (2.0 * ke + float(out["virial"][:3].sum())) / (3.0 * V)
        thermo[n, 0], thermo[n, 1], thermo[n, 2:8], thermo[n, 8], thermo[n, 9] = out["energy"], ke, out["virial"], V, P
        if n == steps:
            break
        de = -(beta / tau_p) * (p0 - P) * dt + (noise / np.sqrt(V) * rng.normal() if noise > 0 else 0.0)
        mu = np.exp(de / 3.0)
        vp = v + a
        xh = x + 0.5 * dt * vp
        wd = c1 * vp + sig * rng.normal(size=x.shape) if gamma > 0 else vp
        x, w, A = mu * (xh + 0.5 * dt * wd), wd / mu, mu * A
        out = calc.compute(A, x, symbols)
        rebuilds += out["info"]["rebuilt"]
    return x, v, A, out, thermo, rebuilds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.05, help="jitter of the start per coordinate, A")
    ap.add_argument("--skin", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=0.001, help="ps")
    ap.add_argument("--temperature", type=float, default=300.0, help="K: start velocities and bath")
    ap.add_argument("--friction", type=float, default=5.0, help="1 / ps, the stochastic runs")
    ap.add_argument("--compressibility", type=float, default=1.6, help="A^3 / eV")
    ap.add_argument("--tau-p", type=float, default=0.1, help="ps")
    ap.add_argument("--check-every", default="1,4,16", help="values of check_every, comma-separated")
    ap.add_argument("--cells", default="2,11", help="diamond cells per edge of the boxes, comma-separated")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    cfg = model_file.model_S()
    every = [int(v) for v in a.check_every.split(",")]
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.ahip")
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
        lib = capi.Library()
        for ncell in [int(v) for v in a.cells.split(",")]:
            cell, pos, _ = lmp_like.diamond_si(ncell)
            cell = np.asarray(cell, dtype=np.float64)
            n = len(pos)
            x0 = pos + np.random.RandomState(7).normal(scale=a.sigma, size=pos.shape)
            symbols = [cfg["type_names"][0]] * n
            mass = masses_of(symbols)
            v0 = maxwell_boltzmann(n, mass, a.temperature, 8)
            py_c, npt_c = Calculator(path, lib=lib, skin=a.skin, reuse=True), Calculator(path, lib=lib, skin=a.skin)
            p0 = pressure_of(py_c.compute(cell, x0, symbols), cell, mass, v0)
            for name, gamma, temperature in (("deterministic barostat, velocity Verlet", 0.0, 0.0), ("stochastic barostat, Langevin", a.friction, a.temperature)):

                def python():
                    py_c.reset()
                    t = time.perf_counter()
                    x, v, A, out, thermo, rebuilds = python_npt(py_c, cell, x0, v0, mass, symbols, a.steps, a.dt, gamma, KB * temperature, p0, a.compressibility, a.tau_p,
                                                                np.random.RandomState(9))
                    return time.perf_counter() - t, x, A, rebuilds, out["info"]["path"]

                def npt(k):
                    t = time.perf_counter()
                    out = npt_c.md(cell, x0, symbols, steps=a.steps, dt=a.dt, velocities=v0, temperature=temperature, friction=gamma, seed=9, check_every=k, pressure=p0,
                                   compressibility=a.compressibility, tau_p=a.tau_p)
                    return time.perf_counter() - t, out

                _, xp, Ap, py_rebuilds, py_path = python()
                first = {k: npt(k)[1] for k in every}
                t_py, t_npt = [], {k: [] for k in every}
                for _ in range(a.reps):
                    t_py.append(python()[0])
                    for k in every:
                        t_npt[k].append(npt(k)[0])
                us = lambda t: 1e6 * float(np.median(t)) / a.steps      # noqa: E731
                V0 = abs(np.linalg.det(cell))
                res = dict(atoms=n, steps=a.steps, variant=name, gamma=gamma, temperature=temperature, dt=a.dt, sigma=a.sigma, skin=a.skin, p0=p0,
                           compressibility=a.compressibility, tau_p=a.tau_p, path_python=py_path, python_us_per_step=us(t_py), python_rebuilds=py_rebuilds,
                           python_volume_ratio=abs(np.linalg.det(Ap)) / V0, python_s=[round(t, 6) for t in t_py], npt={})
                say(f"{n}-atom Si box, model S float32, r_max {cfg['r_max']} A, skin {a.skin} A, {a.steps} steps of {a.dt} ps from {a.temperature} K; {name} (gamma {gamma} / ps, "
                    f"bath {temperature} K); P0 {p0:.5f} eV/A^3 (the start's), beta_T {a.compressibility} A^3/eV, tau_p {a.tau_p} ps; paths: python {py_path}, npt "
                    f"{first[every[0]]['info']['path']}")
                say(f"  python loop over Calculator(reuse=True).compute  : {us(t_py):9.1f} us per step (median of {a.reps}; whole run {', '.join(f'{1e3 * t:.2f}' for t in t_py)} ms); "
                    f"{py_rebuilds} rebuilds; V / V0 at the end {res['python_volume_ratio']:.5f}")
                for k in every:
                    info = first[k]["info"]
                    dx = float(max(np.abs(first[k]["positions"] - xp).max(), np.abs(first[k]["cell"] - Ap).max()))
                    ratio = abs(np.linalg.det(first[k]["cell"])) / V0
                    res["npt"][str(k)] = dict(us_per_step=us(t_npt[k]), ratio=us(t_py) / us(t_npt[k]), rebuilds=info["rebuilds"], evaluations=info["evaluations"],
                                              s=[round(t, 6) for t in t_npt[k]], volume_ratio=ratio, end_point_distance=dx if gamma == 0 else None)
                    say(f"  Calculator.md(pressure=...), check_every {k:2d}       : {us(t_npt[k]):9.1f} us per step (median of {a.reps}; whole run "
                        f"{', '.join(f'{1e3 * t:.2f}' for t in t_npt[k])} ms); ratio {us(t_py) / us(t_npt[k]):.2f}x; {info['rebuilds']} rebuilds, {info['evaluations']} evaluations; "
                        f"V / V0 at the end {ratio:.5f}" + (f"; end point (positions and cell) within {dx:.3e} A of the python route's" if gamma == 0 else
                                                           "; (other noise: the end points are not compared)"))
                results.append(res)
            py_c.close(); npt_c.close()
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
