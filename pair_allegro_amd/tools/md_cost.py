"""What Calculator.md (ahip_md_cell: BAOAB with its state on the device) saves over the same BAOAB written in Python over Calculator(reuse=True).compute.

   python pair_allegro_amd/tools/md_cost.py [--steps 200] [--reps 3] [--out FILE]          (GPU box)

The 64-atom Si cell (2 x 2 x 2 diamond cells) and the 10 648-atom Si box (11 x 11 x 11), every coordinate jittered by --sigma A from a fixed seed,
Maxwell-Boltzmann velocities at --temperature, float32 model S (random weights), r_max 5 A, skin --skin, dt --dt, one GPU, one process, one library, one
calculator per route; NVE (gamma = 0) and Langevin (--friction, bath at --temperature).  "python": the algorithm of include/allegro_hip.h in numpy, one
Calculator(reuse=True).compute per step -- an upload, three downloads and two synchronisations per step, the best a caller could do before ahip_md_cell -- with
numpy's own normal deviates for the thermostat (cheaper than the counter-based generator of the library would be in numpy).  "md": Calculator.md at each
--check-every, one thermo row per step, no frames.  Host wall clock around each run (both return host arrays, so the device is idle when they return).  One
warm-up of each, then --reps alternating repetitions; the medians are reported as microseconds per step, with the rebuilds and evaluations of each route and, for
NVE, the largest distance between their end points."""
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


def python_baoab(calc, cell, x0, v0, mass, symbols, steps, dt, gamma, kT, rng):
    """BAOAB as include/allegro_hip.h states it, a thermo row per step; the calculator decides about its list by itself"""
    m = mass[:, None]
    hdtf, c1 = 0.5 * dt * FTM2V, np.exp(-gamma * dt)
    sig = np.sqrt(1.0 - c1 * c1) * np.sqrt(kT / (m * MVV2E))
    x, w, rebuilds, thermo = x0.copy(), v0.copy(), 0, np.zeros((steps + 1, 8))
    out = calc.compute(cell, x, symbols)
    rebuilds += out["info"]["rebuilt"]
    for n in range(steps + 1):
        a = hdtf * out["forces"] / m
        v = w + a if n > 0 else w
        thermo[n, 0], thermo[n, 1], thermo[n, 2:] = out["energy"], 0.5 * MVV2E * float((m * v * v).sum()), out["virial"]
        if n == steps:
            break
        vp = v + a
        xh = x + 0.5 * dt * vp
        w = c1 * vp + sig * rng.normal(size=x.shape) if gamma > 0 else vp
        x = xh + 0.5 * dt * w
        out = calc.compute(cell, x, symbols)
        rebuilds += out["info"]["rebuilt"]
    return x, v, out, thermo, rebuilds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.05, help="jitter of the start per coordinate, A")
    ap.add_argument("--skin", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=0.001, help="ps")
    ap.add_argument("--temperature", type=float, default=300.0, help="K: start velocities and bath")
    ap.add_argument("--friction", type=float, default=5.0, help="1 / ps, the Langevin runs")
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
            py_c, md_c = Calculator(path, lib=lib, skin=a.skin, reuse=True), Calculator(path, lib=lib, skin=a.skin)
            for gamma in (0.0, a.friction):

                def python():
                    py_c.reset()
                    t = time.perf_counter()
                    x, v, out, thermo, rebuilds = python_baoab(py_c, cell, x0, v0, mass, symbols, a.steps, a.dt, gamma, KB * a.temperature, np.random.RandomState(9))
                    return time.perf_counter() - t, x, rebuilds, out["info"]["path"]

                def md(k):
                    t = time.perf_counter()
                    out = md_c.md(cell, x0, symbols, steps=a.steps, dt=a.dt, velocities=v0, temperature=a.temperature, friction=gamma, seed=9, check_every=k)
                    return time.perf_counter() - t, out

                _, xp, py_rebuilds, py_path = python()
                first = {k: md(k)[1] for k in every}
                t_py, t_md = [], {k: [] for k in every}
                for _ in range(a.reps):
                    t_py.append(python()[0])
                    for k in every:
                        t_md[k].append(md(k)[0])
                us = lambda t: 1e6 * float(np.median(t)) / a.steps      # noqa: E731
                res = dict(atoms=n, steps=a.steps, gamma=gamma, dt=a.dt, temperature=a.temperature, sigma=a.sigma, skin=a.skin, path_python=py_path,
                           python_us_per_step=us(t_py), python_rebuilds=py_rebuilds, python_s=[round(t, 6) for t in t_py], md={})
                say(f"{n}-atom Si box, model S float32, r_max {cfg['r_max']} A, skin {a.skin} A, {a.steps} BAOAB steps of {a.dt} ps from {a.temperature} K, gamma {gamma} / ps; "
                    f"paths: python {py_path}, md {first[every[0]]['info']['path']}")
                say(f"  python BAOAB over Calculator(reuse=True).compute : {us(t_py):9.1f} us per step (median of {a.reps}; whole run {', '.join(f'{1e3 * t:.2f}' for t in t_py)} ms); "
                    f"{py_rebuilds} rebuilds")
                for k in every:
                    info = first[k]["info"]
                    dx = float(np.abs(first[k]["positions"] - xp).max())
                    res["md"][str(k)] = dict(us_per_step=us(t_md[k]), ratio=us(t_py) / us(t_md[k]), rebuilds=info["rebuilds"], evaluations=info["evaluations"],
                                             s=[round(t, 6) for t in t_md[k]], end_point_distance=dx if gamma == 0 else None)
                    say(f"  Calculator.md, check_every {k:2d}                     : {us(t_md[k]):9.1f} us per step (median of {a.reps}; whole run "
                        f"{', '.join(f'{1e3 * t:.2f}' for t in t_md[k])} ms); ratio {us(t_py) / us(t_md[k]):.2f}x; {info['rebuilds']} rebuilds, {info['evaluations']} evaluations"
                        + (f"; end point within {dx:.3e} A of the python route's" if gamma == 0 else "; (other noise: the end points are not compared)"))
                results.append(res)
            py_c.close(); md_c.close()
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
