"""What Calculator.relax(variable_cell=True) (ahip_relax_vcell: FIRE over atoms and cell with its state on the device) saves over the same algorithm written in
Python over Calculator(reuse=True).compute.

   python pair_allegro_amd/tools/vcell_relax_cost.py [--moves 200] [--reps 3] [--out FILE]          (GPU box)

The 64-atom Si cell (2 x 2 x 2 diamond cells) and the 10 648-atom Si box (11 x 11 x 11), every coordinate jittered by --sigma A from a fixed seed, float32 model S
(random weights: it does not converge, so fmax = smax = 0 and every run makes exactly --moves moves), r_max 5 A, skin --skin, one GPU, one process, one library,
one calculator per route.  A random-weight model has no equilibrium volume, so the external pressure is the virial pressure of the start, tr W / 3 V (or
--pressure): the cell then breathes instead of running away.  "python": the algorithm of include/allegro_hip.h in numpy, one Calculator(reuse=True).compute per
move -- an upload, three downloads and two synchronisations per move, the best a caller could do before ahip_relax_vcell; the calculator decides about its
list by itself, with the criterion the library applies on the device.  "relax": Calculator.relax(variable_cell=True) at each --check-every.  Host wall clock
around each run.  One warm-up of each, then --reps alternating repetitions; the medians are reported as microseconds per move, with the moves, rebuilds and
evaluations of each route, det D at the end and the largest distance between their end points (positions and cell entries)."""
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

FIRE = dict(dt_start=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)


def python_vcell_fire(calc, cell0, x0, symbols, moves, pressure):
    """the algorithm of include/allegro_hip.h with c = natoms, fmax = smax = 0, all strain components; the last configuration is evaluated, as the library does"""
    n = len(x0)
    c = float(n)
    q, v = x0.copy(), np.zeros_like(x0)
    D, vD = np.eye(3), np.zeros((3, 3))
    dt, alpha, npos, rebuilds = FIRE["dt_start"], FIRE["alpha_start"], 0, 0
    out = calc.compute(cell0, q, symbols)
    rebuilds += out["info"]["rebuilt"]
    for _ in range(moves):
        A = cell0 @ D.T
        vir = out["virial"]
        W = np.array([[vir[0], vir[3], vir[4]], [vir[3], vir[1], vir[5]], [vir[4], vir[5], vir[2]]]) - pressure * abs(np.linalg.det(A)) * np.eye(3)
        G, GD = out["forces"] @ D, W @ np.linalg.inv(D).T / c
        vf = float(np.vdot(v, G) + np.vdot(vD, GD))
        ff = float(np.vdot(G, G) + np.vdot(GD, GD))
        vv = float(np.vdot(v, v) + np.vdot(vD, vD))
        if vf > 0:
            c1, c2 = 1.0 - alpha, alpha * np.sqrt(vv / ff)
            if npos > FIRE["n_min"]:
                dt = min(dt * FIRE["f_inc"], FIRE["dt_max"])
                alpha *= FIRE["f_alpha"]
            npos += 1
        else:
            c1 = c2 = 0.0
            alpha, dt, npos = FIRE["alpha_start"], dt * FIRE["f_dec"], 0
        v, vD = c1 * v + (c2 + dt) * G, c1 * vD + (c2 + dt) * GD
        norm = dt * float(np.sqrt(np.vdot(v, v) + np.vdot(vD, vD)))
        s = min(1.0, FIRE["max_step"] / norm)
        q, D = q + s * dt * v, D + s * dt * vD / c
        out = calc.compute(cell0 @ D.T, q @ D.T, symbols)
        rebuilds += out["info"]["rebuilt"]
    return q @ D.T, cell0 @ D.T, out, rebuilds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.05, help="jitter of the start per coordinate, A")
    ap.add_argument("--skin", type=float, default=1.0)
    ap.add_argument("--pressure", type=float, default=None, help="external pressure, eV/A^3 (default: the virial pressure of the start)")
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
            py_c, rx_c = Calculator(path, lib=lib, skin=a.skin, reuse=True), Calculator(path, lib=lib, skin=a.skin)
            pressure = a.pressure
            if pressure is None:
                pressure = float(np.sum(py_c.compute(cell, x0, symbols)["virial"][:3]) / 3.0 / abs(np.linalg.det(cell)))

            def python():
                py_c.reset()
                t = time.perf_counter()
                x, A, out, rebuilds = python_vcell_fire(py_c, cell, x0, symbols, a.moves, pressure)
                return time.perf_counter() - t, x, A, rebuilds, out["info"]["path"]

            def relax(k):
                t = time.perf_counter()
                out = rx_c.relax(cell, x0, symbols, fmax=0.0, max_steps=a.moves, check_every=k, variable_cell=True, smax=0.0, pressure=pressure, **FIRE)
                return time.perf_counter() - t, out

            _, xp, Ap, py_rebuilds, py_path = python()
            first = {k: relax(k)[1] for k in every}
            t_py, t_rx = [], {k: [] for k in every}
            for _ in range(a.reps):
                t_py.append(python()[0])
                for k in every:
                    t_rx[k].append(relax(k)[0])
            py_c.close(); rx_c.close()
            us = lambda t: 1e6 * float(np.median(t)) / a.moves
            det = float(np.linalg.det(Ap) / np.linalg.det(cell))
            res = dict(atoms=n, moves=a.moves, sigma=a.sigma, skin=a.skin, pressure=pressure, path_python=py_path, python_us_per_move=us(t_py),
                       python_rebuilds=py_rebuilds, python_det_D=det, python_s=[round(t, 6) for t in t_py], relax={})
            say(f"{n}-atom Si box, model S float32, r_max {cfg['r_max']} A, skin {a.skin} A, {a.moves} variable-cell FIRE moves from a jitter of {a.sigma} A at "
                f"pressure {pressure:.5f} eV/A^3; paths: python {py_path}, relax {first[every[0]]['info']['path']}")
            say(f"  python algorithm over Calculator(reuse=True).compute : {us(t_py):9.1f} us per move (median of {a.reps}; whole run "
                f"{', '.join(f'{1e3 * t:.2f}' for t in t_py)} ms); {py_rebuilds} rebuilds; det D at the end {det:.5f}")
            for k in every:
                info = first[k]["info"]
                dx = max(float(np.abs(first[k]["positions"] - xp).max()), float(np.abs(first[k]["cell"] - Ap).max()))
                res["relax"][str(k)] = dict(us_per_move=us(t_rx[k]), ratio=us(t_py) / us(t_rx[k]), steps=info["steps"], rebuilds=info["rebuilds"],
                                            evaluations=info["evaluations"], s=[round(t, 6) for t in t_rx[k]], end_point_distance=dx)
                say(f"  Calculator.relax(variable_cell=True), check_every {k:2d}   : {us(t_rx[k]):9.1f} us per move (median of {a.reps}; whole run "
                    f"{', '.join(f'{1e3 * t:.2f}' for t in t_rx[k])} ms); ratio {us(t_py) / us(t_rx[k]):.2f}x; {info['steps']} moves, {info['rebuilds']} rebuilds, "
                    f"{info['evaluations']} evaluations; end point within {dx:.3e} A of the python route's")
            results.append(res)
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
