"""What Calculator.relax (ahip_relax_cell: FIRE with its state on the device) saves over the same FIRE written in Python over Calculator(reuse=True).compute.

   python pair_allegro_amd/tools/relax_cost.py [--moves 200] [--reps 3] [--out FILE]          (GPU box)

The 64-atom Si cell (2 x 2 x 2 diamond cells) and the 10 648-atom Si box (11 x 11 x 11), every coordinate jittered by --sigma A from a fixed seed, float32 model S
(random weights: it does not converge, so fmax = 0 and every run makes exactly --moves moves), r_max 5 A, skin --skin, one GPU, one process, one library, one
calculator per route.  "python": the algorithm of include/allegro_hip.h in numpy, one Calculator(reuse=True).compute per move -- an upload, three downloads and
two synchronisations per move, the best a caller could do before ahip_relax_cell.  "relax": Calculator.relax at each --check-every.  Host wall clock around each
run (both return host arrays, so the device is idle when they return).  One warm-up of each, then --reps alternating repetitions; the medians are reported as
microseconds per move, with the moves, rebuilds and evaluations of each route and the largest distance between their end points."""
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


def python_fire(calc, cell, x0, symbols, moves):
    """FIRE as include/allegro_hip.h states it, fmax = 0; the calculator decides about its list by itself"""
    x, v = x0.copy(), np.zeros_like(x0)
    dt, alpha, npos, rebuilds = FIRE["dt_start"], FIRE["alpha_start"], 0, 0
    out = calc.compute(cell, x, symbols)
    rebuilds += out["info"]["rebuilt"]
    for _ in range(moves):
        F = out["forces"]
        vf, ff, vv = float(np.vdot(v, F)), float(np.vdot(F, F)), float(np.vdot(v, v))
        if vf > 0:
            c1, c2 = 1.0 - alpha, alpha * np.sqrt(vv / ff)
            if npos > FIRE["n_min"]:
                dt = min(dt * FIRE["f_inc"], FIRE["dt_max"])
                alpha *= FIRE["f_alpha"]
            npos += 1
        else:
            c1 = c2 = 0.0
            alpha, dt, npos = FIRE["alpha_start"], dt * FIRE["f_dec"], 0
        v = c1 * v + (c2 + dt) * F
        dr = dt * v
        norm = float(np.sqrt(np.vdot(dr, dr)))
        x = x + min(1.0, FIRE["max_step"] / norm) * dr
        out = calc.compute(cell, x, symbols)
        rebuilds += out["info"]["rebuilt"]
    return x, out, rebuilds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.05, help="jitter of the start per coordinate, A")
    ap.add_argument("--skin", type=float, default=1.0)
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

            def python():
                py_c.reset()
                t = time.perf_counter()
                x, out, rebuilds = python_fire(py_c, cell, x0, symbols, a.moves)
                return time.perf_counter() - t, x, rebuilds, out["info"]["path"]

            def relax(k):
                t = time.perf_counter()
                out = rx_c.relax(cell, x0, symbols, fmax=0.0, max_steps=a.moves, check_every=k, **FIRE)
                return time.perf_counter() - t, out

            _, xp, py_rebuilds, py_path = python()
            first = {k: relax(k)[1] for k in every}
            t_py, t_rx = [], {k: [] for k in every}
            for _ in range(a.reps):
                t_py.append(python()[0])
                for k in every:
                    t_rx[k].append(relax(k)[0])
            py_c.close(); rx_c.close()
            us = lambda t: 1e6 * float(np.median(t)) / a.moves
            res = dict(atoms=n, moves=a.moves, sigma=a.sigma, skin=a.skin, path_python=py_path, python_us_per_move=us(t_py), python_rebuilds=py_rebuilds,
                       python_s=[round(t, 6) for t in t_py], relax={})
            say(f"{n}-atom Si box, model S float32, r_max {cfg['r_max']} A, skin {a.skin} A, {a.moves} FIRE moves from a jitter of {a.sigma} A; paths: python "
                f"{py_path}, relax {first[every[0]]['info']['path']}")
            say(f"  python FIRE over Calculator(reuse=True).compute : {us(t_py):9.1f} us per move (median of {a.reps}; whole run {', '.join(f'{1e3 * t:.2f}' for t in t_py)} ms); "
                f"{py_rebuilds} rebuilds")
            for k in every:
                info = first[k]["info"]
                dx = float(np.abs(first[k]["positions"] - xp).max())
                res["relax"][str(k)] = dict(us_per_move=us(t_rx[k]), ratio=us(t_py) / us(t_rx[k]), steps=info["steps"], rebuilds=info["rebuilds"],
                                            evaluations=info["evaluations"], s=[round(t, 6) for t in t_rx[k]], end_point_distance=dx)
                say(f"  Calculator.relax, check_every {k:2d}                  : {us(t_rx[k]):9.1f} us per move (median of {a.reps}; whole run "
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
