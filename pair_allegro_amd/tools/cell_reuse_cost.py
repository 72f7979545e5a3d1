"""What ahip_compute_cell_reuse saves over ahip_compute_cell on a trajectory: a caller that hands over nearly the same structure again and again.

   python pair_allegro_amd/tools/cell_reuse_cost.py [--steps 200] [--reps 3] [--out FILE]          (GPU box)

A random walk (Gaussian steps of --sigma A per coordinate and call, cumulative) on the 64-atom Si cell (2 x 2 x 2 diamond cells) and on the 10 648-atom Si box
(11 x 11 x 11), float32 model S, r_max 5 A, one GPU, one process, one library, one model handle per route.  "fresh": a loop of Model.compute_cell, skin
--fresh-skin (0: a caller that keeps nothing has no use for a skin) -- upload, wrap, ghosts, list, evaluation, download per call.  "reuse": the same loop
through Model.compute_cell_reuse with skin --skin.  Host wall clock around each loop (every call returns host arrays, so the device is idle when it
returns).  One warm-up of each, then --reps alternating repetitions, every repetition of the reuse route starting without a hold; the medians are reported
as microseconds per call, with the share of calls that rebuilt and the largest force difference between the routes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.02, help="standard deviation of one step of the walk per coordinate, A")
    ap.add_argument("--skin", type=float, default=1.0, help="skin of the reuse route, A")
    ap.add_argument("--fresh-skin", type=float, default=0.0, help="skin of the compute_cell route, A")
    ap.add_argument("--cells", default="2,11", help="diamond cells per edge of the boxes, comma-separated")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    cfg = model_file.model_S()
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
            mt = np.zeros(n, np.int32)
            rng = np.random.RandomState(7)
            xs = list(pos[None] + np.cumsum(rng.normal(scale=a.sigma, size=(a.steps,) + pos.shape), axis=0))
            fresh_m, reuse_m = capi.Model(path, 0, lib), capi.Model(path, 0, lib)

            def fresh():
                t = time.perf_counter()
                out = [fresh_m.compute_cell(x, mt, cell, (1, 1, 1), a.fresh_skin, want_eatom=False)[1] for x in xs]
                return time.perf_counter() - t, out

            def reuse():
                reuse_m.cell_reuse_reset()
                t = time.perf_counter()
                out = [reuse_m.compute_cell_reuse(x, mt, cell, (1, 1, 1), a.skin, want_eatom=False)[1] for x in xs]
                return time.perf_counter() - t, out

            _, fo = fresh()
            _, ro = reuse()
            calls, rebuilds = reuse_m.cell_reuse_stats()
            df = max(float(np.abs(p - q).max()) for p, q in zip(fo, ro))
            fmax = max(float(np.abs(p).max()) for p in fo)
            paths = (fresh_m.last_path, reuse_m.last_path)
            nghost = len(reuse_m.last_cell_rows()) - n
            t_fresh, t_reuse = [], []
            for _ in range(a.reps):
                t_fresh.append(fresh()[0])
                t_reuse.append(reuse()[0])
            fresh_m.close(); reuse_m.close()
            us = lambda t: 1e6 * float(np.median(t)) / a.steps
            res = dict(atoms=n, ghosts_at_skin=nghost, steps=a.steps, sigma=a.sigma, skin=a.skin, fresh_skin=a.fresh_skin, path_fresh=paths[0], path_reuse=paths[1],
                       fresh_us_per_call=us(t_fresh), reuse_us_per_call=us(t_reuse), ratio=us(t_fresh) / us(t_reuse), rebuilds=rebuilds, calls=calls,
                       fresh_s=[round(t, 6) for t in t_fresh], reuse_s=[round(t, 6) for t in t_reuse], max_dF=df, max_F=fmax)
            results.append(res)
            say(f"{n}-atom Si box, model S float32, r_max {cfg['r_max']} A, {a.steps}-call walk of sigma {a.sigma} A per call; paths: fresh {paths[0]}, reuse {paths[1]}; "
                f"{nghost} ghosts at skin {a.skin} A")
            say(f"  loop of compute_cell (skin {a.fresh_skin})       : {us(t_fresh):9.1f} us per call (median of {a.reps}; whole walk {', '.join(f'{1e3 * t:.2f}' for t in t_fresh)} ms)")
            say(f"  loop of compute_cell_reuse (skin {a.skin}) : {us(t_reuse):9.1f} us per call (median of {a.reps}; whole walk {', '.join(f'{1e3 * t:.2f}' for t in t_reuse)} ms)")
            say(f"  ratio {res['ratio']:.2f}x; {rebuilds} of {calls} calls rebuilt ({100.0 * rebuilds / max(calls, 1):.1f} %); largest force difference between the routes "
                f"{df:.3e} eV/A (largest force {fmax:.3f} eV/A)")
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
