"""What one ahip_compute_cells call saves over a loop of ahip_compute_cell calls on a data set of small cells.

   python pair_allegro_amd/tools/batch_cost.py [--structures 256] [--reps 3] [--out FILE]          (GPU box)

B jittered copies of the 64-atom Si cell (2 x 2 x 2 diamond cells, 10.86 A), float32 model S, r_max 5 A, one GPU, one process, one library, one model
handle.  "loop": B calls of Model.compute_cell, one structure each (upload, wrap, ghosts, list, evaluation, download per structure).  "batch": one call of
Model.compute_cells for all B.  Host wall clock around the calls (each returns host arrays, so the device is idle when it returns).  One warm-up of each,
then --reps alternating repetitions; the medians are reported as microseconds per structure, with the largest force difference between the two ways."""
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
    ap.add_argument("--structures", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jitter", type=float, default=0.05, help="standard deviation of the displacements, A")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    B = a.structures
    cfg = model_file.model_S()
    cell, pos, _ = lmp_like.diamond_si(2)
    cell = np.asarray(cell, dtype=np.float64)
    rng = np.random.RandomState(5)
    xs = [pos + rng.normal(scale=a.jitter, size=pos.shape) for _ in range(B)]
    n = len(pos)
    mt1 = np.zeros(n, np.int32)
    first = (np.arange(B + 1) * n).astype(np.int32)
    x_all, mt_all = np.concatenate(xs), np.zeros(B * n, np.int32)
    cells, pbc = np.tile(cell, (B, 1, 1)), np.ones((B, 3), np.int32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.ahip")
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
        model = capi.Model(path, 0, capi.Library())

        def loop():
            t = time.perf_counter()
            out = [model.compute_cell(x, mt1, cell) for x in xs]
            return time.perf_counter() - t, out

        def batch():
            t = time.perf_counter()
            out = model.compute_cells(first, x_all, mt_all, cells, pbc)
            return time.perf_counter() - t, out

        _, lo = loop()
        path_loop = model.last_path
        _, bo = batch()
        path_batch, ghosts = model.last_path, model.last_cells_ghosts()
        df = max(float(np.abs(bo[1][k * n: (k + 1) * n] - lo[k][1]).max()) for k in range(B))
        de = max(abs(float(bo[0][k]) - lo[k][0]) for k in range(B))
        t_loop, t_batch = [], []
        for _ in range(a.reps):
            t_loop.append(loop()[0])
            t_batch.append(batch()[0])
        model.close()
    us = lambda t: 1e6 * float(np.median(t)) / B
    res = dict(structures=B, atoms_per_structure=n, ghosts_per_structure=float(ghosts.mean()), path_loop=path_loop, path_batch=path_batch,
               loop_us_per_structure=us(t_loop), batch_us_per_structure=us(t_batch), ratio=us(t_loop) / us(t_batch),
               loop_s=[round(t, 6) for t in t_loop], batch_s=[round(t, 6) for t in t_batch], max_dF=df, max_dE=de)
    say(f"{B} jittered copies of the {n}-atom Si cell, model S float32, r_max {cfg['r_max']} A, {ghosts.mean():.0f} ghosts per structure; paths: loop {path_loop}, batch {path_batch}")
    say(f"loop of compute_cell : {us(t_loop):9.1f} us per structure (median of {a.reps}; whole set {', '.join(f'{1e3 * t:.2f}' for t in t_loop)} ms)")
    say(f"one compute_cells    : {us(t_batch):9.1f} us per structure (median of {a.reps}; whole set {', '.join(f'{1e3 * t:.2f}' for t in t_batch)} ms)")
    say(f"ratio {res['ratio']:.1f}x; largest difference between the two ways: forces {df:.3e} eV/A, energy {de:.3e} eV")
    say(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
