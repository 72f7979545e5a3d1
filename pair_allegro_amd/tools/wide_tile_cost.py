"""What option wide_tile costs or saves on a dense l_max = 2 list: an fcc box whose every centre has 78 edges (more than a 64-slot tile of k_fused_lx holds), on the
device-resident call (ahip_compute_dev) at fixed positions.

   python pair_allegro_amd/tools/wide_tile_cost.py --wide-tile auto [--label tree_auto] [--lib path/to/liballegro_hip.so] [--ncell 30] [--skin 0.15]
                                                   [--warmup 3] [--calls 10] [--out profiles/wide_tile_cost.jsonl]          (GPU box)

The box: ncell^3 fcc cells (a = 3.615 A, 0.02 A jitter; 30 -> 108 000 atoms, 8.4 M edges) with the 5.95 A cutoff of tests/wide_tile_cases.py: all78, on the reference
YAML's model shape (l_max = 2, 32 tensor features, 3 layers).  One library and one value of the option per process (--wide-tile none: the option is not set at all,
for a library that does not know it), so that a driver script can alternate processes of the versions it compares on the same box; each appends one JSON line:
milliseconds per evaluation as the median of the host wall clock around each call with the device synchronised after it, and the stage sums of option timing=1."""
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
import torch  # noqa: E402

from pair_allegro_amd import capi, md, model_file  # noqa: E402

A0, R78 = 3.615, 5.95


def fcc_box(ncell, seed=7):
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    g = np.stack(np.meshgrid(*(np.arange(ncell),) * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    pos = (g[:, None, :] + base[None, :, :]).reshape(-1, 3) * A0
    pos = pos + np.random.RandomState(seed).uniform(-0.02, 0.02, size=pos.shape)
    box = np.full(3, A0 * ncell)
    return box, np.mod(pos, box)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide-tile", default="auto", help="64 | auto | none (do not set the option)")
    ap.add_argument("--label", default=None)
    ap.add_argument("--lib", default=None, help="library to load instead of the tree's own")
    ap.add_argument("--ncell", type=int, default=30)
    ap.add_argument("--skin", type=float, default=0.15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    lib = capi.Library(a.lib)
    box, pos = fcc_box(a.ncell)
    cfg = model_file.model_L(type_names=["Cu"], r_max=R78, num_tensor_features=32, avg_num_neighbors=78.0)
    device = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.ahip")
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
        model = capi.Model(path, 0, lib)
        model.set_option("timing", "1")
        if a.wide_tile != "none":
            model.set_option("wide_tile", a.wide_tile)
        backend = md.HipBackend(model, np.array([63.546]))
        mtype = np.zeros(len(pos), dtype=np.int32)
        sim = md.Simulation(backend, box, cfg["r_max"], a.skin, pos, mtype, np.zeros((len(pos), 3)), device, dt=0.001, overlap=False)
        sim.setup()
        nall, nl = sim.x.shape[0], sim.nlocal
        f = torch.zeros((nall, 3), dtype=torch.float64, device=device)
        ev = torch.zeros(7, dtype=torch.float64, device=device)

        def call():
            model.compute_dev(nl, nall - nl, sim.x.data_ptr(), sim.mtype.data_ptr(), f.data_ptr(), 0, ev.data_ptr())

        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        model.timings()
        f.zero_()
        wall = []
        for _ in range(a.calls):
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t))
        st, _cnt = model.timings_and_counts()
        stages = {k: v / a.calls for k, v in st.items()}
        heavy = model.last_heavy_centres
        used, total = model.tile_occupancy()
        out = dict(label=a.label or a.wide_tile, wide_tile=a.wide_tile, lib=os.path.relpath(lib.path, ROOT), ncell=a.ncell, atoms=len(pos), skin=a.skin, warmup=a.warmup,
                   calls=a.calls, path=model.last_path, edges=model.nedges(), max_degree=model.last_max_degree, heavy_centres=heavy[0], tile_slots_used=used,
                   tile_slots_total=total, energy=float(ev[0]), f_rms=float(torch.sqrt((f[:nl] / a.calls).pow(2).mean())),
                   call_ms_median=float(np.median(wall)), call_ms_min=float(np.min(wall)), call_ms_max=float(np.max(wall)), eval_ms_stages=float(sum(stages.values())),
                   stages_ms=stages)
        model.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
