"""What a model shape costs on the fused kernels against the layer-at-a-time kernels, on the device-resident call (ahip_compute_dev) of a bench.py workload.

   python pair_allegro_amd/tools/shape_gate_cost.py --config 2 --readout-depth 2 [--tensor-features 64] [--l-max 1] [--mlp-depth 3] [--ncell 24]
                                                    [--warmup 5] [--calls 20] [--out profiles/shape_gate_cost.jsonl]          (GPU box)

The geometry and the base model are those of bench.py's --config (2 / 4: diamond Si, model S; 3: Li3PO4, model S; 5 / 6: water, model L / the reference YAML's shape);
the options override the model's read-out depth, tensor features, l_max and MLP depth.  The same file is timed at fixed positions with path=auto (the fused kernel
where csrc/fused_shapes.h finds one) and with path=generic: option timing=1, the stage sums of ahip_get_timings over N calls after a warm-up (HIP events on the launch
stream), and the host wall clock around each call with the device synchronised after it.  One JSON line per case, appended to --out when given."""
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

import bench  # noqa: E402
from pair_allegro_amd import capi, md, model_file  # noqa: E402

PATHS = ("auto", "generic")


def one_case(lib, a):
    wl = bench.workload(a.config, a.ncell)
    cfg = dict(wl["cfg"])
    for key, val in (("readout_depth", a.readout_depth), ("num_tensor_features", a.tensor_features), ("l_max", a.l_max), ("mlp_depth", a.mlp_depth)):
        if val is not None:
            cfg[key] = val
    device = torch.device("cuda", 0)
    out = dict(config=a.config, ncell=a.ncell, atoms=len(wl["pos"]), warmup=a.warmup, calls=a.calls,
               model={k: cfg[k] for k in ("l_max", "num_layers", "num_scalar_features", "num_tensor_features", "mlp_depth", "mlp_width", "readout_depth", "readout_width")})
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.ahip")
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
        for popt in PATHS:
            model = capi.Model(path, 0, lib)
            model.set_option("timing", "1")
            model.set_option("path", popt)
            backend = md.HipBackend(model, wl["masses"])
            vel = np.zeros((len(wl["pos"]), 3))
            sim = md.Simulation(backend, np.diag(wl["cell"]), cfg["r_max"], 1.0, wl["pos"], wl["mtype"], vel, device, dt=0.001, overlap=False)
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
            wall = []
            for _ in range(a.calls):
                t = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t))
            st, cnt = model.timings_and_counts()
            stages = {k: v / a.calls for k, v in st.items()}
            heavy = model.last_heavy_centres
            out[popt] = dict(path=model.last_path, edges=model.nedges(), max_degree=model.last_max_degree, heavy_centres=heavy[0], arith_note=model.arith_note,
                             eval_ms=float(sum(stages.values())), stages_ms=stages, call_ms_median=float(np.median(wall)), call_ms_min=float(np.min(wall)))
            print(f"{popt:8s} path {model.last_path:12s} edges {model.nedges()} stages {out[popt]['eval_ms']:9.3f} ms per evaluation, call {np.median(wall):9.3f} ms "
                  f"(min {np.min(wall):.3f})", flush=True)
            model.close()
            del sim, backend
            torch.cuda.synchronize()
    out["ratio_generic_over_auto"] = out["generic"]["eval_ms"] / out["auto"]["eval_ms"] if out["auto"]["eval_ms"] > 0 else None
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, help="bench.py config: geometry and base model")
    ap.add_argument("--ncell", type=int, default=0, help="replication override of the config, as in bench.py")
    ap.add_argument("--readout-depth", type=int, default=None)
    ap.add_argument("--tensor-features", type=int, default=None)
    ap.add_argument("--l-max", type=int, default=None)
    ap.add_argument("--mlp-depth", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    one_case(capi.Library(), a)


if __name__ == "__main__":
    main()
