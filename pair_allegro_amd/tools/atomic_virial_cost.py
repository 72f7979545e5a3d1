"""What the output "atomic_virial" (per-atom virial) costs on the device-resident call (ahip_compute_dev) of the bench.py workloads.

   python pair_allegro_amd/tools/atomic_virial_cost.py [--configs 4,5,6] [--warmup 5] [--calls 20]          (GPU box)

Per config, three modes at fixed positions on one GPU: nothing registered; "total_energy" registered (the registered-output branch of
ahip_compute_dev: the library's own force / energy arrays, one synchronisation and the read-back of f, eatom, types -- everything but W);
"atomic_virial" registered (the same plus W: the VA instances of the model kernel and the [nall][9] read-back).  Prints ms per call (host wall
clock around the call, the device synchronised after each) and the model kernel's own time (stage "model_fused", HIP events on the launch
stream), and one JSON line per config."""
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

MODES = (None, "total_energy", "atomic_virial")


def one_config(lib, config, warmup, calls):
    wl = bench.workload(config)
    cfg = wl["cfg"]
    device = torch.device("cuda", 0)
    out = dict(config=config, name=wl["name"], atoms=len(wl["pos"]))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.ahip")
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
        for mode in MODES:
            model = capi.Model(path, 0, lib)
            model.set_option("timing", "1")
            if mode:
                model.output_register(mode)
            backend = md.HipBackend(model, wl["masses"])
            vel = np.zeros((len(wl["pos"]), 3))
            sim = md.Simulation(backend, np.diag(wl["cell"]), cfg["r_max"], 1.0, wl["pos"], wl["mtype"], vel, device, dt=0.001, overlap=False)
            sim.setup()
            nall, nl = sim.x.shape[0], sim.nlocal
            f = torch.zeros((nall, 3), dtype=torch.float64, device=device)
            ev = torch.zeros(7, dtype=torch.float64, device=device)

            def call():
                model.compute_dev(nl, nall - nl, sim.x.data_ptr(), sim.mtype.data_ptr(), f.data_ptr(), 0, ev.data_ptr())

            for _ in range(warmup):
                call()
            torch.cuda.synchronize()
            model.timings()
            wall = []
            for _ in range(calls):
                t = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t))
            st, cnt = model.timings_and_counts()
            key = mode or "none"
            out[key] = dict(path=model.last_path, edges=model.nedges(), call_ms_median=float(np.median(wall)), call_ms_min=float(np.min(wall)),
                            model_ms=st.get("model_fused", 0.0) / max(cnt.get("model_fused", 1), 1))
            print(f"config {config} {key:13s} path {model.last_path:12s} edges {model.nedges()} call {np.median(wall):8.3f} ms (min {np.min(wall):.3f})"
                  f"  model kernel {out[key]['model_ms']:.3f} ms", flush=True)
            model.close()
            del sim, backend
            torch.cuda.synchronize()
    out["delta_call_ms"] = out["atomic_virial"]["call_ms_median"] - out["none"]["call_ms_median"]
    out["delta_call_vs_registered_ms"] = out["atomic_virial"]["call_ms_median"] - out["total_energy"]["call_ms_median"]
    out["delta_model_ms"] = out["atomic_virial"]["model_ms"] - out["none"]["model_ms"]
    print(f"config {config}: atomic_virial adds {out['delta_model_ms']:.3f} ms to the model kernel, {out['delta_call_ms']:.3f} ms to the call "
          f"({out['delta_call_vs_registered_ms']:.3f} ms over a call with another output registered)", flush=True)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,5,6")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    lib = capi.Library()
    for c in a.configs.split(","):
        one_config(lib, int(c), a.warmup, a.calls)


if __name__ == "__main__":
    main()
