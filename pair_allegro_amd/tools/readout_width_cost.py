"""What a read-out MLP of width 64 costs on the fused kernels, and what the fused kernels save such a model, on the device-resident call (ahip_compute_dev).

   python pair_allegro_amd/tools/readout_width_cost.py [--configs 2,6:24,5:24] [--warmup 5] [--calls 20] [--out profiles/readout_width_cost.txt]          (GPU box)

Per box (bench.py workloads, `config[:cells per side]`: 2 = 10 648-atom bulk Si, model S on k_fused; 6:24 = 41 472-atom water of 24^3 molecules, the reference YAML's
shape with 32 tensor features on k_fused_lx; 5:24 = the same box with model L, 64 tensor features, on k_fused_lx2), three models at fixed positions on one GPU:
   R = 32  fused             the model as bench.py builds it
   R = 64  fused             the same with readout_width = 64 (the RT = 4 instances)
   R = 64  path=generic      that file on the layer-at-a-time float32 kernels: what a model with a read-out wider than 32 ran on before those instances existed
The three are called ALTERNATELY (one call of each per round, after `warmup` rounds), so clock and thermal drift hit them alike; per mode the median over `calls` rounds of
the host wall clock around the call (device synchronised after each) and the model kernel's own time where there is one (stage "model_fused", HIP events on the launch
stream).  Prints the ratios generic / fused at R = 64 and fused R = 64 / fused R = 32, and one JSON line per box."""
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

MODES = (("R32_fused", 32, None), ("R64_fused", 64, None), ("R64_generic", 64, "generic"))


def one_config(lib, config, ncell, warmup, calls, emit):
    wl = bench.workload(config, ncell)
    device = torch.device("cuda", 0)
    out = dict(config=config, name=wl["name"], atoms=len(wl["pos"]))
    runs = []
    with tempfile.TemporaryDirectory() as td:
        for key, width, path_opt in MODES:
            cfg = dict(wl["cfg"], readout_width=width)
            path = os.path.join(td, f"r{width}.ahip")
            if not os.path.exists(path):
                model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
            model = capi.Model(path, 0, lib)
            model.set_option("timing", "1")
            if path_opt:
                model.set_option("path", path_opt)
            backend = md.HipBackend(model, wl["masses"])
            vel = np.zeros((len(wl["pos"]), 3))
            sim = md.Simulation(backend, np.diag(wl["cell"]), cfg["r_max"], 1.0, wl["pos"], wl["mtype"], vel, device, dt=0.001, overlap=False)
            sim.setup()
            nall, nl = sim.x.shape[0], sim.nlocal
            f = torch.zeros((nall, 3), dtype=torch.float64, device=device)
            ev = torch.zeros(7, dtype=torch.float64, device=device)

            def call(model=model, sim=sim, f=f, ev=ev, nl=nl, nall=nall):
                model.compute_dev(nl, nall - nl, sim.x.data_ptr(), sim.mtype.data_ptr(), f.data_ptr(), 0, ev.data_ptr())

            runs.append(dict(key=key, model=model, sim=sim, backend=backend, call=call, wall=[], keep=(f, ev)))
        for _ in range(warmup):
            for r in runs:
                r["call"]()
                torch.cuda.synchronize()
        for r in runs:
            r["model"].timings()
        for _ in range(calls):
            for r in runs:
                t = time.perf_counter()
                r["call"]()
                torch.cuda.synchronize()
                r["wall"].append(1e3 * (time.perf_counter() - t))
        for r in runs:
            model = r["model"]
            st, cnt = model.timings_and_counts()
            kernel_ms = st.get("model_fused", 0.0) / max(cnt.get("model_fused", 1), 1)
            out[r["key"]] = dict(path=model.last_path, edges=model.nedges(), call_ms_median=float(np.median(r["wall"])), call_ms_min=float(np.min(r["wall"])), model_ms=kernel_ms)
            emit(f"config {config} {r['key']:12s} path {model.last_path:12s} edges {model.nedges()} call {np.median(r['wall']):9.3f} ms (min {np.min(r['wall']):.3f})"
                 f"  model kernel {kernel_ms:.3f} ms")
            model.close()
        del runs
        torch.cuda.synchronize()
    out["generic_over_fused_R64"] = out["R64_generic"]["call_ms_median"] / out["R64_fused"]["call_ms_median"]
    out["fused_R64_over_R32"] = out["R64_fused"]["call_ms_median"] / out["R32_fused"]["call_ms_median"]
    out["fused_R64_over_R32_kernel"] = out["R64_fused"]["model_ms"] / out["R32_fused"]["model_ms"] if out["R32_fused"]["model_ms"] > 0 else float("nan")
    emit(f"config {config}: at R = 64 the layer-at-a-time kernels take {out['generic_over_fused_R64']:.2f} x the fused call; fused R = 64 takes "
         f"{out['fused_R64_over_R32']:.2f} x fused R = 32 (model kernel alone: {out['fused_R64_over_R32_kernel']:.2f} x)")
    emit(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,6:24,5:24")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    lib = capi.Library()
    for c in a.configs.split(","):
        config, _, ncell = c.partition(":")
        one_config(lib, int(config), int(ncell or 0), a.warmup, a.calls, emit)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
