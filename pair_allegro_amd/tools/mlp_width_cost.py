"""What a latent MLP of width 128 costs on the fused kernels, and what the fused kernels save such a model, on the device-resident call (ahip_compute_dev).

   python pair_allegro_amd/tools/mlp_width_cost.py [--configs 2,6:24] [--warmup 5] [--calls 20] [--out profiles/mlp_width_cost.txt]          (GPU box)
   python pair_allegro_amd/tools/mlp_width_cost.py --configs 5:24 --out profiles/lx64_mlp_width_cost.txt                                     (the k_fused_lx2 case)

Per box (bench.py workloads, `config[:cells per side]`: 2 = 10 648-atom bulk Si, model S on k_fused; 6:24 = 41 472-atom water of 24^3 molecules, the reference YAML's
shape with 32 tensor features on k_fused_lx; 6 alone is bench.py's 499 125-atom box; 5:24 = the same 41 472-atom box with model L, 64 tensor features, on k_fused_lx2,
whose width-128 instances sit behind option lx64_mlp_width=auto: the tool sets it on the "W = 128 fused" model of such a shape), three models at fixed positions on one GPU:
   W = 64   fused             the model as bench.py builds it
   W = 128  fused             the same with mlp_width = 128 (the WT / HT = 8 instances)
   W = 128  path=generic      that file on the layer-at-a-time float32 kernels: what a model wider than 64 ran on before those instances existed
The three are called ALTERNATELY (one call of each per round, after `warmup` rounds), so clock and thermal drift hit them alike; per mode the median over `calls` rounds of
the host wall clock around the call (device synchronised after each) and the model kernel's own time where there is one (stage "model_fused", HIP events on the launch
stream).  Prints the ratios generic / fused at W = 128 and fused W = 128 / fused W = 64, the run-to-run spread of every mode over the alternated calls (max - min and
the 10th..90th percentile range) and whether the fused W = 128 model beats path=generic on the same file by more than the larger spread, and one JSON line per box."""
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

MODES = (("W64_fused", 64, None), ("W128_fused", 128, None), ("W128_generic", 128, "generic"))


def one_config(lib, config, ncell, warmup, calls, emit):
    wl = bench.workload(config, ncell)
    device = torch.device("cuda", 0)
    out = dict(config=config, name=wl["name"], atoms=len(wl["pos"]))
    runs = []
    with tempfile.TemporaryDirectory() as td:
        for key, width, path_opt in MODES:
            cfg = dict(wl["cfg"], mlp_width=width)
            path = os.path.join(td, f"m{width}.ahip")
            if not os.path.exists(path):
                model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
            model = capi.Model(path, 0, lib)
            model.set_option("timing", "1")
            if path_opt:
                model.set_option("path", path_opt)
            elif width > 64 and cfg["num_tensor_features"] > 32:
                model.set_option("lx64_mlp_width", "auto")        # the width-128 instances of k_fused_lx2 are opt-in (csrc/fused_shapes.h)
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
            out[r["key"]] = dict(path=model.last_path, edges=model.nedges(), call_ms_median=float(np.median(r["wall"])), call_ms_min=float(np.min(r["wall"])),
                                 call_ms_max=float(np.max(r["wall"])), call_ms_p10=float(np.percentile(r["wall"], 10)), call_ms_p90=float(np.percentile(r["wall"], 90)),
                                 model_ms=st.get("model_fused", 0.0) / max(cnt.get("model_fused", 1), 1))
            emit(f"config {config} {r['key']:13s} path {model.last_path:12s} edges {model.nedges()} call {np.median(r['wall']):9.3f} ms (min {np.min(r['wall']):.3f}, max {np.max(r['wall']):.3f},"
                 f" p10..p90 {np.percentile(r['wall'], 10):.3f}..{np.percentile(r['wall'], 90):.3f})"
                 f"  model kernel {out[r['key']]['model_ms']:.3f} ms")
            model.close()
        del runs
        torch.cuda.synchronize()
    out["generic_over_fused_W128"] = out["W128_generic"]["call_ms_median"] / out["W128_fused"]["call_ms_median"]
    out["fused_W128_over_W64"] = out["W128_fused"]["call_ms_median"] / out["W64_fused"]["call_ms_median"]
    out["fused_W128_over_W64_kernel"] = out["W128_fused"]["model_ms"] / out["W64_fused"]["model_ms"] if out["W64_fused"]["model_ms"] > 0 else float("nan")
    emit(f"config {config}: at W = 128 the layer-at-a-time kernels take {out['generic_over_fused_W128']:.2f} x the fused call; fused W = 128 takes "
         f"{out['fused_W128_over_W64']:.2f} x fused W = 64 (model kernel alone: {out['fused_W128_over_W64_kernel']:.2f} x)")
    # the run-to-run spread over the alternated calls (max - min of a mode, the larger of the two modes compared) against the margin of the fused model over path=generic
    out["spread_ms"] = max(out[k]["call_ms_max"] - out[k]["call_ms_min"] for k in ("W128_fused", "W128_generic"))
    out["margin_ms"] = out["W128_generic"]["call_ms_median"] - out["W128_fused"]["call_ms_median"]
    out["fused_beats_generic_beyond_spread"] = bool(out["W128_fused"]["path"].startswith("fused") and out["margin_ms"] > out["spread_ms"])
    emit(f"config {config}: fused W = 128 is {out['margin_ms']:.3f} ms per call ahead of path=generic on the same file; run-to-run spread {out['spread_ms']:.3f} ms: "
         f"{'beats it by more than the spread' if out['fused_beats_generic_beyond_spread'] else 'DOES NOT beat it by more than the spread'}")
    emit(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,6:24")
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
