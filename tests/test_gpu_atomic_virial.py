"""Output "atomic_virial" on the MI355X: every kernel family that produces forces produces W (tests/atomic_virial_ref.py) -- k_fused (2 and 3
layers, four arithmetics), k_fused_lx / k_fused_lx2, the layer-at-a-time kernels in float32 and float64, and the heavy centres of the wide
kernels; under fused_arith=auto's first-evaluation self-check; on the device-resident call; and registering it changes nothing else."""
import numpy as np
import pytest

import atomic_virial_ref as av
import parity_cases as pc
import util
from pair_allegro_amd import capi, lmp_like, model_file

pytestmark = pytest.mark.gpu

NAMES = ["Ag", "Cu", "O"]
# kernel -> model overrides (as tests/test_gpu_path_parity.py): k_fused model S, k_fused_lx U = 32, k_fused_lx2 U = 64
KERNELS = {
    "k_fused_nl2": dict(num_layers=2),
    "k_fused_nl3": dict(num_layers=3),
    "k_fused_lx": dict(l_max=2, num_tensor_features=32),
    "k_fused_lx2": dict(l_max=2, num_tensor_features=64),
}
BAR = {"f32": 2e-5, "f16x2": 2e-5, "bf16x3": 2e-5, "tf32eq": 1e-4}
_cases = {}


def _case(model_dir, kernel, dtype="float32"):
    """Cu2AgO4 (3 types, triclinic) with the kernel's model shape; the float64 oracle's W."""
    key = (kernel, dtype)
    if key not in _cases:
        g = util.load_golden("Cu2AgO4_r5")
        over = dict(KERNELS[kernel], type_names=NAMES, avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), model_dtype=dtype)
        cfg = model_file.model_L(**over) if over.get("l_max", 1) == 2 else model_file.model_S(**over)
        w = model_file.init_weights(cfg)
        path = f"{model_dir}/gav_{kernel}_{dtype}.ahip"
        model_file.save_ahip(path, cfg, w)
        types = np.array([NAMES.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
        rs = av.rank_system(cfg, g["cell"], g["pos"], types)
        _cases[key] = (cfg, path, rs, av.oracle_w(cfg, w, rs, NAMES))
    return _cases[key]


def _check(res, ref, bar, sum_bar):
    assert res["W"].shape == ref.shape
    scale = np.abs(ref).max()
    err = np.abs(res["W"] - ref).max()
    assert err <= bar * scale, (res["path"], err, scale)
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    dv = np.abs(av.sym_sum(res["W"]) - res["virial"]).max()
    assert dv <= sum_bar * rowscale, (res["path"], dv, rowscale)


def _instances():
    out = []
    for k in KERNELS:
        for a in (("f32", "f16x2", "bf16x3", "tf32eq") if k.startswith("k_fused_nl") else ("f32", "f16x2")):
            out.append((k, a))
    return out


@pytest.mark.parametrize("kernel,arith", _instances())
def test_atomic_virial_fused_kernels(hip_lib, model_dir, kernel, arith):
    cfg, path, rs, ref = _case(model_dir, kernel)
    res = av.run(hip_lib, path, rs, NAMES, options={"path": "fused", "fused_arith": arith})
    assert res["path"] == f"fused_{arith}"
    _check(res, ref, BAR[arith], 1e-6)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_atomic_virial_layer_at_a_time(hip_lib, model_dir, dtype):
    for kernel in ("k_fused_nl2", "k_fused_lx2"):
        cfg, path, rs, ref = _case(model_dir, kernel, dtype)
        res = av.run(hip_lib, path, rs, NAMES, options={"path": "generic"})
        assert res["path"] == ("generic_f32" if dtype == "float32" else "generic_f64")
        if dtype == "float32":
            _check(res, ref, 2e-5, 1e-6)
        else:
            _check(res, ref, 1e-10, 1e-12)


def test_atomic_virial_heavy_centres(hip_lib, model_dir):
    """Water box with centres of more than 64 edges (test_gpu_fused_lx.py: test_model_L_centres_with_more_than_64_edges): those centres run on the
    layer-at-a-time kernels over a compact copy of their edges, the rest on the wide fused kernel; W must equal the all-generic W."""
    cell, pos, types = lmp_like.water(14)
    cfg = model_file.model_L(avg_num_neighbors=53.6)
    path = f"{model_dir}/gav_water_L14.ahip"
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    rs = av.rank_system(cfg, cell, pos, types)
    gen = av.run(hip_lib, path, rs, ["O", "H"], options={"path": "generic"})
    res = av.run(hip_lib, path, rs, ["O", "H"])
    assert gen["path"] == "generic_f32" and res["path"] in pc.FUSED_F32EQ
    assert res["max_degree"] > 64
    scale = np.abs(gen["W"]).max()
    assert np.abs(res["W"] - gen["W"]).max() <= 5e-5 * scale
    rowscale = np.abs(res["W"]).max(axis=1).sum()
    assert np.abs(av.sym_sum(res["W"]) - res["virial"]).max() <= 1e-6 * rowscale


def test_atomic_virial_auto_self_check(hip_lib, model_dir, monkeypatch):
    """fused_arith=auto on a model's first evaluation runs the f32 and the f16x2 instances (2-3 dispatches); W is that of the kept instance."""
    monkeypatch.delenv("AHIP_NO_ARITH_SELFCHECK", raising=False)
    cfg, path, rs, ref = _case(model_dir, "k_fused_nl2")
    res = av.run(hip_lib, path, rs, NAMES)
    assert res["path"] == pc.FUSED_DEFAULT
    kept = av.run(hip_lib, path, rs, NAMES, options={"path": "fused", "fused_arith": "f16x2"})
    scale = np.abs(ref).max()
    assert np.abs(res["W"] - kept["W"]).max() <= 1e-9 * scale
    _check(res, ref, 2e-5, 1e-6)


def _dev_run(lib, path, rs, cfg, options, register=True):
    import torch
    m = capi.Model(path, 0, lib)
    for k, v in options.items():
        m.set_option(k, v)
    if register:
        m.output_register("atomic_virial")
    m.neigh_update_csr(rs.nall, rs.ilist, rs.offsets, rs.flat)
    mapper = np.array([cfg["type_names"].index(s) for s in NAMES], dtype=np.int32)
    dev = torch.device("cuda", 0)
    x = torch.tensor(rs.x, device=dev)
    mt = torch.tensor(mapper[rs.type - 1], dtype=torch.int32, device=dev)
    f = torch.zeros_like(x)
    ev = torch.zeros(7, dtype=torch.float64, device=dev)
    m.compute_dev(rs.nlocal, rs.nghost, x.data_ptr(), mt.data_ptr(), f.data_ptr(), 0, ev.data_ptr())
    torch.cuda.synchronize()
    out = dict(f=f.cpu().numpy(), ev=ev.cpu().numpy(), path=m.last_path, W=m.output_get("atomic_virial").reshape(-1, 9) if register else None)
    m.close()
    return out


@pytest.mark.parametrize("kernel", ["k_fused_nl2", "k_fused_lx2"])
def test_atomic_virial_device_resident_call(hip_lib, model_dir, kernel):
    cfg, path, rs, ref = _case(model_dir, kernel)
    opts = {"path": "fused", "fused_arith": "f16x2"}
    host = av.run(hip_lib, path, rs, NAMES, options=opts)
    dev = _dev_run(hip_lib, path, rs, cfg, opts)
    assert dev["path"] == host["path"] == "fused_f16x2"
    assert np.abs(dev["W"] - host["W"]).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(dev["W"] - ref).max() <= 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize("kernel,arith", [("k_fused_nl2", "f16x2"), ("k_fused_nl3", "f32"), ("k_fused_lx", "f16x2"), ("k_fused_lx2", "f32"),
                                          ("k_fused_nl2", "generic")])
def test_atomic_virial_changes_nothing_else(hip_lib, model_dir, kernel, arith):
    cfg, path, rs, ref = _case(model_dir, kernel)
    opts = {"path": "generic"} if arith == "generic" else {"path": "fused", "fused_arith": arith}
    a = av.run(hip_lib, path, rs, NAMES, options=opts)
    b = av.run(hip_lib, path, rs, NAMES, options=opts, register=False)
    assert a["path"] == b["path"]
    for q in ("f", "eatom", "virial"):
        assert np.abs(a[q] - b[q]).max() <= 1e-10 * np.abs(b[q]).max(), (q, a["path"])
    assert abs(a["pe"] - b["pe"]) <= 1e-10 * abs(b["pe"])
    da = _dev_run(hip_lib, path, rs, cfg, opts)
    db = _dev_run(hip_lib, path, rs, cfg, opts, register=False)
    for k in ("f", "ev"):
        assert np.abs(da[k] - db[k]).max() <= 1e-10 * np.abs(db[k]).max(), (k, da["path"])
