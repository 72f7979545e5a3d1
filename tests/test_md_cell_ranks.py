"""The driver on a decomposed general cell, on the CPU: md.Simulation with a 3x3 box and 2 / 4 gloo ranks (bricks of fractional coordinates: ahip_comm_migrate_cell,
ahip_comm_borders_cell and the vector-shift forward exchange through the host-emulation library) against the one-rank run of the same cell."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pair_allegro_amd import capi, md, model_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_workers(emu_lib, model_dir, tmp_path, world, port, extra):
    out = tmp_path / f"cell{world}.npz"
    worker = os.path.join(ROOT, "tests", "md_cell_worker.py")
    env = dict(os.environ, PYTHONPATH=ROOT + ":" + os.path.join(ROOT, "tests"), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), worker, str(out), emu_lib.path, model_dir] + [str(e) for e in extra]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return np.load(out)


@pytest.mark.parametrize("world,port,overlap", [(2, 29771, 0), (4, 29773, 1)])
def test_gloo_ranks_on_a_triclinic_cell_match_one_rank(emu_lib, model_dir, tmp_path, world, port, overlap):
    """(l) cell Q on 2x1x1 and 2x2x1 bricks, 256 hot atoms, 10 steps with a re-neighboring forced every 4 (the first one wraps atoms that start outside the cell):
    atoms change bricks, nobody is lost, and forces after setup, positions and energy after the run equal the one-rank 3x3 run within the bars of the orthogonal
    gloo tests (tests/test_md_emu.py: forces 1e-10, positions 1e-8 and energy 1e-9 relative once atoms migrate).  The 4-rank run uses the overlapped schedule,
    whose interior / boundary split is taken in fractional coordinates."""
    z = _run_workers(emu_lib, model_dir, tmp_path, world, port, extra=(30000.0, 10, 0.5, overlap))
    assert int(z["nreb"]) >= 3 and int(z["nreb1"]) >= 3
    assert int(z["moved"]) >= 1, "no atom changed its brick"
    if overlap:
        assert int(z["n_int"]) > 0, "rank 0 has no interior atom: the overlapped schedule has nothing to overlap"
    np.testing.assert_allclose(z["f2"], z["f1"], atol=1e-10)
    np.testing.assert_allclose(z["x2"], z["x1"], atol=1e-8)
    np.testing.assert_allclose(z["e2"], z["e1"], rtol=1e-9)
    assert np.abs(z["f1"]).max() > 1e-3


def test_a_3x3_box_takes_a_grid(emu_lib, model_dir):
    """the constructor: a brick thinner than r_max + skin is refused per axis, a thin periodic axis that is not decomposed as well"""
    cfg = model_file.model_S(model_dtype="float64", num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8)
    path = os.path.join(model_dir, "md_cell_ctor.ahip")
    model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    model = capi.Model(path, 0, emu_lib)
    be = md.HipBackend(model, [28.0855])
    cell = np.array([[32.0, 0, 0], [8, 32, 0], [4, 8, 16]])
    x = np.random.default_rng(1).uniform(0, 1, size=(40, 3)) @ cell
    mt = np.zeros(40, np.int32)

    class Dist:                      # never used: the constructor refuses first
        pass

    with pytest.raises(ValueError, match="axis 2.*thinner than r_max\\+skin"):
        md.Simulation(be, cell, 5.0, 1.0, x, mt, None, torch.device("cpu"), grid=(1, 1, 3), rank=0, dist=Dist())
    thin = cell.copy(); thin[2] = [0, 0, 4.0]
    with pytest.raises(ValueError, match="axis 2.*one rank"):
        md.Simulation(be, thin, 5.0, 1.0, x, mt, None, torch.device("cpu"), grid=(2, 1, 1), rank=0, dist=Dist())
    model.close()
