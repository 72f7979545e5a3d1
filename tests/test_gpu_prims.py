"""The device-wide primitives of csrc/prims.hip -- exclusive scan, column sums, max, re-neighbouring flag -- called directly (ahip_debug_scan_i32,
ahip_debug_sum_columns_f64, ahip_debug_max_i32, ahip_reneighbor_flag_dev) at the sizes where their wave / block / tile / grid-cap logic changes.
The host-emulation build replaces these kernels by loops, so only the `hip` variants run the shuffles, the LDS and the atomics; the `emu` variants
are the CPU twin that checks the cases themselves (tests/prims_cases.py)."""
import os

import numpy as np
import pytest
import torch

import prims_cases as pcs
from pair_allegro_amd import capi, model_file

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def backend(request):
    """(library, torch device of the `_dev` pointers)"""
    if request.param == "emu":
        return request.getfixturevalue("emu_lib"), torch.device("cpu")
    return request.getfixturevalue("hip_lib"), torch.device("cuda", 0)


@pytest.mark.parametrize("kind", pcs.SCAN_KINDS)
def test_scan_equals_cumsum(backend, kind):
    lib, _ = backend
    for n in pcs.SCAN_N:
        pcs.check_scan(lib, pcs.scan_input(kind, n))


def test_scan_total_of_int32_max(backend):
    pcs.check_scan(backend[0], pcs.scan_int32_max_input())


def test_scan_regrows_its_scratch(backend):
    """a 5-item scan, then 2 300 000 items on the same scratch: more tiles than the first allocation holds"""
    warm, n = pcs.REGROW
    assert (n + 2047) // 2048 > 2 * ((warm + 2047) // 2048) + 1024
    pcs.check_scan(backend[0], pcs.scan_input("random", n), warm_n=warm)


@pytest.mark.parametrize("ncol", pcs.COLSUM_NCOL)
def test_column_sums_equal_fsum(backend, ncol):
    for nrow in pcs.COLSUM_NROW:
        pcs.check_colsum(backend[0], nrow, ncol)


def test_column_sums_refuse_more_than_8_columns(backend):
    """the kernels keep acc[8] / sm[4][8]: ncol = 9 is refused on the host, before any launch"""
    lib, _ = backend
    with pytest.raises(capi.AhipError):
        lib.debug_sum_columns_f64(np.ones(4 * 9), 9)
    np.testing.assert_array_equal(lib.debug_sum_columns_f64(np.ones(4 * 8), 8), np.full(8, 4.0))


def test_max_equals_numpy(backend):
    for n in pcs.MAX_N:
        pcs.check_max(backend[0], n)


def _tiny_model(lib, model_dir):
    cfg = model_file.model_S(model_dtype="float64", num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8)
    path = os.path.join(model_dir, "prims_tiny.ahip")
    if not os.path.exists(path):
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    return capi.Model(path, 0, lib)


def test_reneighbor_flag(backend, model_dir):
    """ahip_reneighbor_flag_dev against float64 numpy: thresholds 1e-3 and 1e-9 on either side of the reach, and the work words are reset by every call
    (zero displacements right after a call that flagged 1 give 0)."""
    lib, dev = backend
    m = _tiny_model(lib, model_dir)
    flag = torch.full((1,), -7, dtype=torch.int32, device=dev)

    def call(n, x, xh, v, half_skin):
        flag.fill_(-7)
        m.reneighbor_flag_dev(n, x.data_ptr(), xh.data_ptr(), v.data_ptr(), pcs.FLAG_DT, half_skin, flag.data_ptr())
        return int(flag.cpu()[0])

    for n in pcs.FLAG_N:
        x, xh, v, reach = pcs.flag_case(n)
        tx, txh, tv = (torch.from_numpy(np.ascontiguousarray(a).reshape(-1, 3)).to(dev) if n else torch.zeros((1, 3), dtype=torch.float64, device=dev)
                       for a in (x, xh, v))
        if n == 0:
            assert call(0, tx, txh, tv, 0.1) == 0
            continue
        for t in pcs.FLAG_THRESHOLDS:
            pcs.check_flag_value(call(n, tx, txh, tv, reach * t), reach, reach * t, f"n = {n}, half_skin = reach * {t!r}")
        assert call(n, tx, txh, tv, reach * (1.0 - 1e-3)) == 1
        still = torch.zeros_like(tv)
        assert call(n, tx, tx, still, 1e-3) == 0, "the maxima of the previous call were not reset"
    m.close()
