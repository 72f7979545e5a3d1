"""General-cell checks shared by the CPU-emulation tests (test_cell_borders.py) and the GPU tests (test_gpu_cell.py): the ghost rule stated in numpy,
the geometries, and drivers that run the C-ABI calls on tensors of either device."""
import itertools
import os

import numpy as np
import torch

import util
from pair_allegro_amd import capi, lmp_like, model_file

# (geometry, rc, pbc, expected ghosts): counts computed on the CPU, equal to lmp_like.build_rank_system(...).nghost on the fully periodic cases
GHOST_CASES = [
    ("Cu-cubic", 6.0, (1, 1, 1), 360),
    ("Cu-cubic", 16.0, (1, 1, 1), 3426),
    ("Cu2AgO4", 6.0, (1, 1, 1), 345),
    ("aspirin", 6.0, (1, 1, 1), 0),
    ("CuPd-cubic-big", 6.0, (1, 1, 1), 1431),
    ("Cu2AgO4", 6.0, (1, 1, 0), 105),
    ("Cu2AgO4", 6.0, (0, 0, 0), 0),
    ("Cu2AgO4-rotated", 6.0, (1, 1, 1), 345),
]
SENTINEL = -7.0


def fixed_rotation():
    q, r = np.linalg.qr(np.random.RandomState(11).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def geometry(name):
    """cell, wrapped positions, symbols of a committed golden geometry (tests/golden/<name>_r5.npz)"""
    rot = name.endswith("-rotated")
    g = util.load_golden(name.replace("-rotated", "") + "_r5")
    cell, pos = np.array(g["cell"], dtype=np.float64), lmp_like.wrap(g["cell"], g["pos"])
    if rot:
        q = fixed_rotation()
        cell, pos = cell @ q, pos @ q
    return cell, pos, g["symbols"]


def types_of(symbols):
    names = sorted(set(symbols))
    return np.array([names.index(s) % 2 for s in symbols], dtype=np.int32)      # (the border model has two types)


def big_257():
    """CuPd-cubic-big doubled along x and cut to 257 atoms: a thread block boundary and a partial wave"""
    cell, pos, sym = geometry("CuPd-cubic-big")
    cell2 = cell * np.array([[2.0], [1.0], [1.0]])
    pos2 = np.concatenate([pos, pos + cell[0]])[:257]
    return cell2, pos2, (list(sym) + list(sym))[:257]


def reference_ghosts(cell, x, pbc, rc):
    """The rule, stated directly: image n != 0 of atom i is a ghost iff for every d: n_d == 0 on an open axis, -m_d <= s_id + n_d < 1 + m_d on a periodic one
    (s = x cell^-1, m_d = rc / height_d).  Returns the (src, n1, n2, n3) rows in the specified order and the smallest distance of any s + k to a threshold."""
    inv = np.linalg.inv(cell)
    s, m = x @ inv, rc * np.linalg.norm(inv, axis=0)
    K = np.ceil(m).astype(int) + 1
    n = np.array(list(itertools.product(*[range(-k, k + 1) for k in K])))                     # lexicographic, n3 fastest
    t = s[:, None, :] + n[None, :, :]
    ok = np.where(np.asarray(pbc, bool), (t >= -m) & (t < 1 + m), n[None, :, :] == 0).all(-1) & n.any(-1)[None, :]
    i, k = np.nonzero(ok)                                                                    # row-major: ascending atom, then image order
    gap = min(np.abs(t + m).min(), np.abs(t - 1 - m).min())
    return np.concatenate([i[:, None], n[k]], axis=1), gap


def border_model(lib, model_dir, dtype="float64"):
    """a small two-type model: the border and wrap calls only need a handle"""
    cfg = model_file.model_S(model_dtype=dtype, num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8, type_names=["A", "B"])
    path = os.path.join(model_dir, f"cell_border_{dtype}.ahip")
    if not os.path.exists(path):
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    return capi.Model(path, 0, lib)


def run_borders(model, dev, cell, x, mt, pbc, rc, cap):
    """ahip_borders_cell_dev on tensors of `dev` with pre-filled outputs; returns (nghost, xg, mtg, src, shift) as numpy"""
    xt = torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
    mtt = torch.tensor(np.ascontiguousarray(mt), dtype=torch.int32, device=dev)
    xg = torch.full((cap, 3), SENTINEL, dtype=torch.float64, device=dev)
    sh = torch.full((cap, 3), SENTINEL, dtype=torch.float64, device=dev)
    mg = torch.full((cap,), int(SENTINEL), dtype=torch.int32, device=dev)
    src = torch.full((cap,), int(SENTINEL), dtype=torch.int64, device=dev)
    ng = model.borders_cell_dev(len(x), xt.data_ptr(), mtt.data_ptr(), cell, pbc, rc, cap, xg.data_ptr(), mg.data_ptr(), src.data_ptr(), sh.data_ptr())
    return ng, xg.cpu().numpy(), mg.cpu().numpy(), src.cpu().numpy(), sh.cpu().numpy()


def check_ghost_set(model, dev, cell, x, mt, pbc, rc, expected=None):
    ref, gap = reference_ghosts(cell, x, pbc, rc)
    assert gap > 1e-6, f"a tie could decide this case (threshold gap {gap:.3g})"
    if expected is not None:
        assert len(ref) == expected
    ng, xg, mg, src, sh = run_borders(model, dev, cell, x, mt, pbc, rc, len(ref) + 5)
    assert ng == len(ref)
    if ng == 0:
        assert np.all(xg == SENTINEL) and np.all(src == int(SENTINEL))
        return
    shift_ref = ref[:, 1:].astype(np.float64) @ cell
    np.testing.assert_array_equal(src[:ng], ref[:, 0])                                        # ascending source atom ...
    n_got = np.rint(sh[:ng] @ np.linalg.inv(cell)).astype(int)
    np.testing.assert_array_equal(n_got, ref[:, 1:])                                          # ... then (n1, n2, n3) ascending, n3 fastest
    np.testing.assert_allclose(sh[:ng], shift_ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(xg[:ng], x[ref[:, 0]] + shift_ref, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(mg[:ng], mt[ref[:, 0]])
    assert np.all(xg[ng:] == SENTINEL) and np.all(sh[ng:] == SENTINEL) and np.all(mg[ng:] == int(SENTINEL)) and np.all(src[ng:] == int(SENTINEL))


def check_capacity(model, dev):
    """capacity 10 on the 360-ghost case: 360 comes back, rows >= 10 are untouched, the first 10 are the first 10 of the full answer, the retry succeeds"""
    cell, x, sym = geometry("Cu-cubic")
    mt = types_of(sym)
    ng, xg, mg, src, sh = run_borders(model, dev, cell, x, mt, (1, 1, 1), 6.0, 10)
    assert ng == 360
    ng2, xg2, mg2, src2, sh2 = run_borders(model, dev, cell, x, mt, (1, 1, 1), 6.0, 400)
    assert ng2 == 360
    np.testing.assert_array_equal(xg, xg2[:10]); np.testing.assert_array_equal(sh, sh2[:10]); np.testing.assert_array_equal(src, src2[:10])
    assert np.all(xg2[360:] == SENTINEL) and np.all(src2[360:] == int(SENTINEL))
    ng3, xg3, mg3, src3, sh3 = run_borders(model, dev, cell, x, mt, (1, 1, 1), 6.0, 0)        # counting alone
    assert ng3 == 360
    # a buffer larger than the capacity handed over: the rows behind the capacity keep what they held
    xt = torch.tensor(x, dtype=torch.float64, device=dev); mtt = torch.tensor(mt, dtype=torch.int32, device=dev)
    big = [torch.full((50, 3), SENTINEL, dtype=torch.float64, device=dev), torch.full((50,), int(SENTINEL), dtype=torch.int32, device=dev),
           torch.full((50,), int(SENTINEL), dtype=torch.int64, device=dev), torch.full((50, 3), SENTINEL, dtype=torch.float64, device=dev)]
    assert model.borders_cell_dev(len(x), xt.data_ptr(), mtt.data_ptr(), cell, (1, 1, 1), 6.0, 10, *[b.data_ptr() for b in big]) == 360
    for b, full in zip(big, (xg2, mg2, src2, sh2)):
        b = b.cpu().numpy()
        np.testing.assert_array_equal(b[:10], full[:10])
        assert np.all(b[10:] == SENTINEL)


def check_orthogonal_reduction(model, dev):
    """diamond_si(2) (box 10.86 A), rc = 6: the set of (src, shift) equals that of ahip_borders_local_dev"""
    cell, x, _ = lmp_like.diamond_si(2)
    mt = np.zeros(len(x), np.int32)
    ng, xg, mg, src, sh = run_borders(model, dev, cell, x, mt, (1, 1, 1), 6.0, 4096)
    xt = torch.tensor(x, dtype=torch.float64, device=dev); mtt = torch.tensor(mt, dtype=torch.int32, device=dev)
    o = [torch.zeros((4096, 3), dtype=torch.float64, device=dev), torch.zeros(4096, dtype=torch.int32, device=dev),
         torch.zeros(4096, dtype=torch.int64, device=dev), torch.zeros((4096, 3), dtype=torch.float64, device=dev)]
    box = np.diag(cell).copy()
    nl = model.borders_local_dev(len(x), xt.data_ptr(), mtt.data_ptr(), np.zeros(3), box, box, 6.0, 4096, *[b.data_ptr() for b in o])
    assert ng == nl and 0 < ng <= 4096
    a = np.concatenate([src[:ng, None].astype(np.float64), sh[:ng]], axis=1)
    b = np.concatenate([o[2].cpu().numpy()[:nl, None].astype(np.float64), o[3].cpu().numpy()[:nl]], axis=1)
    np.testing.assert_array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])


def run_wrap(model, dev, cell, x, pbc):
    xt = torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
    model.wrap_cell_dev(len(x), xt.data_ptr(), cell, pbc)
    return xt.cpu().numpy()


def check_wrap(model, dev, name="Cu2AgO4"):
    cell, x, _ = geometry(name)
    rng = np.random.RandomState(3)
    x = np.tile(x, (40, 1))                                                                   # 280 rows: more than one block
    k = rng.randint(-4, 5, size=x.shape)
    tol = 1e-12 * np.abs(cell).max()
    np.testing.assert_array_equal(run_wrap(model, dev, cell, x, (1, 1, 1)), x)                # already inside: bit for bit
    np.testing.assert_allclose(run_wrap(model, dev, cell, x + k @ cell, (1, 1, 1)), x, rtol=0, atol=tol)
    inv = np.linalg.inv(cell)
    for pbc in ((1, 1, 0), (0, 1, 0), (0, 0, 0)):
        moved = x + k @ cell
        got = run_wrap(model, dev, cell, moved, pbc)
        want = x + (k * (1 - np.asarray(pbc))) @ cell                                         # only the periodic axes come back
        np.testing.assert_allclose(got, want, rtol=0, atol=tol)
        open_axes = [d for d in range(3) if not pbc[d]]
        np.testing.assert_allclose((got @ inv)[:, open_axes], (moved @ inv)[:, open_axes], rtol=0, atol=1e-12)
        if not any(pbc):
            np.testing.assert_array_equal(got, moved)


def check_errors(model, dev):
    cell, x, sym = geometry("Cu2AgO4")
    mt = types_of(sym)
    singular = cell.copy(); singular[2] = singular[0] + singular[1]
    nan = cell.copy(); nan[1, 1] = np.nan
    for bad in (singular, nan, np.zeros((3, 3))):
        for call in (lambda: run_borders(model, dev, bad, x, mt, (1, 1, 1), 6.0, 16), lambda: run_wrap(model, dev, bad, x, (1, 1, 1)),
                     lambda: model.compute_cell(x, mt, bad)):
            try:
                call()
            except capi.AhipError as e:
                assert e.code == capi.AHIP_ERR_ARG, e
            else:
                raise AssertionError("a singular / non-finite cell was accepted")
    for badtype in (-1, model.num_types):
        mt2 = mt.copy(); mt2[3] = badtype
        try:
            model.compute_cell(x, mt2, cell)
        except capi.AhipError as e:
            assert e.code == capi.AHIP_ERR_ARG and "model type" in e.msg, e
        else:
            raise AssertionError("a model type out of range was accepted")
    # nlocal x images per atom beyond 32 bits: refused before any launch
    try:
        run_borders(model, dev, cell * 1e-3, x * 1e-3, mt, (1, 1, 1), 6.0, 16)
    except capi.AhipError as e:
        assert e.code == capi.AHIP_ERR_ARG and "2^31" in e.msg, e
    else:
        raise AssertionError("an image count beyond 2^31 was accepted")
