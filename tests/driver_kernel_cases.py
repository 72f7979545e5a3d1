"""Cases of the stand-alone driver's kernels (csrc/neigh.hip: cell-list neighbour builder, KOKKOS table hand-over, type mapping, NVE half steps;
csrc/comm.hip: the one-rank exchange plan), shared by the CPU twin (the same kernels as loops in the host-emulation build) and the GPU run of
tests/test_gpu_driver_kernels.py.  `dev` is the torch device whose tensors stand for device memory (cpu for the emulation)."""
import os

import numpy as np
import pytest
import torch

from pair_allegro_amd import capi, model_file

RC = 5.0
NAMES = ["Cu", "Pd"]


def model(lib, model_dir):
    """float64 two-type model S (small widths), layer-at-a-time path: the edge filter of the evaluation is float64 like the brute force"""
    cfg = model_file.model_S(model_dtype="float64", type_names=NAMES, r_max=RC, num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8)
    path = os.path.join(model_dir, "driver_kernels_f64.ahip")
    if not os.path.exists(path):
        model_file.save_ahip(path, cfg, model_file.init_weights(cfg))
    m = capi.Model(path, 0, lib)
    m.set_option("path", "generic")
    return m


def to_dev(a, dev, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev)          # always a copy: a cpu tensor would share the numpy array's memory


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ neighbour builder
def hand_placed():
    """16 A box: a pair exactly at the cutoff along an axis, a 3-4-5 pair exactly at it, two atoms on one point, an atom at box - 1e-13 (its image sits at
    -1e-13, next to the atoms at 0), a pair one ulp beyond the cutoff.  Returns (positions, pairs that must be edges, pairs that must not)."""
    x = np.array([[2.0, 2.0, 2.0], [7.0, 2.0, 2.0],                           # 0-1: exactly rc along x
                  [0.0, 0.0, 0.0], [0.0, 3.0, 4.0],                           # 2-3: 9 + 16 = 25 exactly
                  [10.0, 10.0, 10.0], [10.0, 10.0, 10.0],                     # 4-5: identical positions
                  [16.0 - 1e-13, 8.0, 8.0], [1.0, 8.0, 8.0],                  # 6: image at -1e-13, 1.0000000000001 from atom 7
                  [12.0, 13.0, 0.0], [12.0, 13.0, np.nextafter(RC, 6.0)]])    # 8-9: one ulp beyond rc
    return x, [(0, 1), (2, 3), (4, 5)], [(8, 9)]


def gas(n, box, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 3)) * np.asarray(box)


# name -> (box, positions, (lo pad, hi pad) of the bin grid per dimension or None for the driver's halo + 1e-6, bins expected per dimension)
def neighbour_cases():
    h = hand_placed()[0]
    halo = None
    return {
        "gas300": ((17.3, 11.1, 26.0), gas(300, (17.3, 11.1, 26.0), 1), halo, (5, 4, 7)),
        "box5_26_images": ((5.0, 5.0, 5.0), gas(7, (5.0, 5.0, 5.0), 2), halo, (3, 3, 3)),
        "one_and_two_bins": ((9.9, 5.2, 31.0), gas(120, (9.9, 5.2, 31.0), 3), ((0.0, 2.5, RC), (0.0, 2.5, RC)), (1, 2, 8)),     # ghosts beyond the grid are clamped
        "bin_cap_1024": ((6000.0, 5.5, 5.5), gas(500, (6000.0, 5.5, 5.5), 4), halo, (1024, 3, 3)),
        "hand_placed": ((16.0, 16.0, 16.0), h, halo, (5, 5, 5)),
        "hand_placed_clamped": ((16.0, 16.0, 16.0), h, ((-3.0, -3.0, -3.0), (-2.0, -2.0, -2.0)), (2, 2, 2)),      # grid [3, 14): atoms outside on every side
        "no_atoms": ((16.0, 16.0, 16.0), np.zeros((0, 3)), halo, (5, 5, 5)),
        "one_atom": ((16.0, 16.0, 16.0), np.array([[8.0, 8.0, 8.0]]), halo, (5, 5, 5)),
    }


def brute_force(x, nlocal, rc):
    """all (i < nlocal, j < nall, j != i) with dx^2 + dy^2 + dz^2 <= rc^2 in float64, summed in that order"""
    d = x[None, :, :] - x[:nlocal, None, :]
    rsq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    keep = rsq <= rc * rc
    keep[np.arange(nlocal), np.arange(nlocal)] = False
    i, j = np.nonzero(keep)
    return np.stack([i, j]).astype(np.int64)


def pair_keys(ei, nall):
    return ei[0] * max(nall, 1) + ei[1]


class Built:
    """positions + the library's ghosts on the device, the list built by ahip_build_neighbors_dev and one evaluation behind it"""

    def __init__(self, lib, dev, m, box, x, pads, rc_list, seed=0):
        box = np.asarray(box, dtype=np.float64)
        nl = len(x)
        self.nlocal = nl
        mt = np.random.default_rng(seed + 11).integers(0, 2, size=nl).astype(np.int32)
        xl = to_dev(x.reshape(-1, 3) if nl else np.zeros((1, 3)), dev, np.float64)
        mtl = to_dev(mt if nl else np.zeros(1, np.int32), dev, np.int32)
        cap = 27 * nl + 8
        xa = torch.zeros((nl + cap, 3), dtype=torch.float64, device=dev)
        mta = torch.zeros(nl + cap, dtype=torch.int32, device=dev)
        src = torch.zeros(cap, dtype=torch.long, device=dev)
        shv = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
        ng = m.borders_local_dev(nl, xl.data_ptr(), mtl.data_ptr(), np.zeros(3), box, box, rc_list, cap, xa[nl:].data_ptr(), mta[nl:].data_ptr(),
                                 src.data_ptr(), shv.data_ptr())
        assert 0 <= ng <= cap
        if nl:
            xa[:nl] = xl
            mta[:nl] = mtl
        self.nall = nl + ng
        self.x = xa[: max(self.nall, 1)].contiguous()
        self.mt = mta[: max(self.nall, 1)].contiguous()
        self.nghost = ng
        lo_pad, hi_pad = pads if pads is not None else ((rc_list + 1e-6,) * 3, (rc_list + 1e-6,) * 3)
        self.lo, self.hi = -np.asarray(lo_pad, dtype=np.float64), box + np.asarray(hi_pad, dtype=np.float64)
        self.bins = tuple(int(min(max(np.floor(l / rc_list), 1), 1024)) for l in self.hi - self.lo)
        self.m, self.dev, self.rc_list = m, dev, rc_list
        self.xh = self.x.cpu().numpy()[: self.nall]

    def build_and_evaluate(self):
        """(list size, edge_index of one ahip_compute_dev behind the build)"""
        m = self.m
        m.build_neighbors_dev(self.nlocal, self.nall, self.x.data_ptr(), self.lo, self.hi, self.rc_list)
        size = m.nneigh()
        f = torch.zeros((max(self.nall, 1), 3), dtype=torch.float64, device=self.dev)
        ev = torch.zeros(7, dtype=torch.float64, device=self.dev)
        m.compute_dev(self.nlocal, self.nghost, self.x.data_ptr(), self.mt.data_ptr(), f.data_ptr(), 0, ev.data_ptr())
        sync(self.dev)
        ei, _ = m.get_edges()
        return size, ei


def check_neighbour_case(lib, dev, m, name):
    box, x, pads, bins = neighbour_cases()[name]
    b = Built(lib, dev, m, box, x, pads, RC)
    assert b.bins == bins, (b.bins, bins)
    if name == "box5_26_images":
        assert b.nghost == 26 * len(x)
    if name == "one_atom":
        assert b.nall == 1
    size, ei = b.build_and_evaluate()
    ref = brute_force(b.xh, b.nlocal, RC)
    got, want = pair_keys(ei, b.nall), pair_keys(ref, b.nall)
    assert len(np.unique(got)) == len(got), "a pair appears twice"
    assert set(got.tolist()) == set(want.tolist()), (sorted(set(got.tolist()) ^ set(want.tolist()))[:10], len(got), len(want))
    assert size == ref.shape[1], (size, ref.shape[1])
    if name.startswith("hand_placed"):
        _, must, must_not = hand_placed()
        keys = set(got.tolist())
        for i, j in must:
            assert i * b.nall + j in keys and j * b.nall + i in keys, (i, j)
        for i, j in must_not:
            assert i * b.nall + j not in keys and j * b.nall + i not in keys, (i, j)
    size2, ei2 = b.build_and_evaluate()
    assert size2 == size
    np.testing.assert_array_equal(ei2, ei, err_msg="a second build gave another edge order")
    return ei.shape[1]


def check_skin_list(lib, dev, m):
    """rc_list = r_max + 1: the list holds the brute-force pairs at rc_list, the evaluation keeps those at r_max"""
    box, x, _, _ = neighbour_cases()["gas300"]
    b = Built(lib, dev, m, box, x, None, RC + 1.0)
    size, ei = b.build_and_evaluate()
    assert size == brute_force(b.xh, b.nlocal, RC + 1.0).shape[1]
    ref = brute_force(b.xh, b.nlocal, RC)
    assert size > ref.shape[1] > 0
    got = pair_keys(ei, b.nall)
    assert len(np.unique(got)) == len(got) and set(got.tolist()) == set(pair_keys(ref, b.nall).tolist())


# ------------------------------------------------------------------------------------------------ KOKKOS table hand-over, type mapping
def table_system():
    """18^3 jittered grid (3 A), 5000 centres in a permuted ilist, rows of 0 .. 8 neighbours drawn from the grid neighbours and a few far atoms"""
    rng = np.random.default_rng(21)
    g = np.stack(np.meshgrid(*[np.arange(18)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    x = 3.0 * g + rng.uniform(-0.2, 0.2, size=g.shape)
    nall, inum = len(x), 5000
    rows = []
    for i in range(inum):
        cand = [i + d for d in (1, -1, 18, -18, 324, -324) if 0 <= i + d < nall] + [int(c) for c in rng.integers(0, nall, size=3) if c != i]
        rows.append(np.array(rng.permutation(cand)[: int(rng.integers(0, 9))], dtype=np.int32))
    rows[7] = rows[7][:0]                                   # a row of length 0, whatever the draw
    ilist = rng.permutation(inum).astype(np.int32)
    mt = rng.integers(0, 2, size=nall).astype(np.int32)
    return x, mt, nall, inum, ilist, rows


def check_table_handover(lib, dev, m):
    x, mt, nall, inum, ilist, rows = table_system()
    maxn = max(len(r) for r in rows) + 2
    assert inum > 2048, "the scan of the row lengths crosses a tile"
    tab = np.full((inum, maxn), 0x12345678, dtype=np.int32)
    numneigh = np.full(nall, 3, dtype=np.int32)             # atoms that are no centres carry a count nobody may read
    for i, r in enumerate(rows):
        tab[i, : len(r)] = r | (3 << 29)                    # the bits LAMMPS keeps above NEIGHMASK
        numneigh[i] = len(r)
    xd, mtd = to_dev(x, dev, np.float64), to_dev(mt, dev, np.int32)
    ild, nnd = to_dev(ilist, dev, np.int32), to_dev(numneigh, dev, np.int32)

    def evaluate():
        f = torch.zeros((nall, 3), dtype=torch.float64, device=dev)
        ev = torch.zeros(7, dtype=torch.float64, device=dev)
        m.compute_dev(inum, nall - inum, xd.data_ptr(), mtd.data_ptr(), f.data_ptr(), 0, ev.data_ptr())
        sync(dev)
        return m.get_edges() + (f.cpu().numpy(),)

    off = np.concatenate([[0], np.cumsum([len(rows[i]) for i in ilist])]).astype(np.int64)
    flat = np.concatenate([rows[i] for i in ilist]).astype(np.int32)
    m.neigh_update_csr(nall, ilist, off, flat)
    ei0, r0, f0 = evaluate()
    assert ei0.shape[1] > inum
    for layout in ("right", "left"):
        store = to_dev(tab if layout == "right" else np.ascontiguousarray(tab.T), dev, np.int32)      # left: slot-major storage, atom stride 1
        sa, ss = (maxn, 1) if layout == "right" else (1, inum)
        m.neigh_update_dev_table(inum, nall, ild.data_ptr(), nnd.data_ptr(), store.data_ptr(), sa, ss)
        assert m.nneigh() == len(flat)
        ei, r, f = evaluate()
        np.testing.assert_array_equal(ei, ei0, err_msg=layout)
        np.testing.assert_array_equal(r, r0, err_msg=layout)
        np.testing.assert_allclose(f, f0, rtol=0, atol=1e-12 * max(1.0, np.abs(f0).max()))


def check_table_rejections(lib, dev, m):
    """refused by the validation kernels, which write nothing out of range: every bad value is an index inside the table, every pointer is in range"""
    il = to_dev(np.arange(3), dev, np.int32)
    nn = to_dev(np.full(3, 2), dev, np.int32)
    tab = to_dev(np.array([[1, 2], [0, 7], [0, 1]]), dev, np.int32)              # neighbour 7 of a 3-atom system
    with pytest.raises(capi.AhipError, match="neighbour index out of range"):
        m.neigh_update_dev_table(3, 3, il.data_ptr(), nn.data_ptr(), tab.data_ptr(), 2, 1)
    good = to_dev(np.array([[1, 2], [0, 2], [0, 1]]), dev, np.int32)
    bad_il = to_dev(np.array([0, 1, 5]), dev, np.int32)
    with pytest.raises(capi.AhipError, match="ilist entry out of range"):
        m.neigh_update_dev_table(3, 3, bad_il.data_ptr(), nn.data_ptr(), good.data_ptr(), 2, 1)
    with pytest.raises(capi.AhipError, match="strides must be positive"):
        m.neigh_update_dev_table(3, 3, il.data_ptr(), nn.data_ptr(), good.data_ptr(), 0, 1)
    m.neigh_update_dev_table(3, 3, il.data_ptr(), nn.data_ptr(), good.data_ptr(), 2, 1)
    assert m.nneigh() == 6


def check_map_types(lib, dev, m):
    n = 5000
    rng = np.random.default_rng(8)
    types = rng.integers(1, 4, size=n).astype(np.int32)
    mapper = np.array([1, 0, 1], dtype=np.int32)
    td = to_dev(types, dev, np.int32)
    out = torch.full((n + 1,), -9, dtype=torch.int32, device=dev)
    m.map_types_dev(n, td.data_ptr(), mapper, out.data_ptr())
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:n], mapper[types - 1])
    assert got[n] == -9
    with pytest.raises(capi.AhipError, match="not mapped"):
        m.map_types_dev(n, td.data_ptr(), np.array([0, -1, 1], dtype=np.int32), out.data_ptr())
    with pytest.raises(capi.AhipError, match="out of range"):
        m.map_types_dev(n, td.data_ptr(), np.array([0, 1], dtype=np.int32), out.data_ptr())


# ------------------------------------------------------------------------------------------------ NVE half steps
NVE_N = [1, 85, 86, 1000]                   # 3 n = 255 / 258: either side of one 256-thread block
MASSES = [1.008, 107.87]
DT, FTM2V = 0.0007, 1.0 / 1.0364269e-4
SENTINEL = -12345.678
U52 = 2.0 ** -52


def nve_case(n):
    rng = np.random.default_rng(400 + n)
    nall = n + 37
    x, v, f = rng.uniform(-40, 40, (nall + 1, 3)), rng.normal(0, 3.0, (nall + 1, 3)), rng.normal(0, 2.0, (nall + 1, 3))
    for a in (x, v, f):
        a[nall] = SENTINEL                   # the guard row
    mt = rng.integers(0, 2, size=nall + 1).astype(np.int32)
    return nall, x, v, f, mt


def check_nve(lib, dev, m, n, which):
    """which: 0 / 1 = ahip_nve_dev mode, "first" = ahip_nve_first_dev.  Float64 numpy with the library's own dtfm = (dt / 2 * ftm2v) * (1 / mass); the compiler may
    contract v + dtfm f (and x + dt v) to a fused multiply-add, so per element |dv| <= 2^-52 (|v| + |dtfm f|), |dx| <= 2^-52 (|x| + |dt v'|) + dt * the bar of v."""
    nall, x, v, f, mt = nve_case(n)
    xd, vd, fd, mtd = to_dev(x, dev), to_dev(v, dev), to_dev(f, dev), to_dev(mt, dev, np.int32)
    if which == "first":
        m.nve_first_dev(n, nall, xd.data_ptr(), vd.data_ptr(), fd.data_ptr(), mtd.data_ptr(), MASSES, DT, FTM2V)
    else:
        m.nve_dev(which, n, xd.data_ptr(), vd.data_ptr(), fd.data_ptr(), mtd.data_ptr(), MASSES, DT, FTM2V)
    sync(dev)
    x1, v1, f1 = xd.cpu().numpy(), vd.cpu().numpy(), fd.cpu().numpy()
    dtfm = ((0.5 * DT * FTM2V) * (1.0 / np.asarray(MASSES)))[mt[:n], None]
    vref = v[:n] + dtfm * f[:n]
    vbar = U52 * (np.abs(v[:n]) + np.abs(dtfm * f[:n]))
    assert np.all(np.abs(v1[:n] - vref) <= vbar)
    assert np.abs(vref - v[:n]).min() > 0, "the force moved every velocity"
    if which == 1:
        np.testing.assert_array_equal(x1, x)
    else:
        xref = x[:n] + DT * vref
        assert np.all(np.abs(x1[:n] - xref) <= U52 * (np.abs(x[:n]) + np.abs(DT * vref)) + DT * vbar)
    np.testing.assert_array_equal(x1[n:], x[n:])             # ghosts and the guard row
    np.testing.assert_array_equal(v1[n:], v[n:])
    if which == "first":
        assert np.all(f1[:nall] == 0.0), "nve_first zeroes every row of f, ghosts included"
        np.testing.assert_array_equal(f1[nall], f[nall])
    else:
        np.testing.assert_array_equal(f1, f)


# ------------------------------------------------------------------------------------------------ one-rank exchange plan
def check_local_plan(lib, dev):
    """4096 ghosts, 1000 of them images of one row (the atomics of k_comm_scatter_local contend): forward is exact, reverse within
    (images of the row) * 2^-53 * sum|f| per component (that many additions, each rounding a partial sum)"""
    rng = np.random.default_rng(66)
    nl, ng = 600, 4096
    src = rng.integers(0, nl, size=ng).astype(np.int64)
    src[rng.permutation(ng)[:1000]] = 17
    shift = rng.integers(-1, 2, size=(ng, 3)).astype(np.float64) * np.array([17.3, 11.1, 26.0])
    x = rng.uniform(0, 30, size=(nl + ng + 1, 3))
    x[nl + ng] = SENTINEL
    f = rng.normal(0, 1.0, size=(nl + ng + 1, 3))
    f[nl + ng] = SENTINEL
    srcd, shd, xd, fd = to_dev(src, dev, np.int64), to_dev(shift, dev), to_dev(x, dev), to_dev(f, dev)
    comm = capi.Comm(lib, 0, 1)
    comm.set_plan_local(nl, ng, srcd.data_ptr(), shd.data_ptr())
    comm.forward(xd.data_ptr())
    comm.reverse(fd.data_ptr())
    sync(dev)
    x1, f1 = xd.cpu().numpy(), fd.cpu().numpy()
    comm.close()
    np.testing.assert_array_equal(x1[:nl], x[:nl])
    np.testing.assert_array_equal(x1[nl: nl + ng], x[src] + shift)
    np.testing.assert_array_equal(x1[nl + ng], x[nl + ng])
    ref = f[:nl].astype(np.longdouble)
    np.add.at(ref, src, f[nl: nl + ng].astype(np.longdouble))
    mag = np.abs(f[:nl])
    np.add.at(mag, src, np.abs(f[nl: nl + ng]))
    images = np.bincount(src, minlength=nl)
    assert images[17] >= 1000
    assert np.all(np.abs(f1[:nl] - ref) <= (images[:, None] * 2.0 ** -53) * mag)
    np.testing.assert_array_equal(f1[nl:], f[nl:])           # the ghost rows and the guard row keep their contents
