"""The brick decomposition of ANY cell (csrc/comm.hip: ahip_comm_migrate_cell, ahip_comm_borders_cell, then ahip_comm_forward / ahip_comm_reverse on the plan
borders installed) with every rank of a grid in one process: cases, numpy references and checks of tests/test_comm_cell_ranks.py.  Transport, baton and the
reverse bound come from tests/comm_rank_cases.py.

Cells (rows = lattice vectors), rc = 5:
  P = [[32,0,0],[8,32,0],[0,0,16]]   dyadic, so cell^-1 and every s = x . cell^-1 are exact; m_b = 5/32 and m_c = 5/16 are exact, m_a is not
  Q = [[32,0,0],[8,32,0],[4,8,16]]   tilted on all three axes, still dyadic; only m_c is exact
  R = Q rotated by a fixed general rotation: nothing exact
Atoms are drawn in fractional coordinates on the grid of multiples of UF = 2^-14; on P and Q (entries multiples of 4) the Cartesian coordinates are then multiples
of 2^-12, on R they are rounded to that.  An axis is EXACT when m_d is exact and its grid is 1, 2 or 4: there atoms sit exactly on the decision planes.  Everywhere
else check_inputs asserts |s_d - plane| > 2^-30 for every atom, every image and every plane, which makes every decision independent of rounding and of FMA
contraction (the library's s is an fma chain, numpy's a matrix product).  mtype carries the atom's global id, so every ghost row names its owner."""
import itertools

import numpy as np

import comm_rank_cases as cr
from comm_rank_cases import RC, SENTINEL, U, run_ranks, sync, to_dev
from pair_allegro_amd import capi

UF = 2.0 ** -14
NF = 2 ** 14
GAP = 2.0 ** -30


def _rotation():
    q, r = np.linalg.qr(np.random.RandomState(11).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


P = np.array([[32.0, 0, 0], [8, 32, 0], [0, 0, 16]])
Q = np.array([[32.0, 0, 0], [8, 32, 0], [4, 8, 16]])
CELLS = {"P": P, "Q": Q, "R": Q @ _rotation()}
EXACT_M = {"P": (1, 2), "Q": (2,), "R": ()}            # axes whose m_d is exact

# name -> (cell, grid, pbc, kind)
CASES = {
    "P_one": ("P", (1, 1, 1), (1, 1, 1), "gas"),
    "Q_one": ("Q", (1, 1, 1), (1, 1, 1), "gas"),
    "R_one": ("R", (1, 1, 1), (1, 1, 1), "gas"),
    "P_x2": ("P", (2, 1, 1), (1, 1, 1), "gas"),
    "P_x3": ("P", (3, 1, 1), (1, 1, 1), "gas"),
    "P_x4": ("P", (4, 1, 1), (1, 1, 1), "gas"),
    "P_y2": ("P", (1, 2, 1), (1, 1, 1), "gas"),
    "P_z3": ("P", (1, 1, 3), (1, 1, 1), "gas"),
    "P_x3y2": ("P", (3, 2, 1), (1, 1, 1), "gas"),
    "Q_x2y2z2": ("Q", (2, 2, 2), (1, 1, 1), "gas"),
    "Q_x3y3": ("Q", (3, 3, 1), (1, 1, 1), "gas"),
    "R_x3y2": ("R", (3, 2, 1), (1, 1, 1), "gas"),
    "P_z2_open_z": ("P", (1, 1, 2), (1, 1, 0), "gas"),
    "P_z3_open_z": ("P", (1, 1, 3), (1, 1, 0), "gas"),
    "P_x3_open_x": ("P", (3, 1, 1), (0, 1, 1), "outside"),
    "P_x3_empty": ("P", (3, 1, 1), (1, 1, 1), "empty"),
    "P_x3_single": ("P", (3, 1, 1), (1, 1, 1), "single"),
    "P_x3_big": ("P", (3, 1, 1), (1, 1, 1), "big"),
}
ONE_RANK = ["P_one", "Q_one", "R_one"]
GRID_CASES = [n for n in CASES if n not in ONE_RANK]
MIGRATION_CASES = ["P_x3", "P_y2", "P_x3y2", "Q_x2y2z2", "Q_x3y3", "R_x3y2", "P_z2_open_z", "P_x3_open_x", "P_x3_big"]


def geometry(cell, rc=RC):
    """cell^-1 and m_d = rc / h_d, operation for operation as cell_geometry (csrc/cell_geom.h) computes them"""
    a, b, c = cell
    cr_ = [np.array([b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]]),
           np.array([c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]]),
           np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])]
    det = a[0] * cr_[0][0] + a[1] * cr_[0][1] + a[2] * cr_[0][2]
    inv = np.zeros((3, 3))
    m = np.zeros(3)
    for d in range(3):
        inv[:, d] = cr_[d] / det
        m[d] = rc * np.sqrt((cr_[d][0] * cr_[d][0] + cr_[d][1] * cr_[d][1]) + cr_[d][2] * cr_[d][2]) / abs(det)
    return inv, m


class CellCase:
    """Atoms of every rank of one grid on one cell: x [N][3] (the global id is the row), owner [N], owned[r] = ids of rank r in the order the rank holds them."""

    def __init__(self, name):
        cellname, grid, pbc, kind = CASES[name]
        self.name, self.cellname, self.grid, self.kind = name, cellname, tuple(grid), kind
        self.pbc = tuple(pbc)
        self.cell = CELLS[cellname].copy()
        self.inv, self.m = geometry(self.cell)
        self.coords = cr.coords_of(grid)
        self.n = len(self.coords)
        self.exact = [d in EXACT_M[cellname] and grid[d] in (1, 2, 4) for d in range(3)]
        for d in range(3):
            assert self.m[d] * grid[d] <= 1.0
        rng = np.random.default_rng(2000 + sorted(CASES).index(name))
        parts = []
        for r, c in enumerate(self.coords):
            k = self._atoms_of(rng, r, np.array(c))
            parts.append(k[rng.permutation(len(k))] if len(k) else k)
        sk = np.concatenate(parts)                                   # fractional coordinates in units of UF
        x = (sk * UF) @ self.cell
        if cellname == "R":
            x = np.round(x / U) * U
        assert np.all(x == np.round(x / U) * U), "every coordinate is a multiple of 2^-12"
        self.x = x
        self.owner = self.brick_of(self.frac(x))
        if cellname != "R":
            assert np.array_equal(self.owner, np.concatenate([np.full(len(p), r) for r, p in enumerate(parts)])), "an atom was placed outside its brick"
        self.owned = [np.nonzero(self.owner == r)[0] for r in range(self.n)]
        self.move = rng.integers(0, int(0.25 / U), size=self.x.shape) * U            # forward test: every owned position moves by less than 0.25

    # -- the rules of include/allegro_hip.h, in numpy
    def frac(self, x):
        return x @ self.inv

    def bounds(self, coord):
        g = np.array(self.grid, dtype=np.float64)
        return np.asarray(coord, dtype=np.float64) / g, (np.asarray(coord, dtype=np.float64) + 1.0) / g

    def brick_of(self, s):
        g = np.array(self.grid)
        c = np.clip(np.floor(s * g), 0, g - 1).astype(np.int64)
        return (c[:, 0] * g[1] + c[:, 1]) * g[2] + c[:, 2]

    def rank_of(self, c):
        return (c[0] * self.grid[1] + c[1]) * self.grid[2] + c[2]

    def neighbour(self, coord, d, step):
        """(rank, +1 / -1 / 0: the lattice vector a_d times this is added to what is sent there, open: the step crosses the face of an open axis)"""
        c = list(coord)
        c[d] += step
        wraps = 0
        if c[d] < 0:
            c[d] += self.grid[d]; wraps = +1
        elif c[d] >= self.grid[d]:
            c[d] -= self.grid[d]; wraps = -1
        return self.rank_of(c), wraps, bool(wraps) and not self.pbc[d]

    def wrap(self, x):
        """cell_wrap_row: periodic axes only, an atom already inside untouched"""
        k = np.where(np.array(self.pbc, dtype=bool), -np.floor(self.frac(x)), 0.0)
        out = x + ((k[:, 0:1] * self.cell[0] + k[:, 1:2] * self.cell[1]) + k[:, 2:3] * self.cell[2])
        return np.where((k == 0.0).all(axis=1)[:, None], x, out)

    # -- atoms, as integers k with s = k * UF
    def _krange(self, coord, d):
        g = self.grid[d]
        return -(-int(coord[d]) * NF // g), -(-(int(coord[d]) + 1) * NF // g)            # ceil(lo * NF), ceil(hi * NF): k * UF in [lo, hi)

    def _gas(self, rng, coord, n):
        return np.stack([rng.integers(*self._krange(coord, d), size=n) for d in range(3)], axis=1)

    def _planes(self, rng, coord):
        """per EXACT axis: lo, hi - u, lo + m (not in the lower slab), lo + m - u (in it), hi - m (in the upper slab), hi - m - u (not), and both cell faces"""
        rows = []
        for d in range(3):
            if not self.exact[d]:
                continue
            klo, khi = self._krange(coord, d)
            km = int(round(self.m[d] * NF))
            assert km * UF == self.m[d] and klo * self.grid[d] == coord[d] * NF
            vals = [klo, khi - 1, klo + km, klo + km - 1, khi - km, khi - km - 1]
            if coord[d] == 0:
                vals.append(0)
            if coord[d] == self.grid[d] - 1:
                vals.append(NF - 1)
            p = self._gas(rng, coord, len(vals))
            p[:, d] = vals
            rows.append(p)
        return np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int64)

    def _atoms_of(self, rng, r, coord):
        if self.kind == "single":              # one atom per rank: in the lower slab of a / in neither / on the last plane below hi; all in the lower slabs of b and c (corner images)
            klo, khi = self._krange(coord, 0)
            return np.array([[[klo + 300, klo + 2731, khi - 1][r], 100 + r, NF // 8]])
        if self.kind == "empty" and r > 0:
            return np.zeros((0, 3), dtype=np.int64)
        planes = self._planes(rng, coord)
        n = 9000 - len(planes) if self.kind == "big" else int(rng.integers(30, 95))
        while n % 32 == 0 or (n + len(planes)) % 32 == 0:
            n -= 1
        g = self._gas(rng, coord, n)
        if self.kind == "empty":               # near both a faces of brick 0
            klo, khi = self._krange(coord, 0)
            g[:, 0] = np.where(rng.integers(0, 2, size=n) == 0, klo + rng.integers(0, 1500, size=n), khi - 1 - rng.integers(0, 1500, size=n))
        if self.kind == "outside":             # open a axis: atoms beyond both cell faces, by less than m_a (so that the slab rule of the set check covers them)
            far = int(0.9 * self.m[0] * NF)
            if coord[0] == 0:
                g[:6, 0] = -rng.integers(1, far, size=6)
            if coord[0] == self.grid[0] - 1:
                g[:6, 0] = NF + rng.integers(0, far, size=6)
        return np.concatenate([g, planes])


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = CellCase(name)
    return _cases[name]


def images(cs):
    return [n for n in itertools.product((-1, 0, 1), repeat=3) if all(n[d] == 0 or cs.pbc[d] for d in range(3))]


def planes_of(cs, d):
    """every decision plane along d of every brick that is NOT exact: brick faces (exact on a dyadic cell where c / g is a dyadic number: always with 1, 2 or 4
    bricks, and the cell faces 0 and 1 with any), slab cuts and the outer edges of the ghost shell (exact when m_d is exact as well)"""
    out = []
    for c in range(cs.grid[d]):
        lo, hi = c / cs.grid[d], (c + 1) / cs.grid[d]
        out += [f for k, f in ((c, lo), (c + 1, hi)) if cs.cellname == "R" or (k * NF) % cs.grid[d] != 0]
        if not cs.exact[d]:
            out += [lo + cs.m[d], hi - cs.m[d], lo - cs.m[d], hi + cs.m[d]]
    return np.array(out)


def check_planes(cs, x, what):
    """either the plane is exact (then so is every s, and an atom on it is there by construction) or |s_d - plane| > 2^-30: for every atom and every image"""
    worst = np.inf
    for n in images(cs):
        s = cs.frac(x + np.array(n, dtype=np.float64) @ cs.cell)
        for d in range(3):
            if len(planes_of(cs, d)) == 0:
                continue
            gap = np.abs(s[:, d, None] - planes_of(cs, d)[None, :]).min()
            worst = min(worst, gap)
            assert gap > GAP, f"{cs.name}, {what}: an atom lies within 2^-30 ({gap:.3e}) of a decision plane of axis {d}, image {n}"
    return worst


def check_inputs(cs):
    gap = check_planes(cs, cs.x, "positions")
    if cs.cellname != "R":                       # dyadic: s is exact, so x -> s -> x comes back bit for bit
        s = cs.frac(cs.x)
        assert np.array_equal(s @ cs.cell, cs.x) and np.array_equal(s, np.round(s / UF) * UF)
    for d in range(3):
        if cs.exact[d] and cs.kind in ("gas", "outside", "big"):
            for r, c in enumerate(cs.coords):
                lo, hi = cs.bounds(c)
                v = set(cs.frac(cs.x[cs.owned[r]])[:, d].tolist())
                want = {lo[d], hi[d] - UF, lo[d] + cs.m[d], lo[d] + cs.m[d] - UF, hi[d] - cs.m[d], hi[d] - cs.m[d] - UF}
                assert want <= v, (cs.name, r, d, want - v)
    if cs.kind in ("gas", "outside"):
        assert all(30 <= len(o) <= 100 + 24 and len(o) % 32 != 0 for o in cs.owned), [len(o) for o in cs.owned]
    if cs.kind == "outside":
        sa = cs.frac(cs.x)[:, 0]
        assert np.any(sa < 0) and np.any(sa >= 1), "atoms beyond both faces of the open axis"
    return gap


# ------------------------------------------------------------------------------------------------ borders: the two references
def brute_force_rows(cs, rank):
    """(a) the SET: images x + n . cell, n in {-1, 0, 1}^3 (0 on open axes), with lo_d - m_d <= s_d < hi_d + m_d on every axis, the owned atoms excluded.
    Returns (ids, n, positions)."""
    lo, hi = cs.bounds(cs.coords[rank])
    ids, ns, pos = [], [], []
    for n in images(cs):
        xs = cs.x + np.array(n, dtype=np.float64) @ cs.cell
        s = cs.frac(xs)
        inside = np.all((s >= lo - cs.m) & (s < hi + cs.m), axis=1)
        if n == (0, 0, 0):
            inside &= cs.owner != rank
        k = np.nonzero(inside)[0]
        ids.append(k); ns.append(np.tile(np.array(n), (len(k), 1))); pos.append(xs[k])
    return np.concatenate(ids), np.concatenate(ns), np.concatenate(pos)


def shifted(cs, x, n):
    """x + n . cell as the swap chain adds it: one lattice vector per dimension, in dimension order, nothing added where n_d = 0"""
    out = x.copy()
    for d in range(3):
        k = n[:, d] != 0
        out[k] = out[k] + n[k, d, None].astype(np.float64) * cs.cell[d]
    return out


def swap_chain_rows(cs):
    """(b) the ORDER, in fractional coordinates.  Per dimension, over the rows known before it: lower list (s_d < lo_d + m_d) and upper list (s_d >= hi_d - m_d) in
    ascending row order, s from the row's current Cartesian position, go to the rank below / above, with +a_d / -a_d added where the step wraps and nothing sent
    across the face of an open axis; appended is first what came from above, then what came from below.  Returns per rank (ids, n, positions), owned first."""
    ids = [o.copy() for o in cs.owned]
    ns = [np.zeros((len(o), 3), dtype=np.int64) for o in cs.owned]
    pos = [cs.x[o].copy() for o in cs.owned]
    for d in range(3):
        out = []
        for r, c in enumerate(cs.coords):
            lo, hi = cs.bounds(c)
            s = cs.frac(pos[r])[:, d]
            lists = []
            for q, mask in enumerate((s < lo[d] + cs.m[d], s >= hi[d] - cs.m[d])):
                _, wraps, open_face = cs.neighbour(c, d, -1 if q == 0 else +1)
                if open_face:
                    mask = np.zeros_like(mask)
                p, nn = pos[r][mask].copy(), ns[r][mask].copy()
                if wraps:
                    p = p + float(wraps) * cs.cell[d]
                    nn[:, d] += wraps
                lists.append((ids[r][mask], nn, p))
            out.append(lists)
        for r, c in enumerate(cs.coords):
            above, below = cs.neighbour(c, d, +1)[0], cs.neighbour(c, d, -1)[0]
            ids[r] = np.concatenate([ids[r], out[above][0][0], out[below][1][0]])
            ns[r] = np.concatenate([ns[r], out[above][0][1], out[below][1][1]])
            pos[r] = np.concatenate([pos[r], out[above][0][2], out[below][1][2]])
    return list(zip(ids, ns, pos))


_refs = {}


def references(name):
    if name not in _refs:
        cs = case(name)
        _refs[name] = ([brute_force_rows(cs, r) for r in range(cs.n)], swap_chain_rows(cs))
    return _refs[name]


# ------------------------------------------------------------------------------------------------ one library run per case and backend
def borders_call(cs, comm, nl, x, mt, cap, coord):
    return comm.borders_cell(nl, x.data_ptr(), mt.data_ptr(), cap, cs.cell, cs.pbc, RC, cs.grid, coord)


def exchange_rank_fn(cs, dev, caps, borders=borders_call):
    """rank function: borders, then forward on moved positions, then reverse on random forces -- all on the plan that borders installed"""
    def fn(rank, coord, comm):
        own = cs.owned[rank]
        nl, cap = len(own), caps[rank]
        xh = np.full((cap + 1, 3), SENTINEL)
        xh[:nl] = cs.x[own]
        mh = np.full(cap + 1, -7, dtype=np.int32)
        mh[:nl] = own
        x, mt = to_dev(xh, dev), to_dev(mh, dev, np.int32)
        nall = borders(cs, comm, nl, x, mt, cap, coord)
        sync(dev)
        out = {"nlocal": nl, "nall": nall, "cap": cap, "x": x.cpu().numpy().copy(), "id": mt.cpu().numpy().copy(), "sent_borders": [list(g) for g in comm.sent]}
        if nall > cap:
            return out
        x[:nl] += to_dev(cs.move[own], dev)
        n0 = len(comm.sent)
        comm.forward(x.data_ptr())
        sync(dev)
        out["x_fwd"] = x.cpu().numpy().copy()
        out["sent_forward"] = [list(g) for g in comm.sent[n0:]]
        fh = np.random.default_rng(77 + rank).normal(0.0, 1.0, size=(nall + 1, 3))
        fh[nall] = SENTINEL
        f = to_dev(fh, dev)
        n0 = len(comm.sent)
        comm.reverse(f.data_ptr())
        sync(dev)
        out["f_in"], out["f_out"] = fh, f.cpu().numpy().copy()
        out["sent_reverse"] = [list(g) for g in comm.sent[n0:]]
        return out
    return fn


_runs = {}


def exchange_run(lib, dev, name):
    """borders_cell + forward + reverse of a case on one backend, run once and shared by the tests (nobody changes the result); capacity = brute-force count + 3"""
    key = (dev.type, name)
    if key not in _runs:
        cs = case(name)
        brute, _ = references(name)
        caps = [len(cs.owned[r]) + len(brute[r][0]) + 3 for r in range(cs.n)]
        res = run_ranks(cs.grid, exchange_rank_fn(cs, dev, caps), lib, dev)
        print(f"\n{name} on {dev.type}: cell {cs.cellname}, grid {cs.grid}, pbc {cs.pbc}")
        for r, o in enumerate(res):
            nmsg = sum(len(g) for k in ("sent_borders", "sent_forward", "sent_reverse") for g in o.get(k, []))
            print(f"  rank {r}: {o['nlocal']} owned rows, {o['nall'] - o['nlocal']} ghost rows, {nmsg} messages sent ({sum(len(g) for g in o['sent_borders'])} in borders)")
        _runs[key] = res
    return _runs[key]


def recover_n(cs, ids, xg):
    """the image of every ghost row: (x_ghost - x_owner) . cell^-1, rounded"""
    t = (xg - cs.x[ids]) @ cs.inv
    n = np.rint(t)
    assert np.abs(t - n).max(initial=0.0) < 1e-9
    return n.astype(np.int64)


def sorted_idn(ids, n, pos):
    a = np.concatenate([np.asarray(ids, dtype=np.float64)[:, None], n.astype(np.float64), pos], axis=1)
    return a[np.lexsort(a[:, :4].T[::-1])]


# ------------------------------------------------------------------------------------------------ borders checks
def check_borders_set(cs, res, brute):
    """dyadic cells: the multiset of (id, x, y, z) bit for bit.  R: by (id, n), n recovered from the row; positions within 3 * 2^-52 * max|x| (the brute force adds
    n . cell as one product, the library one lattice vector per dimension: at most three roundings of a number no larger than max|x| apart)"""
    for r, o in enumerate(res):
        nl, nall = o["nlocal"], o["nall"]
        bid, bn, bpos = brute[r]
        assert nall <= o["cap"], f"rank {r}: the library asks for {nall} rows, brute force counts {nl + len(bid)}"
        np.testing.assert_array_equal(o["x"][:nl], cs.x[cs.owned[r]], err_msg=f"rank {r}: owned rows")
        np.testing.assert_array_equal(o["id"][:nl], cs.owned[r], err_msg=f"rank {r}: owned ids")
        assert nall - nl == len(bid), f"rank {r}: {nall - nl} ghost rows, brute force has {len(bid)}"
        gid, gx = o["id"][nl:nall], o["x"][nl:nall]
        if cs.cellname != "R":
            np.testing.assert_array_equal(cr.sorted_rows(gid, gx), cr.sorted_rows(bid, bpos), err_msg=f"rank {r}: ghost multiset (id, x, y, z)")
        else:
            a, b = sorted_idn(gid, recover_n(cs, gid, gx), gx), sorted_idn(bid, bn, bpos)
            np.testing.assert_array_equal(a[:, :4], b[:, :4], err_msg=f"rank {r}: ghost multiset (id, n)")
            tol = 3 * 2.0 ** -52 * max(np.abs(a[:, 4:]).max(initial=0.0), np.abs(b[:, 4:]).max(initial=0.0))
            assert np.abs(a[:, 4:] - b[:, 4:]).max(initial=0.0) <= tol, f"rank {r}: ghost positions off by {np.abs(a[:, 4:] - b[:, 4:]).max():.3e} > {tol:.3e}"
        assert np.all(o["x"][nall:] == SENTINEL) and np.all(o["id"][nall:] == -7), f"rank {r}: rows behind the last ghost were written"


def check_borders_order(cs, res, chain):
    """on every cell bit for bit: the chain adds the lattice vectors in dimension order, as the library does"""
    for r, o in enumerate(res):
        ids, _, pos = chain[r]
        assert o["nall"] == len(ids), f"rank {r}: the library returns {o['nall']} rows, the chain has {len(ids)}"
        np.testing.assert_array_equal(o["id"][: o["nall"]], ids, err_msg=f"rank {r}: ids in row order")
        np.testing.assert_array_equal(o["x"][: o["nall"]], pos, err_msg=f"rank {r}: rows in order")


def open_pairs(cs):
    """pairs of ranks whose ONLY contact is across the face of an open axis (three or more bricks along it, equal coordinates elsewhere)"""
    out = set()
    for a, ca in enumerate(cs.coords):
        for b, cb in enumerate(cs.coords):
            d = cr.along(cs, a, b)
            if d >= 0 and not cs.pbc[d] and cs.grid[d] >= 3 and {ca[d], cb[d]} == {0, cs.grid[d] - 1}:
                out.add((a, b))
    return out


def check_messages(cs, res, keys, row_bytes):
    """what the transport counted: two separate payload messages to two peers in a dimension of three or more bricks (periodic), ONE merged payload message per
    group in a dimension of two bricks, and none at all -- payload or count -- between the two edge bricks of an open axis"""
    for key in keys:
        for d in range(3):
            if cs.grid[d] >= 3 and cs.pbc[d] and cs.kind not in ("empty", "single"):
                hits = [cr.two_message_groups(cs, r, o[key], d, row_bytes) for r, o in enumerate(res)]
                assert max(hits) >= 1, f"{key}, dimension {d}: no rank sent two separate messages ({hits})"
            if cs.grid[d] == 2:
                for r, o in enumerate(res):
                    for g in o[key]:
                        toward = [(p, nb) for p, nb in g if cr.along(cs, r, p) == d and nb >= row_bytes]
                        assert len(toward) <= 1, f"{key}, rank {r}, dimension {d}: {toward}"
        for r, o in enumerate(res):
            for g in o[key]:
                for p, nb in g:
                    assert (r, p) not in open_pairs(cs), f"{key}: rank {r} sent {nb} bytes to rank {p} across the face of an open axis"


# ------------------------------------------------------------------------------------------------ forward / reverse
def check_forward(cs, res, chain):
    """(f) each ghost equals its owner's NEW position plus its shift chain, exactly"""
    new = cs.x + cs.move
    for r, o in enumerate(res):
        nl, nall = o["nlocal"], o["nall"]
        ids, ns, _ = chain[r]
        np.testing.assert_array_equal(o["x_fwd"][:nl], new[cs.owned[r]], err_msg=f"rank {r}: owned rows changed")
        np.testing.assert_array_equal(o["x_fwd"][nl:nall], shifted(cs, new[ids[nl:]], ns[nl:]), err_msg=f"rank {r}: ghost rows after forward")
        assert np.all(o["x_fwd"][nall:] == SENTINEL), f"rank {r}: forward wrote behind the last ghost"
    assert np.abs(cs.move).max() > 0


# ------------------------------------------------------------------------------------------------ capacity protocol
def capacity_rank_fn(cs, dev, cap0, ncalls):
    def fn(rank, coord, comm):
        own = cs.owned[rank]
        nl = len(own)
        cap, answers = cap0, []
        for _ in range(ncalls):
            xh = np.full((max(cap, nl) + 1, 3), SENTINEL)
            xh[:nl] = cs.x[own]
            mh = np.full(max(cap, nl) + 1, -7, dtype=np.int32)
            mh[:nl] = own
            x, mt = to_dev(xh, dev), to_dev(mh, dev, np.int32)
            nall = borders_call(cs, comm, nl, x, mt, cap, coord)
            sync(dev)
            answers.append((cap, nall))
            if nall <= cap:
                return {"answers": answers, "x": x.cpu().numpy()[:nall].copy(), "id": mt.cpu().numpy()[:nall].copy()}
            cap = nall
        return {"answers": answers}
    return fn


def check_capacity_protocol(lib, dev, name="P_x3y2"):
    cs = case(name)
    brute, _ = references(name)
    need = [len(cs.owned[r]) + len(brute[r][0]) for r in range(cs.n)]
    cap0 = max(need) - 1
    direct = exchange_run(lib, dev, name)
    res = run_ranks(cs.grid, capacity_rank_fn(cs, dev, cap0, 4), lib, dev)
    print(f"\n{name}: needs {need}, first capacity {cap0}, answers of rank 0 {res[0]['answers']}")
    for r, o in enumerate(res):
        assert o["answers"][0][1] > cap0, "the first call must report an overflow"
        assert "x" in o, f"no fitting call within 4: {o['answers']}"
        assert o["answers"][:-1] == res[0]["answers"][:-1], f"overflow answers (capacity, answer) of rank {r}: {o['answers'][:-1]}, of rank 0: {res[0]['answers'][:-1]}"
        assert all(a > c for c, a in o["answers"][:-1])
        n = direct[r]["nall"]
        assert o["answers"][-1][1] == n
        np.testing.assert_array_equal(o["x"], direct[r]["x"][:n], err_msg=f"rank {r}")
        np.testing.assert_array_equal(o["id"], direct[r]["id"][:n], err_msg=f"rank {r}")


# ------------------------------------------------------------------------------------------------ migration
class Migration:
    """Displaced positions of a case and the numpy chain of what migrate_cell must leave behind.  Per decomposed dimension an atom stays, or moves one brick down /
    up (by floor(2^14 / g) grid planes, which is at most one brick height); atoms of rank 0 only stay or arrive, so some brick outgrows its array in the
    overflow test.  On an open axis the atoms of the edge bricks that move outwards leave [0, 1) and must stay, unwrapped.  By hand: atoms exactly on brick faces of
    exact axes and on both cell faces, and whole-cell jumps along axes that are not decomposed (the wrap alone)."""

    def __init__(self, cs):
        self.cs = cs
        rng = np.random.default_rng(6000 + sorted(CASES).index(cs.name))
        n = len(cs.x)
        s0 = cs.frac(cs.x)
        ks = s0 / UF                                   # (R: not integers; the displacement below is added in s all the same)
        dk = np.zeros((n, 3))
        cell0 = np.clip(np.floor(s0 * np.array(cs.grid)), 0, np.array(cs.grid) - 1).astype(np.int64)
        self.hand = {}
        used = np.zeros(n, dtype=bool)
        for d in range(3):
            g = cs.grid[d]
            if g == 1:
                if cs.pbc[d]:                          # the wrap alone: a few atoms one whole cell away
                    k = rng.choice(n, size=min(n, 6), replace=False)
                    dk[k, d] = rng.choice([-NF, NF], size=len(k))
                continue
            way = rng.choice([0, 0, -1, 1], size=n)
            way[cs.owner == 0] = 0
            dk[:, d] = way * (NF // g)
            if cs.exact[d] and cs.cellname != "R":     # exactly onto faces: the upper face of the own brick (belongs to the brick above; at the top brick it is the cell face), the own lower face
                for c in range(g):
                    cand = np.nonzero((cell0[:, d] == c) & ~used & (cs.owner != 0))[0]
                    if len(cand) >= 2:
                        a, b = cand[:2]
                        used[[a, b]] = True
                        dk[a, d] = (c + 1) * NF // g - ks[a, d]
                        dk[b, d] = c * NF // g - ks[b, d]
                        self.hand.setdefault("onto a face", []).extend([int(a), int(b)])
        self.x = cs.x + (dk * UF) @ cs.cell
        if cs.cellname == "R":
            self.x = np.round(self.x / U) * U
        self.v = np.stack([np.arange(n) + 0.25, -0.5 * np.arange(n) - 1.0, 1000.0 + np.arange(n) * 0.125], axis=1)
        self.tag = np.arange(n, dtype=np.int64) + 10 ** 6
        self.xw = cs.wrap(self.x)
        self.chain, self.lists, self.sizes = self._chain()

    def _chain(self):
        """wrap; per decomposed dimension keep / down / up from the brick index clamp(floor(s_d g), 0, g - 1) of the WRAPPED position: on a periodic axis delta =
        (brick - coord) mod g, g - 1 = down and wins, 1 = up; on an open axis brick - coord = -1 / +1 without the modulus.  New order: kept rows, then the down list
        of the upper neighbour, then the up list of the lower neighbour; nothing travels across the face of an open axis."""
        cs = self.cs
        sw = cs.frac(self.xw)
        ids = [o.copy() for o in cs.owned]
        lists, worst = {}, 0
        for d in range(3):
            g = cs.grid[d]
            if g == 1:
                continue
            parts = []
            for r, c in enumerate(cs.coords):
                cl = np.clip(np.floor(sw[ids[r], d] * g), 0, g - 1).astype(np.int64)
                if cs.pbc[d]:
                    delta = (cl - c[d]) % g
                    down = delta == g - 1
                    up = (delta == 1) & ~down
                else:
                    down, up = cl - c[d] == -1, cl - c[d] == 1
                parts.append((ids[r][~(down | up)], ids[r][down], ids[r][up]))
            lists[d] = [(len(p[1]), len(p[2])) for p in parts]
            for r, c in enumerate(cs.coords):
                above, _, open_up = cs.neighbour(c, d, +1)
                below, _, open_dn = cs.neighbour(c, d, -1)
                ids[r] = np.concatenate([parts[r][0], parts[above][1][:0] if open_up else parts[above][1], parts[below][2][:0] if open_dn else parts[below][2]])
                worst = max(worst, len(ids[r]))
        return ids, lists, worst


_migrations = {}


def migration(name):
    if name not in _migrations:
        _migrations[name] = Migration(case(name))
    return _migrations[name]


def check_migration_inputs(mg):
    cs = mg.cs
    check_planes(cs, mg.x, "displaced positions")
    check_planes(cs, mg.xw, "wrapped displaced positions")
    s, sw = cs.frac(mg.x), cs.frac(mg.xw)
    g = np.array(cs.grid)
    per = np.array(cs.pbc, dtype=bool)
    assert np.any(s[:, per] < 0) and np.any(s[:, per] >= 1), "atoms cross both cell faces on periodic axes"
    assert np.all((sw[:, per] >= 0) & (sw[:, per] < 1)), "the numpy wrap leaves an atom outside"
    cell0 = np.clip(np.floor(cs.frac(cs.x) * g), 0, g - 1)
    cell1 = np.clip(np.floor(sw * g), 0, g - 1)
    assert np.any(np.all(mg.x == cs.x, axis=1)), "atoms that do not move"
    if sum(k > 1 for k in cs.grid) >= 2:
        assert np.any((cell0 != cell1).sum(axis=1) >= 2), "atoms that change brick in two dimensions at once"
    if any(cs.exact[d] and cs.grid[d] > 1 for d in range(3)) and cs.cellname != "R":
        assert len(mg.hand.get("onto a face", [])) >= 2
        d = [d for d in range(3) if cs.exact[d] and cs.grid[d] > 1][0]
        faces = np.arange(cs.grid[d] + 1) / cs.grid[d]
        assert np.isin(s[mg.hand["onto a face"], d], faces).all()
    for d in range(3):
        if not cs.pbc[d] and cs.grid[d] > 1:
            out = (s[:, d] < 0) | (s[:, d] >= 1)
            assert np.any(out & (np.abs(mg.x - cs.x).max(axis=1) > 0)), f"nobody leaves [0, 1) on the open axis {d}"
            assert np.allclose(sw[out, d], s[out, d], rtol=0, atol=1e-12), "the numpy wrap moved an atom along an open axis"
    for d in cr.distinct_peer_dims(cs):
        if cs.pbc[d]:
            assert any(dn > 0 and up > 0 for dn, up in mg.lists[d]), f"dimension {d}: no rank has both a down and an up list ({mg.lists[d]})"


def migration_rank_fn(mg, dev, cap):
    cs = mg.cs

    def fn(rank, coord, comm):
        own = cs.owned[rank]
        nl = len(own)

        def arr(src, fill, dtype, cols=None):
            a = np.full((cap + 1,) + ((cols,) if cols else ()), fill, dtype=dtype)
            a[:nl] = src[own]
            return to_dev(a, dev, dtype)

        x, v = arr(mg.x, SENTINEL, np.float64, 3), arr(mg.v, SENTINEL, np.float64, 3)
        tag, mt = arr(mg.tag, -7, np.int64), arr(np.arange(len(cs.x)), -7, np.int32)
        nn = comm.migrate_cell(nl, x.data_ptr(), v.data_ptr(), tag.data_ptr(), mt.data_ptr(), cap, cs.cell, cs.pbc, cs.grid, coord)
        sync(dev)
        return {"n": nn, "x": x.cpu().numpy(), "v": v.cpu().numpy(), "tag": tag.cpu().numpy(), "id": mt.cpu().numpy(), "sent": [list(g) for g in comm.sent]}
    return fn


def check_migration(lib, dev, name):
    mg = migration(name)
    cs = mg.cs
    check_migration_inputs(mg)
    res = run_ranks(cs.grid, migration_rank_fn(mg, dev, mg.sizes + 5), lib, dev)
    print(f"\n{name} on {dev.type}: (down, up) list lengths per rank {mg.lists}")
    for r, o in enumerate(res):
        print(f"  rank {r}: {len(cs.owned[r])} -> {o['n']} owned rows, {sum(len(g) for g in o['sent'])} messages sent")
    # R: the wrap adds k . cell as products the compiler may contract; within 8 * 2^-53 * (|x| + sum |k_j a_j|), a bound of its four roundings.  Dyadic: exact.
    k = np.where(np.array(cs.pbc, dtype=bool), np.abs(np.floor(cs.frac(mg.x))), 0.0)
    tol = 8 * 2.0 ** -53 * (np.abs(mg.x) + k @ np.abs(cs.cell)) if cs.cellname == "R" else np.zeros_like(mg.x)
    for r, o in enumerate(res):
        ids = mg.chain[r]
        assert o["n"] == len(ids), f"rank {r}: {o['n']} owned atoms, the chain has {len(ids)}"
        n = o["n"]
        np.testing.assert_array_equal(o["id"][:n], ids, err_msg=f"rank {r}: mtype in order")
        np.testing.assert_array_equal(o["tag"][:n], mg.tag[ids], err_msg=f"rank {r}: tag")
        assert np.all(np.abs(o["x"][:n] - mg.xw[ids]) <= tol[ids]), f"rank {r}: wrapped x"
        np.testing.assert_array_equal(o["v"][:n], mg.v[ids], err_msg=f"rank {r}: v")
        untouched = np.all(mg.xw[ids] == mg.x[ids], axis=1)
        np.testing.assert_array_equal(o["x"][:n][untouched], mg.x[ids][untouched], err_msg=f"rank {r}: an atom already inside comes back bit for bit")
    # independent of the chain: nobody lost or doubled, everybody in the brick of its wrapped s
    everybody = np.concatenate([o["id"][: o["n"]] for o in res])
    np.testing.assert_array_equal(np.sort(everybody), np.arange(len(cs.x)), err_msg="every atom exactly once over all ranks")
    for r, o in enumerate(res):
        xr = o["x"][: o["n"]]
        np.testing.assert_array_equal(cs.brick_of(cs.frac(xr)), np.full(len(xr), r), err_msg=f"rank {r}: brick of the wrapped position")
        s = cs.frac(xr)
        per = np.array(cs.pbc, dtype=bool)
        assert np.all((s[:, per] >= 0) & (s[:, per] < 1)), f"rank {r}: a position outside the cell on a periodic axis"
    check_messages(cs, res, ["sent"], 64)
    for d in cr.distinct_peer_dims(cs):
        assert max(up for _, up in mg.lists[d]) > 0, f"dimension {d}: every up list is empty"


def check_migration_overflow(lib, dev, name):
    """a common capacity that the fullest brick exceeds by one row: every rank returns the same negative number of larger magnitude"""
    mg = migration(name)
    cs = mg.cs
    cap = mg.sizes - 1
    assert cap >= max(len(o) for o in cs.owned), "the capacity must hold what every rank starts with"
    res = run_ranks(cs.grid, migration_rank_fn(mg, dev, cap), lib, dev)
    answers = [o["n"] for o in res]
    print(f"\n{name}: capacity {cap}, answers {answers}")
    assert len(set(answers)) == 1 and answers[0] < 0 and -answers[0] > cap, answers


# ------------------------------------------------------------------------------------------------ refusals
REFUSALS = {
    # name: (cell, pbc, grid, word the message must hold)
    "thin brick": (P, (1, 1, 1), (1, 1, 4), "thinner than rc"),                                   # h_c / 4 = 4 < 5
    "singular cell": (np.array([[32.0, 0, 0], [8, 32, 0], [40, 32, 0]]), (1, 1, 1), (2, 1, 1), "singular"),
    "non-finite cell": (np.array([[32.0, 0, 0], [8, np.nan, 0], [0, 0, 16]]), (1, 1, 1), (2, 1, 1), "non-finite"),
    "thin periodic axis, one brick": (np.array([[32.0, 0, 0], [8, 32, 0], [0, 0, 4]]), (1, 1, 1), (2, 1, 1), "ahip_borders_cell_dev"),
}


def check_refusal(lib, dev, name):
    cell, pbc, grid, word = REFUSALS[name]

    def fn(rank, coord, comm):
        x = to_dev(np.full((16, 3), 1.0), dev)
        v = to_dev(np.zeros((16, 3)), dev)
        tag = to_dev(np.arange(16), dev, np.int64)
        mt = to_dev(np.zeros(16), dev, np.int32)
        out = {}
        try:
            comm.borders_cell(4, x.data_ptr(), mt.data_ptr(), 16, cell, pbc, RC, grid, coord)
            out["borders"] = None
        except capi.AhipError as e:
            out["borders"] = (e.code, e.msg)
        if "cell" in name:
            try:
                comm.migrate_cell(4, x.data_ptr(), v.data_ptr(), tag.data_ptr(), mt.data_ptr(), 16, cell, pbc, grid, coord)
                out["migrate"] = None
            except capi.AhipError as e:
                out["migrate"] = (e.code, e.msg)
        sync(dev)
        out["sent"] = [list(g) for g in comm.sent]
        out["x"] = x.cpu().numpy()
        return out

    res = run_ranks(grid, fn, lib, dev)
    for r, o in enumerate(res):
        for key in ("borders", "migrate"):
            if key in o:
                assert o[key] is not None and o[key][0] == capi.AHIP_ERR_ARG, f"rank {r}, {key}: {o[key]}"
                assert word in o[key][1], o[key][1]
        assert o["sent"] == [], f"rank {r} sent {o['sent']}"
        assert np.all(o["x"] == 1.0)
