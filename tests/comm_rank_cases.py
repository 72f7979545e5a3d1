"""The spatial decomposition of csrc/comm.hip (ahip_comm_borders, ahip_comm_forward, ahip_comm_reverse, ahip_comm_migrate) with every rank of a grid inside
ONE process: transport, cases, references and checks of tests/test_comm_ranks.py, shared by the CPU twin (host-emulation build) and the MI355X.

Ranks are threads, and the BATON is what makes that legal.  Every rank of an N-rank grid is a Python thread that owns a capi.Comm with a hosted transfer
callback.  ctypes drops the GIL while a thread is inside the library, and the host emulation is single-threaded by design (tests/host_emu/hip/hip_runtime.h:
global threadIdx / blockIdx, kernels launched as loops), so two rank threads must never be inside library code at the same time.  Hence one lock, the baton:
  - a rank thread holds the baton for the whole of its rank function, in particular whenever it is inside a library call;
  - the transfer callback -- the only place where a rank has to wait for another -- reads what it has to send while it still holds the baton, RELEASES it, does
    its mailbox work (post every send of the group, then wait for the receives), takes the baton BACK and only then copies the received bytes in and returns;
  - the GPU run keeps the same discipline: it costs nothing, and a single thread drives the device at any time.
Do not "simplify" the baton away: without it the emulation's globals race and the results are garbage that looks like a kernel bug.

Every wait has a time limit (WAIT seconds; a condition, not a measurement): on expiry the callback raises, the library returns its "host transfer callback
failed" error, the rank thread records the exception and run_ranks re-raises the first one.  A protocol mismatch ends as a failed test, never as a hang.

Inputs make "exact" mean exact: rc = 5, integer box lengths that are a multiple of the brick count, every coordinate a multiple of 2^-12.  Then x + shift,
lo + rc, hi - rc, floor(x / width) and x - floor(x / b) * b (contracted to a fused multiply-add or not: the product is exact) are exact in float64, and every
comparison below is bit for bit unless a bound is stated.  mtype carries the atom's global id, so every ghost row names its owner."""
import ctypes
import itertools
import queue
import threading
import time

import numpy as np
import torch

from pair_allegro_amd import capi

RC = 5.0
U = 2.0 ** -12
WAIT = 30.0                      # time limit of every wait inside the transport
JOIN = 240.0                     # time limit for all rank threads of one run together
SENTINEL = -12345.678


# ------------------------------------------------------------------------------------------------ transport: ranks as threads
class Transport:
    """Mailboxes between the rank threads of one grid + the baton.  `groups[r]` logs, per callback group of rank r, its sends as (peer, bytes)."""

    def __init__(self, n, dev):
        self.n, self.dev = n, dev
        self.baton = threading.Lock()
        self.box = {(a, b): queue.Queue() for a in range(n) for b in range(n) if a != b}
        self.cv = threading.Condition()
        self.red, self.red_round = {}, [0] * n
        self.abort = threading.Event()
        self.errors = []
        self.groups = [[] for _ in range(n)]

    def fail(self, rank, exc):
        self.errors.append((rank, exc))
        self.abort.set()

    # raw memory the library handed to the callback: host memory in the emulation, device memory on the GPU (md.Simulation._tensor_at)
    def _view(self, ptr, nbytes):
        class _Mem:
            pass
        m = _Mem()
        m.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(m, device=self.dev)

    def _read(self, ptr, nbytes):
        if self.dev.type == "cuda":
            data = self._view(ptr, nbytes).cpu().numpy().tobytes()
            torch.cuda.synchronize()
            return data
        return ctypes.string_at(int(ptr), nbytes)

    def _write(self, ptr, data):
        if self.dev.type == "cuda":
            self._view(ptr, len(data)).copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
            torch.cuda.synchronize()
        else:
            ctypes.memmove(int(ptr), data, len(data))

    def _take(self, me, peer):
        end = time.monotonic() + WAIT
        while True:
            if self.abort.is_set():
                raise RuntimeError(f"rank {me}: another rank failed while this one waited for rank {peer}")
            try:
                return self.box[peer, me].get(timeout=0.02)
            except queue.Empty:
                if time.monotonic() > end:
                    raise TimeoutError(f"rank {me}: no message from rank {peer} within {WAIT} s")

    def _allreduce(self, me, kind, data):
        """kind 2: float64 sum taken in rank order; kind 3: int32 max.  The k-th all-reduce of every rank is one round."""
        end = time.monotonic() + WAIT
        with self.cv:
            k = self.red_round[me]
            self.red_round[me] += 1
            slot = self.red.setdefault(k, {})
            slot[me] = (kind, data)
            self.cv.notify_all()
            while len(slot) < self.n:
                if self.abort.is_set():
                    raise RuntimeError(f"rank {me}: another rank failed during all-reduce {k}")
                if time.monotonic() > end:
                    raise TimeoutError(f"rank {me}: all-reduce {k} has {len(slot)} of {self.n} ranks after {WAIT} s")
                self.cv.wait(0.02)
        assert {v[0] for v in slot.values()} == {kind} and {len(v[1]) for v in slot.values()} == {len(data)}, f"all-reduce {k}: the ranks disagree on kind or size"
        parts = [np.frombuffer(slot[r][1], dtype=np.float64 if kind == 2 else np.int32) for r in range(self.n)]
        acc = parts[0].copy()
        for p in parts[1:]:
            acc = acc + p if kind == 2 else np.maximum(acc, p)
        return acc.tobytes()

    def xfer(self, me, ops):
        """The hosted transfer callback of rank `me`: called from inside a library call, that is with the baton held."""
        try:
            sends = [(peer, self._read(ptr, nb)) for kind, peer, ptr, nb in ops if kind == 0]
            reds = [(kind, ptr, self._read(ptr, nb)) for kind, peer, ptr, nb in ops if kind >= 2]
            got = []
            self.baton.release()
            try:
                if sends:
                    self.groups[me].append([(peer, len(d)) for peer, d in sends])
                for peer, d in sends:                                      # every send of the group is posted before the first receive is waited for
                    self.box[me, peer].put(d)
                for kind, peer, ptr, nb in ops:
                    if kind == 1:
                        d = self._take(me, peer)
                        if len(d) != nb:
                            raise AssertionError(f"rank {me} expects {nb} bytes from rank {peer}, the next message has {len(d)}")
                        got.append((ptr, d))
                for kind, ptr, d in reds:
                    got.append((ptr, self._allreduce(me, kind, d)))
            finally:
                self.baton.acquire()
            for ptr, d in got:
                self._write(ptr, d)
        except BaseException as e:
            self.fail(me, e)
            raise


def coords_of(grid):
    """coordinate of every rank; rank of a coordinate is (cx * gy + cy) * gz + cz (rank_of in comm.hip)"""
    return [c for c in itertools.product(range(grid[0]), range(grid[1]), range(grid[2]))]


def run_ranks(grid, fn, lib, dev):
    """One thread per rank of `grid`; each creates its capi.Comm and calls fn(rank, coord, comm) under the baton.  comm.sent is the transport's log of the
    rank's send groups.  Returns the per-rank results; re-raises the first exception any rank recorded."""
    coords = coords_of(grid)
    n = len(coords)
    tr = Transport(n, dev)
    results = [None] * n

    def body(r):
        try:
            with tr.baton:
                comm = capi.Comm(lib, r, n, xfer=(lambda ops: tr.xfer(r, ops)) if n > 1 else None)
                comm.sent = tr.groups[r]
                try:
                    results[r] = fn(r, np.array(coords[r], dtype=np.int32), comm)
                finally:
                    comm.close()
        except BaseException as e:
            tr.fail(r, e)

    threads = [threading.Thread(target=body, args=(r,), daemon=True, name=f"rank{r}") for r in range(n)]
    for t in threads:
        t.start()
    end = time.monotonic() + JOIN
    for t in threads:
        t.join(max(0.0, end - time.monotonic()))
    if any(t.is_alive() for t in threads):
        tr.abort.set()
        raise TimeoutError(f"rank threads still running after {JOIN} s: {[t.name for t in threads if t.is_alive()]}")
    if tr.errors:
        raise tr.errors[0][1]
    return results


# ------------------------------------------------------------------------------------------------ cases
# name -> (grid, box, kind)
CASES = {
    "one": ((1, 1, 1), (16, 16, 16), "gas"),
    "x2": ((2, 1, 1), (16, 8, 8), "gas"),
    "x3": ((3, 1, 1), (24, 8, 8), "gas"),
    "x3_wide": ((3, 1, 1), (36, 12, 12), "gas"),
    "y3": ((1, 3, 1), (8, 24, 8), "gas"),
    "x4": ((4, 1, 1), (32, 8, 8), "gas"),
    "x3y2": ((3, 2, 1), (24, 16, 8), "gas"),
    "x3y3": ((3, 3, 1), (24, 24, 8), "gas"),
    "empty_bricks": ((3, 1, 1), (24, 8, 8), "empty"),
    "one_atom_each": ((3, 1, 1), (24, 8, 8), "single"),
    "block_boundary": ((3, 1, 1), (24, 8, 8), "big"),
}
MIGRATION_CASES = ["x2", "x3", "y3", "x4", "x3y2", "x3y3", "block_boundary"]


class Case:
    """Atoms of every rank of one grid: x [N][3] (the global id is the row), owner [N], owned[r] = ids of rank r in the order the rank holds them."""

    def __init__(self, name):
        grid, box, kind = CASES[name]
        self.name, self.grid, self.kind = name, tuple(grid), kind
        self.box = np.array(box, dtype=np.float64)
        self.width = self.box / np.array(grid)
        assert np.all(self.width == np.floor(self.width)) and np.all(self.width >= RC)
        self.coords = coords_of(grid)
        self.n = len(self.coords)
        rng = np.random.default_rng(1000 + sorted(CASES).index(name))
        xs, self.owned = [], []
        for r, c in enumerate(self.coords):
            xr = self._atoms_of(rng, r, np.array(c))
            xr = xr[rng.permutation(len(xr))] if len(xr) else xr
            self.owned.append(np.arange(len(xr)) + sum(len(a) for a in xs))
            xs.append(xr)
        self.x = np.concatenate(xs)
        assert np.all(self.x == np.round(self.x / U) * U), "every coordinate is a multiple of 2^-12"
        self.owner = np.concatenate([np.full(len(o), r) for r, o in enumerate(self.owned)]).astype(np.int64)
        cell = np.floor(self.x / self.width).astype(np.int64)
        assert np.array_equal((cell[:, 0] * grid[1] + cell[:, 1]) * grid[2] + cell[:, 2], self.owner), "an atom was placed outside its brick"
        self.move = rng.integers(0, int(0.25 / U), size=self.x.shape) * U            # forward test: every owned position moves by less than 0.25

    def brick(self, coord):
        lo = np.asarray(coord) * self.width
        return lo, lo + self.width

    def rank_of(self, c):
        return (c[0] * self.grid[1] + c[1]) * self.grid[2] + c[2]

    def neighbour(self, coord, d, step):
        """(rank, shift applied to what is sent there): neighbour() in comm.hip"""
        c = list(coord)
        c[d] += step
        shift = 0.0
        if c[d] < 0:
            c[d] += self.grid[d]; shift = self.box[d]
        elif c[d] >= self.grid[d]:
            c[d] -= self.grid[d]; shift = -self.box[d]
        return self.rank_of(c), shift

    def _gas(self, rng, lo, n):
        return lo + rng.integers(0, (self.width / U).astype(np.int64), size=(n, 3)) * U

    def _planes(self, rng, coord):
        """per dimension: lo, hi - u, lo + rc (not in the lower slab), lo + rc - u (in it), hi - rc (in the upper slab), hi - rc - u (not), 0, box - u"""
        lo, hi = self.brick(coord)
        rows = []
        for d in range(3):
            vals = [lo[d], hi[d] - U, lo[d] + RC, lo[d] + RC - U, hi[d] - RC, hi[d] - RC - U]
            if coord[d] == 0:
                vals.append(0.0)
            if coord[d] == self.grid[d] - 1:
                vals.append(self.box[d] - U)
            p = self._gas(rng, lo, len(vals))
            p[:, d] = vals
            rows.append(p)
        return np.concatenate(rows)

    def _atoms_of(self, rng, r, coord):
        lo, hi = self.brick(coord)
        if self.kind == "single":                 # one atom per rank: in the lower slab / in both slabs / on the last representable plane below hi
            return np.array([[[lo[0] + 1.0, lo[0] + 4.0, hi[0] - U][r], 4.0 + U * r, 4.0]])
        if self.kind == "empty" and r > 0:
            return np.zeros((0, 3))
        planes = self._planes(rng, coord)
        n = 9000 - len(planes) if self.kind == "big" else int(rng.integers(30, 101))
        while n % 32 == 0 or (n + len(planes)) % 32 == 0:
            n -= 1
        g = self._gas(rng, lo, n)
        if self.kind == "empty":                  # near both x faces of brick 0: [0, 2.5) and [5.5, 8)
            g[:, 0] = np.where(rng.integers(0, 2, size=n) == 0, 0.0, 5.5) + rng.integers(0, int(2.5 / U), size=n) * U
        return np.concatenate([g, planes])


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def to_dev(a, dev, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev)


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ borders: the two references
def brute_force_rows(cs, rank):
    """(a) the SET: images x + n * box, n in {-1, 0, 1}^3, of all atoms of all ranks inside [lo - rc, hi + rc) on every axis, the owned atoms themselves excluded.
    Follows from the slab rules (v < lo + rc, v >= hi - rc) whatever the order of the swaps.  Returns (ids, positions)."""
    lo, hi = cs.brick(cs.coords[rank])
    ids, pos = [], []
    for n in itertools.product((-1, 0, 1), repeat=3):
        xs = cs.x + np.array(n, dtype=np.float64) * cs.box
        inside = np.all((xs >= lo - RC) & (xs < hi + RC), axis=1)
        if n == (0, 0, 0):
            inside &= cs.owner != rank
        k = np.nonzero(inside)[0]
        ids.append(k)
        pos.append(xs[k])
    return np.concatenate(ids), np.concatenate(pos)


def swap_chain_rows(cs):
    """(b) the ORDER: the swap chain over all ranks at once.  Per dimension, over the rows known before it: lower list (v < lo + rc) and upper list (v >= hi - rc) in
    ascending row order go to the rank below / above, shifted by +-box where the step wraps; appended is first what came from above (the swap to the lower
    neighbour receives from the upper one), then what came from below.  Returns per rank (ids, positions) of all rows, owned first."""
    ids = [o.copy() for o in cs.owned]
    pos = [cs.x[o].copy() for o in cs.owned]
    for d in range(3):
        out = []                                                 # per rank: [(ids, shifted positions) of the lower list, ... of the upper list]
        for r, c in enumerate(cs.coords):
            lo, hi = cs.brick(c)
            v = pos[r][:, d]
            lists = []
            for q, mask in enumerate((v < lo[d] + RC, v >= hi[d] - RC)):
                _, shift = cs.neighbour(c, d, -1 if q == 0 else +1)
                p = pos[r][mask].copy()
                p[:, d] += shift
                lists.append((ids[r][mask], p))
            out.append(lists)
        for r, c in enumerate(cs.coords):
            above, _ = cs.neighbour(c, d, +1)
            below, _ = cs.neighbour(c, d, -1)
            ids[r] = np.concatenate([ids[r], out[above][0][0], out[below][1][0]])
            pos[r] = np.concatenate([pos[r], out[above][0][1], out[below][1][1]])
    return list(zip(ids, pos))


_refs = {}


def references(name):
    """brute-force rows and chain rows of every rank of a case, computed once"""
    if name not in _refs:
        cs = case(name)
        _refs[name] = ([brute_force_rows(cs, r) for r in range(cs.n)], swap_chain_rows(cs))
    return _refs[name]


def sorted_rows(ids, pos):
    a = np.concatenate([np.asarray(ids, dtype=np.float64)[:, None], pos], axis=1)
    return a[np.lexsort(a.T[::-1])]


# ------------------------------------------------------------------------------------------------ one library run per case and backend
def exchange_rank_fn(cs, dev, caps):
    """rank function: borders, then forward on moved positions, then reverse on random forces -- all on the plan that borders installed"""
    def fn(rank, coord, comm):
        own = cs.owned[rank]
        nl, cap = len(own), caps[rank]
        lo, hi = cs.brick(coord)
        xh = np.full((cap + 1, 3), SENTINEL)
        xh[:nl] = cs.x[own]
        mh = np.full(cap + 1, -7, dtype=np.int32)
        mh[:nl] = own
        x, mt = to_dev(xh, dev), to_dev(mh, dev, np.int32)
        nall = comm.borders(nl, x.data_ptr(), mt.data_ptr(), cap, lo, hi, cs.box, RC, cs.grid, coord)
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
    """the library's borders + forward + reverse of a case on one backend, run once and shared by the tests (nobody changes the result).  The capacity of a
    rank is the brute-force count + 3 rows: a library that wants more says so and the borders tests fail on the count."""
    key = (dev.type, name)
    if key not in _runs:
        cs = case(name)
        brute, _ = references(name)
        caps = [len(cs.owned[r]) + len(brute[r][0]) + 3 for r in range(cs.n)]
        res = run_ranks(cs.grid, exchange_rank_fn(cs, dev, caps), lib, dev)
        print(f"\n{name} on {dev.type}: grid {cs.grid}, box {tuple(cs.box)}")
        for r, o in enumerate(res):
            nmsg = sum(len(g) for k in ("sent_borders", "sent_forward", "sent_reverse") for g in o.get(k, []))
            print(f"  rank {r}: {o['nlocal']} owned rows, {o['nall'] - o['nlocal']} ghost rows, {nmsg} messages sent ({sum(len(g) for g in o['sent_borders'])} in borders)")
        _runs[key] = res
    return _runs[key]


def along(cs, me, peer):
    """the dimension in which the bricks of two ranks differ when they differ in exactly one, else -1"""
    diff = [d for d in range(3) if cs.coords[me][d] != cs.coords[peer][d]]
    return diff[0] if len(diff) == 1 else -1


def two_message_groups(cs, rank, groups, d, min_bytes):
    """send groups of one rank that hold two separate payload messages to two different peers along dimension d"""
    hit = 0
    for g in groups:
        peers = {peer for peer, nb in g if nb >= min_bytes and along(cs, rank, peer) == d}
        hit += len(peers) == 2
    return hit


def distinct_peer_dims(cs):
    return [d for d in range(3) if cs.grid[d] >= 3]


# ------------------------------------------------------------------------------------------------ borders checks
def check_borders_set(cs, res, brute):
    for r, o in enumerate(res):
        nl, nall = o["nlocal"], o["nall"]
        assert nall <= o["cap"], f"rank {r}: the library asks for {nall} rows, brute force counts {nl + len(brute[r][0])}"
        np.testing.assert_array_equal(o["x"][:nl], cs.x[cs.owned[r]], err_msg=f"rank {r}: owned rows")
        np.testing.assert_array_equal(o["id"][:nl], cs.owned[r], err_msg=f"rank {r}: owned ids")
        assert nall - nl == len(brute[r][0]), f"rank {r}: {nall - nl} ghost rows, brute force has {len(brute[r][0])}"
        np.testing.assert_array_equal(sorted_rows(o["id"][nl:nall], o["x"][nl:nall]), sorted_rows(*brute[r]), err_msg=f"rank {r}: ghost multiset (id, x, y, z)")
        assert np.all(o["x"][nall:] == SENTINEL) and np.all(o["id"][nall:] == -7), f"rank {r}: rows behind the last ghost were written"


def check_borders_order(cs, res, chain):
    for r, o in enumerate(res):
        ids, pos = chain[r]
        assert o["nall"] == len(ids), f"rank {r}: the library returns {o['nall']} rows, the chain has {len(ids)}"
        np.testing.assert_array_equal(o["id"][: o["nall"]], ids, err_msg=f"rank {r}: ids in row order")
        np.testing.assert_array_equal(o["x"][: o["nall"]], pos, err_msg=f"rank {r}: rows in order")


def check_borders_messages(cs, res):
    """what the transport counted: a dimension with three or more bricks sends two separate slab messages (28 bytes per row) to two peers from some rank"""
    for d in distinct_peer_dims(cs):
        hits = [two_message_groups(cs, r, o["sent_borders"], d, 28) for r, o in enumerate(res)]
        assert max(hits) >= 1, f"dimension {d}: no rank sent two separate border messages ({hits})"
    if cs.name == "x2":                                            # two bricks: the slabs of both swaps travel as ONE message per rank
        for r, o in enumerate(res):
            slabs = [g for g in o["sent_borders"] if any(nb >= 28 for _, nb in g)]
            assert [len(g) for g in slabs] == [1], f"rank {r}: {slabs}"


def slab_classes(cs, rank, d=0):
    """class per owned row of rank along d: 1 lower slab, 2 upper slab, 3 both, 0 neither (row_class(SlabCut))"""
    lo, hi = cs.brick(cs.coords[rank])
    v = cs.x[cs.owned[rank], d]
    return (v < lo[d] + RC).astype(int) | ((v >= hi[d] - RC).astype(int) << 1)


# ------------------------------------------------------------------------------------------------ forward / reverse checks
def check_forward(cs, res):
    new = cs.x + cs.move
    for r, o in enumerate(res):
        nl, nall = o["nlocal"], o["nall"]
        ids = o["id"][nl:nall]
        shift = o["x"][nl:nall] - cs.x[ids]                              # the ghost's own shift: its old position minus its owner's old position (exact)
        np.testing.assert_array_equal(o["x_fwd"][:nl], new[cs.owned[r]], err_msg=f"rank {r}: owned rows changed")
        np.testing.assert_array_equal(o["x_fwd"][nl:nall], new[ids] + shift, err_msg=f"rank {r}: ghost rows after forward")
        assert np.all(o["x_fwd"][nall:] == SENTINEL), f"rank {r}: forward wrote behind the last ghost"
    assert np.abs(cs.move).max() > 0


def check_reverse(cs, res):
    """owned row = longdouble sum of f over all rows of that atom on all ranks, within (rows of the atom) * 2^-53 * sum |f| per component: that many additions,
    spread over several hops, each rounding a partial sum no larger than sum |f| (the bound of driver_kernel_cases.check_local_plan)"""
    n = len(cs.x)
    ref = np.zeros((n, 3), dtype=np.longdouble)
    mag = np.zeros((n, 3))
    rows = np.zeros(n, dtype=np.int64)
    for o in res:
        ids = o["id"][: o["nall"]]
        np.add.at(ref, ids, o["f_in"][: o["nall"]].astype(np.longdouble))
        np.add.at(mag, ids, np.abs(o["f_in"][: o["nall"]]))
        rows += np.bincount(ids, minlength=n)
    assert rows.max() >= 4, "some atom has a corner image: k_comm_unpack_add adds more than once into one row"
    for r, o in enumerate(res):
        nl, nall = o["nlocal"], o["nall"]
        own = cs.owned[r]
        err = np.abs(o["f_out"][:nl].astype(np.longdouble) - ref[own])
        bound = (rows[own, None] * 2.0 ** -53) * mag[own]
        assert np.all(err <= bound), f"rank {r}: reverse misses the bound by up to {float((err - bound).max()):.3e} (row {int(np.argmax((err - bound).max(axis=1)))})"
        np.testing.assert_array_equal(o["f_out"][nall], o["f_in"][nall], err_msg=f"rank {r}: the row behind the last ghost")
    return int(rows.max())


def check_exchange_messages(cs, res):
    """forward and reverse take the per-swap remote branch: two separate 24-byte-per-row messages to two peers in every dimension with three or more bricks"""
    for d in distinct_peer_dims(cs):
        for key in ("sent_forward", "sent_reverse"):
            if key == "sent_reverse" and cs.kind == "empty":               # only brick 0 has ghosts elsewhere: ranks 1 and 2 return one message each, rank 0 none
                assert [sum(len(g) for g in o[key]) for o in res] == [0, 1, 1]
                continue
            hits = [two_message_groups(cs, r, o[key], d, 24) for r, o in enumerate(res)]
            assert max(hits) >= 1, f"{key}, dimension {d}: no rank sent two separate messages ({hits})"


# ------------------------------------------------------------------------------------------------ capacity protocol of borders
def capacity_rank_fn(cs, dev, cap0, ncalls):
    def fn(rank, coord, comm):
        own = cs.owned[rank]
        nl = len(own)
        lo, hi = cs.brick(coord)
        cap, answers = cap0, []
        for _ in range(ncalls):
            xh = np.full((max(cap, nl) + 1, 3), SENTINEL)
            xh[:nl] = cs.x[own]
            mh = np.full(max(cap, nl) + 1, -7, dtype=np.int32)
            mh[:nl] = own
            x, mt = to_dev(xh, dev), to_dev(mh, dev, np.int32)
            nall = comm.borders(nl, x.data_ptr(), mt.data_ptr(), cap, lo, hi, cs.box, RC, cs.grid, coord)
            sync(dev)
            answers.append((cap, nall))
            if nall <= cap:
                return {"answers": answers, "x": x.cpu().numpy()[:nall].copy(), "id": mt.cpu().numpy()[:nall].copy()}
            cap = nall
        return {"answers": answers}
    return fn


def check_capacity_protocol(lib, dev, name="x3y2"):
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
    """Displaced positions of a case (each atom by less than one brick width per decomposed dimension) and the numpy chain of what migrate must leave behind."""

    def __init__(self, cs):
        self.cs = cs
        rng = np.random.default_rng(5000 + sorted(CASES).index(cs.name))
        n = len(cs.x)
        xd = cs.x.copy()
        used = np.zeros(n, dtype=bool)
        cell = np.floor(cs.x / cs.width).astype(np.int64)
        self.hand = {}
        for d in range(3):
            g, w = cs.grid[d], cs.width[d]
            if g == 1:
                continue
            lo = cell[:, d] * w

            def pick(cond, what):
                k = np.nonzero(cond & ~used)[0]
                assert len(k), f"{cs.name}: no atom for '{what}' along {d}"
                used[k[0]] = True
                self.hand.setdefault(what, []).append(int(k[0]))
                return k[0]

            xd[pick((cell[:, d] == 0) & (cs.x[:, d] <= w / 2), "to -2^-12"), d] = -U                       # leaves the box downwards
            xd[pick((cell[:, d] == g - 1) & (cs.x[:, d] >= cs.box[d] - w / 2), "to box"), d] = cs.box[d]  # lands exactly on the upper box face
            for c in range(g - 1):
                xd[pick((cell[:, d] == c) & (cs.x[:, d] > lo), "onto the upper brick face"), d] = (c + 1) * w   # exactly on a face: belongs to the brick above
            for c in range(g):
                xd[pick(cell[:, d] == c, "onto the own lower face"), d] = c * w                                # exactly on its own lower face: stays
            # the gas: rank 0 keeps its atoms (it only gains, so some brick outgrows its array in the overflow test); elsewhere half stay, a quarter each goes one brick
            # down / up, to a uniformly drawn plane of the neighbour brick less than one brick width away
            free = np.nonzero(~used & (cs.owner != 0))[0]
            way = rng.choice([0, 0, -1, 1], size=len(free))
            off = np.round((cs.x[free, d] - lo[free]) / U).astype(np.int64)          # planes between the atom and its lower face
            room_up, room_dn = off, np.round(w / U).astype(np.int64) - off - 1
            up = free[(way == 1) & (room_up > 0)]
            dn = free[(way == -1) & (room_dn > 0)]
            xd[up, d] = lo[up] + w + rng.integers(0, room_up[(way == 1) & (room_up > 0)]) * U
            xd[dn, d] = lo[dn] - U * (1 + rng.integers(0, room_dn[(way == -1) & (room_dn > 0)]))
            assert np.all(np.abs(xd[:, d] - cs.x[:, d]) < w), "an atom moves by a whole brick width"
        self.x = xd
        self.v = np.stack([np.arange(n) + 0.25, -0.5 * np.arange(n) - 1.0, 1000.0 + np.arange(n) * 0.125], axis=1)
        self.tag = np.arange(n, dtype=np.int64) + 10 ** 6
        self.chain, self.lists, self.sizes = self._chain()

    def wrapped(self):
        return self.x - np.floor(self.x / self.cs.box) * self.cs.box

    def _chain(self):
        """wrap; per decomposed dimension keep / down / up by the rule of row_class(MigCut) (cell clipped into the grid, delta = (cell - coord) mod g, g - 1 = down
        and wins, 1 = up); new order: kept rows, then the down list of the upper neighbour, then the up list of the lower neighbour (from[0], then from[1], as in
        borders and as md.py's torch chain has it: the swap towards the lower neighbour receives from the upper one.  The source comment "from below, then from above"
        names the lists the senders took the rows from, not the ranks they came from).
        Returns (ids per rank in final order, {dimension: per rank (len down, len up)}, largest row count any rank reaches)."""
        cs = self.cs
        xw = self.wrapped()
        ids = [o.copy() for o in cs.owned]
        lists, worst = {}, 0
        for d in range(3):
            g = cs.grid[d]
            if g == 1:
                continue
            parts = []
            for r, c in enumerate(cs.coords):
                cl = np.clip(np.floor(xw[ids[r], d] / cs.width[d]).astype(np.int64), 0, g - 1)
                delta = (cl - c[d]) % g
                down = delta == g - 1
                up = (delta == 1) & ~down
                parts.append((ids[r][~(down | up)], ids[r][down], ids[r][up]))
            lists[d] = [(len(p[1]), len(p[2])) for p in parts]
            for r, c in enumerate(cs.coords):
                above, _ = cs.neighbour(c, d, +1)
                below, _ = cs.neighbour(c, d, -1)
                ids[r] = np.concatenate([parts[r][0], parts[above][1], parts[below][2]])
                worst = max(worst, len(ids[r]))
        return ids, lists, worst


_migrations = {}


def migration(name):
    if name not in _migrations:
        _migrations[name] = Migration(case(name))
    return _migrations[name]


def check_migration_inputs(mg):
    cs = mg.cs
    cell0 = np.floor(cs.x / cs.width).astype(np.int64)
    xw = mg.wrapped()
    cell1 = np.clip(np.floor(xw / cs.width).astype(np.int64), 0, np.array(cs.grid) - 1)
    changed = cell0 != cell1
    assert np.any(mg.x < 0) and np.any(mg.x >= cs.box), "atoms cross the box face both ways"
    assert np.any(~changed.any(axis=1) & np.all(mg.x == cs.x, axis=1)), "atoms that do not move"
    assert len(mg.hand["onto the upper brick face"]) >= 1
    if sum(g > 1 for g in cs.grid) >= 2:
        assert np.any(changed.sum(axis=1) >= 2), "atoms that change brick in two dimensions at once"
    for d in distinct_peer_dims(cs):
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
        nn = comm.migrate(nl, x.data_ptr(), v.data_ptr(), tag.data_ptr(), mt.data_ptr(), cap, cs.box, cs.grid, coord)
        sync(dev)
        return {"n": nn, "x": x.cpu().numpy(), "v": v.cpu().numpy(), "tag": tag.cpu().numpy(), "id": mt.cpu().numpy(), "sent": [list(g) for g in comm.sent]}
    return fn


def check_migration(lib, dev, name):
    mg = migration(name)
    cs = mg.cs
    check_migration_inputs(mg)
    res = run_ranks(cs.grid, migration_rank_fn(mg, dev, mg.sizes + 5), lib, dev)
    xw = mg.wrapped()
    print(f"\n{name} on {dev.type}: (down, up) list lengths per rank {mg.lists}")
    for r, o in enumerate(res):
        print(f"  rank {r}: {len(cs.owned[r])} -> {o['n']} owned rows, {sum(len(g) for g in o['sent'])} messages sent")
    for r, o in enumerate(res):
        ids = mg.chain[r]
        assert o["n"] == len(ids), f"rank {r}: {o['n']} owned atoms, the chain has {len(ids)}"
        n = o["n"]
        np.testing.assert_array_equal(o["id"][:n], ids, err_msg=f"rank {r}: mtype in order")
        np.testing.assert_array_equal(o["tag"][:n], mg.tag[ids], err_msg=f"rank {r}: tag")
        np.testing.assert_array_equal(o["x"][:n], xw[ids], err_msg=f"rank {r}: wrapped x")
        np.testing.assert_array_equal(o["v"][:n], mg.v[ids], err_msg=f"rank {r}: v")
    # independent of the chain: nobody lost or doubled, everybody in the brick of its wrapped position
    everybody = np.concatenate([o["id"][: o["n"]] for o in res])
    np.testing.assert_array_equal(np.sort(everybody), np.arange(len(cs.x)), err_msg="every atom exactly once over all ranks")
    for r, o in enumerate(res):
        xr = o["x"][: o["n"]]
        assert np.all(xr >= 0) and np.all(xr < cs.box), f"rank {r}: a position outside the box"
        np.testing.assert_array_equal(np.floor(xr / cs.width), np.broadcast_to(np.array(cs.coords[r], dtype=np.float64), xr.shape), err_msg=f"rank {r}: brick of the wrapped position")
    # what the transport counted: with three or more bricks the down and the up records (64 bytes each) leave as two messages to two peers
    for d in distinct_peer_dims(cs):
        hits = [two_message_groups(cs, r, o["sent"], d, 64) for r, o in enumerate(res)]
        assert max(hits) >= 1, f"dimension {d}: no rank sent two separate migration messages ({hits})"
        assert max(up for _, up in mg.lists[d]) > 0, f"dimension {d}: every up list is empty"


def check_migration_overflow(lib, dev, name):
    """a common capacity that the fullest brick exceeds by one row: every rank returns the same negative number of larger magnitude (contents not asserted)"""
    mg = migration(name)
    cs = mg.cs
    cap = mg.sizes - 1
    assert cap >= max(len(o) for o in cs.owned), "the capacity must hold what every rank starts with"
    res = run_ranks(cs.grid, migration_rank_fn(mg, dev, cap), lib, dev)
    answers = [o["n"] for o in res]
    print(f"\n{name}: capacity {cap}, answers {answers}")
    assert len(set(answers)) == 1 and answers[0] < 0 and -answers[0] > cap, answers
