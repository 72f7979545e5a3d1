"""csrc/comm.hip at kernel level with every rank of a grid in one process (ranks as threads, one baton: tests/comm_rank_cases.py): the ghost rows of
ahip_comm_borders against brute force (the set) and against a numpy swap chain (the order), ahip_comm_forward / ahip_comm_reverse on the plan borders installed,
ahip_comm_migrate against a numpy chain -- on grids with one, two and three or more bricks per dimension, the last of which no other test reaches (every
other multi-rank test draws its grid from md.choose_grid of 2, 4 or 8).  On the CPU (host-emulation build) and on the MI355X."""
import numpy as np
import pytest
import torch

import comm_rank_cases as cr
import driver_kernel_cases as dk

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
NAMES = list(cr.CASES)


@pytest.fixture(params=BACKENDS)
def backend(request):
    """(library, torch device of the `_dev` pointers)"""
    if request.param == "emu":
        return request.getfixturevalue("emu_lib"), torch.device("cpu")
    return request.getfixturevalue("hip_lib"), torch.device("cuda", 0)


def test_case_inputs():
    """what the cases promise: row counts that are no multiple of 32, rows of class 3 (both slabs) on x3 and of class 0 (neither) on x3_wide, the plane atoms on
    either side of both slab criteria, more than 8192 rows with a partial last chunk on block_boundary, empty ranks on empty_bricks"""
    for name in NAMES:
        cs = cr.case(name)
        if cs.kind == "gas":
            assert all(30 < len(o) and len(o) % 32 != 0 for o in cs.owned), name
            for r, c in enumerate(cs.coords):
                lo, hi = cs.brick(c)
                for d in range(3):
                    v = set(cs.x[cs.owned[r], d].tolist())
                    assert {lo[d], hi[d] - cr.U, lo[d] + cr.RC, lo[d] + cr.RC - cr.U, hi[d] - cr.RC, hi[d] - cr.RC - cr.U} <= v, (name, r, d)
            assert 0.0 in cs.x[:, 0] and cs.box[0] - cr.U in cs.x[:, 0]
    assert any(3 in cr.slab_classes(cr.case("x3"), r) for r in range(3))
    assert all(0 in cr.slab_classes(cr.case("x3_wide"), r) for r in range(3))
    big = cr.case("block_boundary")
    assert len(big.x) == 27000 and all(len(o) > 8192 and len(o) % 32 != 0 for o in big.owned)
    assert [len(o) > 0 for o in cr.case("empty_bricks").owned] == [True, False, False]
    assert [len(o) for o in cr.case("one_atom_each").owned] == [1, 1, 1]


def test_transport_turns_a_mismatch_into_an_error(backend):
    """a rank that announces a receive nobody sends for, with the peer already gone: the wait ends (here at once, through the abort flag; after 30 s at the
    latest), the library reports the callback's failure and run_ranks raises -- nothing hangs"""
    lib, dev = backend

    def fn(rank, coord, comm):
        if rank == 1:
            raise ValueError("rank 1 leaves early")
        buf = torch.zeros(4, dtype=torch.int32, device=dev)
        comm.allreduce(buf.data_ptr(), 1, 1)

    with pytest.raises((ValueError, RuntimeError)):
        cr.run_ranks((2, 1, 1), fn, lib, dev)


@pytest.mark.parametrize("name", NAMES)
def test_borders_rows_are_the_brute_force_images(backend, name):
    """(a) the set: owned rows in the order given, then exactly the periodic images inside [lo - rc, hi + rc) on every axis, as a multiset of (id, position), bit for bit"""
    res = cr.exchange_run(backend[0], backend[1], name)
    cr.check_borders_set(cr.case(name), res, cr.references(name)[0])


@pytest.mark.parametrize("name", NAMES)
def test_borders_rows_are_in_swap_chain_order(backend, name):
    """(b) the order: rows, ids and the returned row count equal the numpy swap chain of comm_rank_cases.swap_chain_rows; and the transport saw two separate
    slab messages to two peers in every dimension with three or more bricks (one merged message with two)"""
    res = cr.exchange_run(backend[0], backend[1], name)
    cr.check_borders_order(cr.case(name), res, cr.references(name)[1])
    cr.check_borders_messages(cr.case(name), res)


def test_one_rank_borders_equal_borders_local(backend, model_dir):
    """case `one`: ahip_comm_borders on a 1x1x1 grid (all swaps are self copies) gives the ghosts of ahip_borders_local_dev on the same atoms, as a multiset"""
    lib, dev = backend
    cs = cr.case("one")
    res = cr.exchange_run(lib, dev, "one")[0]
    nl, nall = res["nlocal"], res["nall"]
    m = dk.model(lib, model_dir)
    cap = nall - nl + 5
    xl, ml = cr.to_dev(cs.x, dev), cr.to_dev(np.arange(nl), dev, np.int32)
    xg = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
    mg = torch.zeros(cap, dtype=torch.int32, device=dev)
    src = torch.zeros(cap, dtype=torch.long, device=dev)
    shv = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
    ng = m.borders_local_dev(nl, xl.data_ptr(), ml.data_ptr(), np.zeros(3), cs.box, cs.box, cr.RC, cap, xg.data_ptr(), mg.data_ptr(), src.data_ptr(), shv.data_ptr())
    cr.sync(dev)
    m.close()
    assert ng == nall - nl
    np.testing.assert_array_equal(cr.sorted_rows(mg.cpu().numpy()[:ng], xg.cpu().numpy()[:ng]), cr.sorted_rows(res["id"][nl:nall], res["x"][nl:nall]))


def test_borders_capacity_protocol(backend):
    """x3y2, every rank with (largest true need) - 1 rows: all ranks get the same answer > capacity, the call repeated with the answer as capacity reaches the
    rows of a direct call within 4 calls, and no call times out (the ranks that overflowed keep exchanging messages of the announced sizes)"""
    cr.check_capacity_protocol(backend[0], backend[1])


@pytest.mark.parametrize("name", NAMES)
def test_forward_moves_every_ghost_with_its_owner(backend, name):
    res = cr.exchange_run(backend[0], backend[1], name)
    cr.check_forward(cr.case(name), res)


@pytest.mark.parametrize("name", NAMES)
def test_reverse_sums_every_row_of_an_atom_into_its_owner(backend, name):
    res = cr.exchange_run(backend[0], backend[1], name)
    most = cr.check_reverse(cr.case(name), res)
    cr.check_exchange_messages(cr.case(name), res)
    print(f"\n{name}: an atom has {most} rows")


@pytest.mark.parametrize("name", cr.MIGRATION_CASES)
def test_migration_equals_the_numpy_chain(backend, name):
    """owned count and every row of x (wrapped), v, tag, mtype in order; every atom once and in the brick of its wrapped position; with three or more bricks a
    non-empty `up` list and two separate messages (counted by the transport)"""
    cr.check_migration(backend[0], backend[1], name)


@pytest.mark.parametrize("name", ["x3", "x3y2"])
def test_migration_overflow_is_agreed_on(backend, name):
    cr.check_migration_overflow(backend[0], backend[1], name)
