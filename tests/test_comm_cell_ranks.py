"""Brick decomposition of any cell across ranks (csrc/comm.hip: ahip_comm_migrate_cell, ahip_comm_borders_cell and the vector-shift forward exchange) with every
rank of a grid in one process (ranks as threads, one baton: tests/comm_rank_cases.py): triclinic cells P, Q (dyadic) and R (rotated), open axes, one to four
bricks per dimension.  Cases, references and checks: tests/comm_cell_cases.py.  On the CPU (host-emulation build) and on the MI355X."""
import numpy as np
import pytest
import torch

import cell_cases as cc
import comm_cell_cases as ck
import comm_rank_cases as cr

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def backend(request):
    """(library, torch device of the `_dev` pointers)"""
    if request.param == "emu":
        return request.getfixturevalue("emu_lib"), torch.device("cpu")
    return request.getfixturevalue("hip_lib"), torch.device("cuda", 0)


def test_case_inputs():
    """what the cases promise: exact m_b, m_c on P and m_c on Q; every atom, every image and every decision plane either exact by construction or more than 2^-30
    apart (so no result depends on rounding or FMA contraction), for the positions and for the displaced positions of the migration cases; row counts that are no
    multiple of 32; about 9000 rows per rank on the big case; atoms beyond both faces of the open axis"""
    assert np.array_equal(ck.geometry(ck.P)[1][1:], [5 / 32, 5 / 16]) and ck.geometry(ck.Q)[1][2] == 5 / 16
    inv = ck.geometry(ck.Q)[0]
    assert np.array_equal(inv @ ck.Q, np.eye(3)) and np.array_equal(ck.geometry(ck.P)[0] @ ck.P, np.eye(3)), "cell^-1 of the dyadic cells is exact"
    for name in ck.CASES:
        gap = ck.check_inputs(ck.case(name))
        print(f"{name}: smallest distance to a plane on an inexact axis {gap:.3e}")
    for name in ck.MIGRATION_CASES:
        ck.check_migration_inputs(ck.migration(name))
    big = ck.case("P_x3_big")
    assert all(len(o) > 8192 and len(o) % 32 != 0 for o in big.owned)
    assert [len(o) > 0 for o in ck.case("P_x3_empty").owned] == [True, False, False]
    assert [len(o) for o in ck.case("P_x3_single").owned] == [1, 1, 1]
    assert any(ck.case("P_y2").exact[d] and ck.case("P_y2").grid[d] == 2 for d in range(3)), "a decomposed exact axis"


@pytest.mark.parametrize("name", ck.GRID_CASES)
def test_borders_rows_are_the_brute_force_images(backend, name):
    """(a) the set: owned rows in the order given, then exactly the images x + n . cell (n = 0 on open axes) with lo_d - m_d <= s_d < hi_d + m_d on every axis"""
    res = ck.exchange_run(backend[0], backend[1], name)
    ck.check_borders_set(ck.case(name), res, ck.references(name)[0])


@pytest.mark.parametrize("name", ck.GRID_CASES)
def test_borders_rows_are_in_swap_chain_order(backend, name):
    """(b) the order: rows, ids and the returned count equal the numpy swap chain in fractional coordinates, bit for bit on every cell; (c) the messages the
    transport saw: two separate ones per dimension of three or more bricks, one merged at two bricks, none across an open face"""
    res = ck.exchange_run(backend[0], backend[1], name)
    ck.check_borders_order(ck.case(name), res, ck.references(name)[1])
    ck.check_messages(ck.case(name), res, ["sent_borders"], 28)


@pytest.mark.parametrize("name", ck.ONE_RANK)
def test_one_rank_agrees_with_the_one_rank_builder(backend, model_dir, name):
    """(d) grid (1,1,1): the ghost multiset of ahip_borders_cell_dev on the same atoms -- bit for bit on the dyadic cells, by (id, n) and within 3 * 2^-52 * max|x|
    on R (the builder adds n . cell as one vector, the swaps one lattice vector per dimension)"""
    lib, dev = backend
    cs = ck.case(name)
    res = ck.exchange_run(lib, dev, name)[0]
    nl, nall = res["nlocal"], res["nall"]
    ck.check_borders_set(cs, [res], ck.references(name)[0])
    m = cc.border_model(lib, model_dir)
    ng, xg, mg, src, sh = cc.run_borders(m, dev, cs.cell, cs.x, np.arange(nl, dtype=np.int32), cs.pbc, cr.RC, nall - nl + 5)
    m.close()
    assert ng == nall - nl
    gid, gx = res["id"][nl:nall], res["x"][nl:nall]
    if cs.cellname != "R":
        np.testing.assert_array_equal(cr.sorted_rows(mg[:ng], xg[:ng]), cr.sorted_rows(gid, gx))
    else:
        a, b = ck.sorted_idn(gid, ck.recover_n(cs, gid, gx), gx), ck.sorted_idn(mg[:ng], ck.recover_n(cs, mg[:ng], xg[:ng]), xg[:ng])
        np.testing.assert_array_equal(a[:, :4], b[:, :4])
        assert np.abs(a[:, 4:] - b[:, 4:]).max() <= 3 * 2.0 ** -52 * np.abs(a[:, 4:]).max()


def test_orthogonal_cell_agrees_with_the_box_call(backend):
    """(e) cell = diag(box), full pbc, on case x3y2 of tests/comm_rank_cases.py: the rows of ahip_comm_borders, bit for bit and in order"""
    lib, dev = backend
    cs = cr.case("x3y2")
    want = cr.exchange_run(lib, dev, "x3y2")
    caps = [o["cap"] for o in want]
    got = cr.run_ranks(cs.grid, ck.exchange_rank_fn(cs, dev, caps, borders=lambda cs, comm, nl, x, mt, cap, coord: comm.borders_cell(
        nl, x.data_ptr(), mt.data_ptr(), cap, np.diag(cs.box), (1, 1, 1), cr.RC, cs.grid, coord)), lib, dev)
    for r, (a, b) in enumerate(zip(got, want)):
        assert a["nall"] == b["nall"], f"rank {r}: {a['nall']} rows, the box call has {b['nall']}"
        np.testing.assert_array_equal(a["id"], b["id"], err_msg=f"rank {r}: ids")
        np.testing.assert_array_equal(a["x"], b["x"], err_msg=f"rank {r}: rows")
        np.testing.assert_array_equal(a["x_fwd"], b["x_fwd"], err_msg=f"rank {r}: rows after forward")


@pytest.mark.parametrize("name", ck.GRID_CASES)
def test_forward_moves_every_ghost_with_its_owner(backend, name):
    """(f) each ghost equals its owner's new position plus its shift chain, exactly"""
    res = ck.exchange_run(backend[0], backend[1], name)
    ck.check_forward(ck.case(name), res, ck.references(name)[1])
    ck.check_messages(ck.case(name), res, ["sent_forward"], 24)


@pytest.mark.parametrize("name", ck.GRID_CASES)
def test_reverse_sums_every_row_of_an_atom_into_its_owner(backend, name):
    """(g) within the bound of comm_rank_cases.check_reverse"""
    res = ck.exchange_run(backend[0], backend[1], name)
    most = cr.check_reverse(ck.case(name), res)
    ck.check_messages(ck.case(name), res, ["sent_reverse"], 24)
    print(f"\n{name}: an atom has {most} rows")


@pytest.mark.parametrize("name", ck.MIGRATION_CASES)
def test_migration_equals_the_numpy_chain(backend, name):
    """(h) owned count and every row of x (wrapped), v, tag, mtype in order; nobody lost or doubled; every atom in the brick of its wrapped s; an atom that leaves
    [0, 1) on an open axis stays with its edge brick, unwrapped; the messages as in (c)"""
    ck.check_migration(backend[0], backend[1], name)


@pytest.mark.parametrize("name", ["P_x3", "P_x3y2", "R_x3y2"])
def test_migration_overflow_is_agreed_on(backend, name):
    ck.check_migration_overflow(backend[0], backend[1], name)


def test_borders_capacity_protocol(backend):
    """(i) P (3,2,1), every rank with (largest true need) - 1 rows: one answer > capacity for all, the retry reaches the rows of a direct call"""
    ck.check_capacity_protocol(backend[0], backend[1])


@pytest.mark.parametrize("name", list(ck.REFUSALS))
def test_refusals_come_before_any_message(backend, name):
    """(j) every rank gets AHIP_ERR_ARG, the transport's log shows zero messages and no row was touched"""
    ck.check_refusal(backend[0], backend[1], name)
