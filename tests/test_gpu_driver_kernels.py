"""The kernels of the stand-alone driver -- the cell-list neighbour builder against brute force, the KOKKOS table hand-over and the type mapping on
device memory, the NVE half steps against float64 numpy, the one-rank exchange plan -- on the CPU (the same kernel sources as loops, host-emulation
build) and on the MI355X.  Cases and references: tests/driver_kernel_cases.py."""
import pytest
import torch

import driver_kernel_cases as dk

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def backend(request):
    """(library, torch device of the `_dev` pointers)"""
    if request.param == "emu":
        return request.getfixturevalue("emu_lib"), torch.device("cpu")
    return request.getfixturevalue("hip_lib"), torch.device("cuda", 0)


@pytest.fixture
def model(backend, model_dir):
    m = dk.model(backend[0], model_dir)
    yield m
    m.close()


@pytest.mark.parametrize("name", list(dk.neighbour_cases()))
def test_neighbour_builder_equals_brute_force(backend, model, name):
    """ahip_borders_local_dev + ahip_build_neighbors_dev + one ahip_compute_dev: the edges are the brute-force pairs over the materialised rows, none
    twice, the list size is their number, and a second build gives the same edge_index (the within-bin order is sorted)."""
    n = dk.check_neighbour_case(backend[0], backend[1], model, name)
    print(f"\n{name}: {n} edges")


def test_list_with_a_skin_is_filtered_at_r_max(backend, model):
    dk.check_skin_list(backend[0], backend[1], model)


def test_table_handover_equals_the_csr_handover(backend, model):
    """ahip_neigh_update_dev_table, row-major and column-major, high bits above the neighbour mask set, permuted ilist, an empty row, 5000 centres:
    the same edges (and forces) as the same list handed over with ahip_neigh_update_csr."""
    dk.check_table_handover(backend[0], backend[1], model)


def test_table_handover_rejects_bad_input(backend, model):
    dk.check_table_rejections(backend[0], backend[1], model)


def test_map_types(backend, model):
    dk.check_map_types(backend[0], backend[1], model)


@pytest.mark.parametrize("which", [0, 1, "first"])
def test_nve_half_steps(backend, model, which):
    for n in dk.NVE_N:
        dk.check_nve(backend[0], backend[1], model, n, which)


def test_local_exchange_plan(backend):
    dk.check_local_plan(backend[0], backend[1])
