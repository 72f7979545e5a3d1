"""Any periodic cell on the CPU emulation (the kernels of csrc/neigh.hip compiled for the host): the ghost builder ahip_borders_cell_dev against the
rule stated in numpy -- triclinic cells, cells thinner than the cutoff, open axes, a rotated cell -- its capacity protocol, its reduction to
ahip_borders_local_dev on an orthogonal box, the wrap ahip_wrap_cell_dev, and the argument errors."""
import numpy as np
import pytest
import torch

import cell_cases as cc
from pair_allegro_amd import lmp_like

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def model(emu_lib, model_dir):
    m = cc.border_model(emu_lib, model_dir)
    yield m
    m.close()


@pytest.mark.parametrize("name,rc,pbc,expected", cc.GHOST_CASES)
def test_ghost_set_equals_the_rule(model, name, rc, pbc, expected):
    cell, x, sym = cc.geometry(name)
    cc.check_ghost_set(model, CPU, cell, x, cc.types_of(sym), pbc, rc, expected)


@pytest.mark.parametrize("name,rc", [(c[0], c[1]) for c in cc.GHOST_CASES if c[2] == (1, 1, 1) and "rotated" not in c[0]])
def test_counts_equal_the_host_builder(name, rc):
    """the table's counts are those of lmp_like.build_rank_system, the host ghost builder the parity tests run on"""
    cell, x, sym = cc.geometry(name)
    ref, _ = cc.reference_ghosts(cell, x, (1, 1, 1), rc)
    assert lmp_like.build_rank_system(cell, x, np.ones(len(x), np.int32), rc).nghost == len(ref)


def test_one_atom_and_a_block_boundary(model):
    cell, x, sym = cc.geometry("Cu-cubic")
    cc.check_ghost_set(model, CPU, cell, x[:1], cc.types_of(sym)[:1], (1, 1, 1), 6.0)
    cell, x, sym = cc.big_257()
    cc.check_ghost_set(model, CPU, cell, x, cc.types_of(sym), (1, 1, 1), 6.0)


def test_capacity_protocol(model):
    cc.check_capacity(model, CPU)


def test_orthogonal_box_reduces_to_borders_local(model):
    cc.check_orthogonal_reduction(model, CPU)


def test_wrap(model):
    cc.check_wrap(model, CPU)
    cc.check_wrap(model, CPU, "Cu2AgO4-rotated")


def test_argument_errors(model):
    cc.check_errors(model, CPU)
