"""Option dense_centres and ahip_last_heavy_centres without a GPU: the option's words, the symbol in the header, the binding and the host-emulation library, and
that the option changes nothing where no fused kernel runs (the emulation has none: tests/host_emu)."""
import os
import re

import numpy as np
import pytest

import dense_centres_cases as dc
from pair_allegro_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_centres_option_words(emu_lib, model_dir):
    c = dc.case(model_dir, "S_light4")
    m = capi.Model(c["path"], 0, emu_lib)
    for v in ("whole", "split", "whole"):
        m.set_option("dense_centres", v)
    for bad in ("bogus", "", "Split", "1"):
        with pytest.raises(capi.AhipError) as e:
            m.set_option("dense_centres", bad)
        assert e.value.code == capi.AHIP_ERR_ARG and "whole|split" in e.value.msg
    m.close()


def test_last_heavy_centres_is_declared_bound_and_exported(emu_lib):
    header = open(os.path.join(ROOT, "include", "allegro_hip.h")).read()
    assert re.search(r"\bint ahip_last_heavy_centres\(ahip_model \*m, int \*ncentres, long long \*nedges\);", header)
    assert '"dense_centres" = "whole" | "split"' in header
    assert "ahip_last_heavy_centres" in capi.SYMBOLS and hasattr(emu_lib.lib, "ahip_last_heavy_centres")
    # header, binding and library carry the same symbol set
    declared = set(re.findall(r"\b(ahip_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.SYMBOLS)
    assert all(hasattr(emu_lib.lib, s) for s in capi.SYMBOLS)
    lib = os.path.join(ROOT, "pair_allegro_amd", "liballegro_hip.so")
    if os.path.exists(lib):                      # the product library, when it has been built (loading it needs no GPU)
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "ahip_last_heavy_centres")
    assert isinstance(capi.Model.last_heavy_centres, property)
    n = emu_lib.lib.ahip_last_heavy_centres(None, None, None)
    assert n == capi.AHIP_ERR_ARG


def test_split_changes_nothing_without_a_fused_kernel(emu_lib, model_dir):
    """The emulation evaluates every list on the layer-at-a-time kernels: the same numbers with either value, no centres reported."""
    c = dc.case(model_dir, "S_light4")
    assert dc.heavy_counts(c)[0] == len(dc.HEAVY)
    whole = dc.run(emu_lib, c)
    split = dc.run(emu_lib, c, options={"dense_centres": "split"})
    assert whole["path"] == split["path"] == "generic_f32"
    assert whole["heavy"] == split["heavy"] == (0, 0)
    assert whole["max_degree"] == split["max_degree"] == c["deg"].max()
    for q in ("forces", "eatom", "virial"):
        assert np.array_equal(whole[q], split[q]), q
    assert whole["pe"] == split["pe"]
