"""The arithmetic policy of the fused kernels (pair_allegro_amd/csrc/arith_policy.h) on the CPU: the stand-alone program
tests/host_emu/arith_policy_main.cpp prints what the header resolves for every combination of its inputs and `_rules` below
restates the rules independently; and every enumerated option of ahip_set_option takes its words and refuses anything else
with its exact text (host-emulation library)."""
import itertools
import os
import subprocess

import pytest

from oracle import allegro_torch
from pair_allegro_amd import capi, model_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")

WORDS = ["auto", "f32", "f16x2", "bf16x3", "tf32eq", "b3", "fp8"]       # effective option: the option's words, the override's b3, junk
PATH_NAMES = {0: "fused_f32", 1: "fused_bf16x3", 2: "fused_tf32eq", 3: "fused_f16x2"}


def _rules(word, allow_tf32, degraded, force_f32, table, wide):
    """0 f32, 1 bf16x3, 2 tf32eq, 3 f16x2.  Written from the rules, not from the library."""
    auto = word == "auto"
    f16x2 = word == "f16x2" or (auto and not degraded and not force_f32)
    if wide:                                   # f16x2 and f32 only; allow_tf32 and fused_tb play no part
        return 3 if f16x2 else 0
    if word in ("bf16x3", "b3"):
        return 1
    if word == "tf32eq":
        return 2
    if auto and allow_tf32 and not force_f32:  # whatever `degraded` is
        return 2
    if f16x2:
        return 3 if table else 0               # the f16x2 instances exist with the tabulated two-body embedding only
    return 0                                   # f32, a degraded or forced auto, any unrecognised word


def test_policy_table_matches_the_rules():
    subprocess.run(["make", "-C", EMU, "_build/arith_policy"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = subprocess.run([os.path.join(EMU, "_build", "arith_policy")], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    got = {}
    names = {}
    for line in out:
        f = line.split()
        if f[0] == "name":
            names[int(f[1])] = f[2]
            continue
        word, allow, degraded, force, tb, fam, arith, path = f
        assert tb in ("table", "mlp") and fam in ("k_fused", "wide")
        key = (word, int(allow), int(degraded), int(force), tb == "table", fam == "wide")
        assert key not in got
        got[key] = (int(arith), path)
    want = {}
    for key in itertools.product(WORDS, (0, 1), (0, 1), (0, 1), (True, False), (False, True)):
        a = _rules(*key)
        want[key] = (a, PATH_NAMES[a])
    assert len(want) == 224 and set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    # the enumerators of the option carry the option's words, in the order of its error text
    assert names == dict(enumerate(OPTIONS["fused_arith"].split("|")))


OPTIONS = {
    "path": "auto|fused|generic",
    "precision": "model|float64",
    "fused_arith": "auto|f32|f16x2|bf16x3|tf32eq",
    "fused_tb": "table|mlp",
    "cutoff_compare": "le|lt",
    "edge_schedule": "auto|static|dynamic",
    "tile_pack": "auto|separate|fused",
}


def test_enumerated_options_take_their_words_only(emu_lib, model_dir):
    cfg = model_file.model_S(model_dtype="float64", num_scalar_features=16, num_tensor_features=8, mlp_width=16, readout_width=8)
    p = os.path.join(model_dir, "options.nequip.pth")
    allegro_torch.export_nequip_pth(p, cfg)
    m = capi.Model(p, 0, emu_lib)
    for key, words in OPTIONS.items():
        for w in words.split("|") + [words.split("|")[0]]:         # every word, and back to the default
            m.set_option(key, w)
        for bad in ("nope", "", words, words.split("|")[0].upper(), words.split("|")[0] + "|"):
            with pytest.raises(capi.AhipError) as e:
                m.set_option(key, bad)
            assert e.value.msg == f"option {key}: expected {words}" and e.value.code == 1
    with pytest.raises(capi.AhipError) as e:
        m.set_option("b3", "auto")
    assert e.value.msg == "unknown option 'b3'"
    with pytest.raises(capi.AhipError) as e:
        m.set_option("fused_arith", "b3")                          # the environment override's word is not an option value
    assert e.value.msg == "option fused_arith: expected auto|f32|f16x2|bf16x3|tf32eq"
