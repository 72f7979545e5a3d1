"""GPU tests of the f16x2 operand split of k_fused in its mixed-precision-fma form (csrc/fused_h.h: split2_h<true>): one v_cvt_pk_f16_f32, two
v_fma_mix_f32 for the remainders v - hi, two v_mul_f32 and one v_cvt_pk_f16_f32 for the scaled lo' pair, in place of convert, convert back, subtract, scale, convert.

(i)   The split alone, through the driver kernel k_split_probe (ahip_debug_fused_linear with AHIP_DEBUG_SPLIT=mix|ref): 2^16 floats, hi and lo' bit for bit against
      the NumPy form of util.split_emulation.f16_terms, hi = f16(v), lo' = f16((v - hi) 2^11), both round-to-nearest-even.
(ii)  The 64-atom Si box and the three-type Cu2AgO4 box, 1..3 layers x latent MLP depth 1..3 x read-out depth 1..2, default options, and the 8-wave shape forced
      once: max|dF| against the float64 oracle below parity_cases.F32EQ_DF (5e-6 eV/A, the bar of a float32-equivalent split arithmetic) and below
      max(3 e_generic, 1e-5), e_generic being the error of the layer-at-a-time float32 kernels on the same file (the bar of fused_shape_cases.assert_bars); energies and
      virial within 5e-4 (util.assert_close_to).
(iii) Two launches of the same list, per-atom energies bit for bit: the jittered simple-cubic box (6 neighbours per atom, up to six centres per 64-slot tile: the
      per-edge arm of the environment backward) and Cu2AgO4 (one centre of 36..39 edges per tile: the fourth wave of every tile holds no edge).
Every figure is printed before it is asserted.  The oracle runs once per model (fused_shape_cases.model) and is shared.
Measured on the MI355X: 0 mismatches of 65 536 in both forms; max|dF| 3.1e-7 .. 2.8e-6 over the 36 instances (layer-at-a-time float32 kernels: 6.4e-7 .. 9.7e-6);
8-wave tiles 4.9e-7."""
import numpy as np
import pytest

import fused_shape_cases as fsc
import parity_cases as pc
import util

pytestmark = pytest.mark.gpu


def _si64():
    """The 64-atom Si golden as a geometry of fused_shape_cases (one type, r_max 5)."""
    if "Si64" not in fsc._geoms:
        g = util.load_golden("Si64_r5")
        fsc._geoms["Si64"] = (g["cell"], g["pos"], g["symbols"], ["Si"], 5.0, float(g["nedges"]) / len(g["pos"]))
    return "Si64"


def _sweep():
    """2^16 float32 values: random exponents across [2^-20, 65504] with both signs, +-0, values one ulp either side of float16 rounding ties (normal and subnormal hi),
    values whose remainder v - hi is subnormal in float16 before the 2^11 scale, the largest finite float16 and its neighbours, float16's smallest normal and subnormal."""
    rs = np.random.RandomState(20250)
    n = 1 << 16
    special = [0.0, -0.0, 65504.0, -65504.0, np.nextafter(np.float32(65504.0), np.float32(0)), 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0]
    # ties: the midpoint of two neighbouring float16 values, and the float32 neighbours of that midpoint
    h = rs.randint(0x0001, 0x7BFF, size=4096).astype(np.uint16)                     # positive finite float16 below the largest, subnormals included
    lo16 = h.view(np.float16).astype(np.float32)
    hi16 = (h + np.uint16(1)).view(np.float16).astype(np.float32)
    mid = ((lo16.astype(np.float64) + hi16.astype(np.float64)) * 0.5).astype(np.float32)      # exact in float32 (12 significant bits)
    ties = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    ties = np.concatenate([ties, -ties])
    # remainders in the float16 subnormals: a small normal float16 plus a fraction of its ulp
    base = (rs.randint(0x0400, 0x2C00, size=4096).astype(np.uint16)).view(np.float16).astype(np.float32)       # normal float16 in [2^-14, 2^-4)
    ulp16 = np.float32(2.0) ** (np.floor(np.log2(base)) - 10)
    frac = rs.uniform(-0.5, 0.5, size=base.shape).astype(np.float32)
    subn = (base + frac * ulp16).astype(np.float32)                                  # |v - hi| <= ulp16 / 2 < 2^-15: a float16 subnormal before the scale
    subn = np.concatenate([subn, -subn])
    fixed = np.concatenate([np.array(special, dtype=np.float32), ties.astype(np.float32), subn])
    m = n - len(fixed)
    assert m > 0
    e = rs.uniform(-20.0, np.log2(65504.0), size=m)
    v = (np.exp2(e) * rs.choice([-1.0, 1.0], size=m)).astype(np.float32)
    v = np.clip(v, -65504.0, 65504.0).astype(np.float32)
    out = np.concatenate([fixed, v]).astype(np.float32)
    assert out.shape == (n,) and np.isfinite(out).all() and np.abs(out).max() <= 65504.0
    return out


def _numpy_split(v):
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


@pytest.mark.parametrize("form", ["mix", "ref"])
def test_split_bits_against_numpy(hip_lib, monkeypatch, form):
    """hi and lo' of the device split, both forms, bit for bit against NumPy over the sweep."""
    v = _sweep()
    K = v.size // 32
    monkeypatch.setenv("AHIP_DEBUG_SPLIT", form)
    out = hip_lib.debug_fused_linear(np.zeros((K, K)), v.reshape(32, K))
    words = out.reshape(-1).view(np.uint32)
    npairs = v.size // 2
    hi_d = np.stack([words[:npairs] & 0xFFFF, words[:npairs] >> 16], axis=1).reshape(-1).astype(np.uint16)
    lo_d = np.stack([words[npairs:] & 0xFFFF, words[npairs:] >> 16], axis=1).reshape(-1).astype(np.uint16)
    hi_n, lo_n = _numpy_split(v)
    nsub = int((np.abs((v - hi_n.view(np.float16).astype(np.float32))) < 2.0 ** -14).sum())
    bad_hi, bad_lo = int((hi_d != hi_n).sum()), int((lo_d != lo_n).sum())
    print(f"split {form}: {v.size} values, {nsub} with a remainder below 2^-14, hi mismatches {bad_hi}, lo mismatches {bad_lo}")
    if bad_lo:
        i = int(np.nonzero(lo_d != lo_n)[0][0])
        print(f"  first lo mismatch: v = {float(v[i])!r} device {int(lo_d[i]):#06x} numpy {int(lo_n[i]):#06x}")
    assert bad_hi == 0 and bad_lo == 0


@pytest.mark.parametrize("rd", [1, 2])
@pytest.mark.parametrize("md", [1, 2, 3])
@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("tag", ["Si64", "Cu2AgO4"])
def test_k_fused_instances_against_oracle_and_layer_kernels(hip_lib, model_dir, tag, nl, md, rd):
    if tag == "Si64":
        _si64()
    c = fsc.measure(hip_lib, fsc.model(model_dir, tag, "k_fused", num_layers=nl, mlp_depth=md, readout_depth=rd))
    print(f"{tag} {nl} layers MLP depth {md} read-out depth {rd}: max|dF| vs f64 oracle fused {c['err']:.3e}, layer-at-a-time f32 {c['egen']:.3e}")
    assert c["fused"]["info"]["path"] == "fused_f16x2" and c["generic"]["info"]["path"] == "generic_f32", c["fused"]["info"]
    util.assert_close_to(c["fused"], c["ref"], 5e-4, what=f"{tag} {nl}/{md}/{rd}")
    assert c["err"] < pc.F32EQ_DF
    assert c["err"] < max(3.0 * c["egen"], 1e-5)


def test_k_fused_eight_wave_shape_forced(hip_lib, model_dir, monkeypatch):
    """AHIP_FUSED_NW=8 on Cu2AgO4: three centres share a 128-slot tile (4-wave tiles: one centre each), same bars."""
    c = fsc.model(model_dir, "Cu2AgO4", "k_fused", num_layers=2, mlp_depth=2, readout_depth=1)
    pair, rs, f4, e4, _ = fsc.one_evaluation(hip_lib, c)
    try:
        assert pair.model.last_path == "fused_f16x2"
        slots4 = pair.model.tile_occupancy()[1]
    finally:
        pair.model.close()
    monkeypatch.setenv("AHIP_FUSED_NW", "8")
    pair, _, f8, e8, _ = fsc.one_evaluation(hip_lib, c, rs=rs)
    try:
        assert pair.model.last_path == "fused_f16x2"
        slots8 = pair.model.tile_occupancy()[1]
    finally:
        pair.model.close()
    forces = np.zeros((len(c["pos"]), 3))
    np.add.at(forces, rs.tag - 1, f8)
    err = float(np.abs(forces - c["ref"]["forces"]).max())
    print(f"Cu2AgO4 8-wave tiles: {slots8} slots (4-wave: {slots4}), max|dF| vs f64 oracle {err:.3e}, max|dE_atom| vs the 4-wave run {np.abs(e8 - e4).max():.3e}")
    assert slots8 % 128 == 0 and slots8 < slots4
    assert err < pc.F32EQ_DF


@pytest.mark.parametrize("tag", ["sc27", "Cu2AgO4"])
def test_two_launches_bit_for_bit(hip_lib, model_dir, tag):
    c = fsc.model(model_dir, tag, "k_fused", num_layers=2, mlp_depth=2, readout_depth=1)
    runs = []
    rs = None
    for _ in range(2):
        pair, rs, f, e, pe = fsc.one_evaluation(hip_lib, c, rs=rs)
        try:
            assert pair.model.last_path == "fused_f16x2"
            used, total = pair.model.tile_occupancy()
            deg = pair.model.last_max_degree
        finally:
            pair.model.close()
        runs.append((f, e, pe))
    tiles = total // 64
    print(f"{tag}: {rs.nlocal} centres, {used} edges in {tiles} tiles of 64 slots, largest degree {deg}")
    assert total % 64 == 0
    if tag == "sc27":
        assert rs.nlocal >= 4 * (tiles - 1) + 1 and rs.nlocal / tiles >= 4.0          # at most the last tile holds fewer than four centres
    else:
        assert tiles == rs.nlocal and deg <= 48                                        # one centre per tile, slots 48..63 (the fourth wave) empty
    assert int((runs[0][1] != runs[1][1]).sum()) == 0
    assert np.isfinite(runs[0][1]).all()
    forces = np.zeros((len(c["pos"]), 3))
    np.add.at(forces, rs.tag - 1, runs[0][0])
    err = float(np.abs(forces - c["ref"]["forces"]).max())
    print(f"{tag}: max|dF| vs f64 oracle {err:.3e}")
    assert err < pc.F32EQ_DF
