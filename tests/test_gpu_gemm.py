"""The float32 MFMA GEMM of the layer-at-a-time path (csrc/gemm.hip: k_gemm_f32, four instances TRANSB x VECA) called directly through
ahip_debug_gemm_f32 against float64 numpy -- widths that are no multiple of 4, 16 or 64, row strides and sub-block views that are not 16-byte
aligned, row counts around the 64-row block, both epilogues -- and through models whose every width is odd for the kernels (tensor product,
row reductions) that only see U and S through a model.  The host-emulation build has no MFMA: its entry point answers "unsupported"."""
import numpy as np
import pytest

import parity_cases as pc
import util
from pair_allegro_amd import capi, model_file

ES = [1, 63, 64, 65, 200]
KN = [(1, 1), (3, 15), (16, 64), (17, 65), (40, 130), (300, 37), (6, 6)]
LAYOUTS = ["dense", "padded", "view"]        # lda = K; lda = K + 5; lda = 9 K with the view starting at column K (V + lm * U of a [E][9][U] array)
U24 = 2.0 ** -24
# Epilogues (__expf): largest relative deviation measured on an MI355X over the cases of this file, of silu_out from float64 silu(C) and of the
# dsilu_z result from float64 C * silu'(z), C being the kernel's own product.  The bars are 4 x the measurement, and may never exceed CAP.
SILU_MEASURED, DSILU_MEASURED = 4.30e-7, 5.02e-7
SILU_REL, DSILU_REL = 4.0 * SILU_MEASURED, 4.0 * DSILU_MEASURED
CAP_REL, CAP_ABS = 1e-5, 1e-7
# silu'(z) crosses zero at z = -1.278, where the cancelled float32 factor has no relative bar: the elements with |silu'(z)| < 0.05 are held by an absolute term,
# the cap itself (measured there: 8.0e-8 at |C| up to 4.5, i.e. float32 rounding of a factor of size 1 times C)
DSILU_ABS = CAP_ABS
seen_veca = set()


def cases(K, N):
    """every (E, transB, accumulate, layout) of one (K, N), numbered: odd numbers get ldc > N and a padded W"""
    k = 0
    for E in ES:
        for transB in (0, 1):
            for acc in (0, 1):
                for layout in LAYOUTS:
                    k += 1
                    yield E, transB, acc, layout, k


def make(E, K, N, transB, layout, k):
    rng = np.random.default_rng([E, K, N, transB, LAYOUTS.index(layout), k])
    lda, a_off = {"dense": (K, 0), "padded": (K + 5, 0), "view": (9 * K, K)}[layout]
    A = rng.standard_normal(a_off + (E - 1) * lda + K + 3).astype(np.float32)
    rows, cols = (N, K) if transB else (K, N)
    ldw = cols + (k % 2) * 3
    W = (rng.standard_normal(rows * ldw) / np.sqrt(K)).astype(np.float32)       # variance-preserving like the model's weights: C = O(1)
    ldc = N + (k % 2) * 3
    C_in = rng.standard_normal(E * ldc).astype(np.float32)
    Av = A[a_off + np.arange(E)[:, None] * lda + np.arange(K)[None, :]].astype(np.float64)
    Wm = W[np.arange(rows)[:, None] * ldw + np.arange(cols)[None, :]].astype(np.float64)
    B = Wm.T if transB else Wm
    veca = lda % 4 == 0 and K % 4 == 0 and (4 * a_off) % 16 == 0                  # gemm_f32's choice (device allocations are 256-byte aligned)
    seen_veca.add((bool(veca), K, layout))
    return dict(E=E, K=K, N=N, A=A, lda=lda, a_off=a_off, W=W, ldw=ldw, transB=transB, C_in=C_in, ldc=ldc, Av=Av, B=B)


def run(lib, c, acc, silu=False, z=None):
    C = c["C_in"].copy()
    S = np.full(c["E"] * c["ldc"], 7.5, dtype=np.float32) if silu else None
    lib.debug_gemm_f32(c["E"], c["K"], c["N"], c["A"], c["lda"], c["a_off"], c["W"], c["ldw"], bool(c["transB"]), C, c["ldc"], bool(acc), S, z)
    C = C.reshape(c["E"], c["ldc"])
    np.testing.assert_array_equal(C[:, c["N"]:], c["C_in"].reshape(c["E"], c["ldc"])[:, c["N"]:], err_msg="columns of C beyond N were written")
    if silu:
        S = S.reshape(c["E"], c["ldc"])
        assert np.all(S[:, c["N"]:] == 7.5), "columns of silu_out beyond N were written"
    return C[:, : c["N"]], (S[:, : c["N"]] if silu else None)


def silu64(v):
    return v / (1.0 + np.exp(-v))


def dsilu64(z):
    sg = 1.0 / (1.0 + np.exp(-z))
    return sg * (1.0 + z * (1.0 - sg))


def test_emulation_build_reports_unsupported(emu_lib):
    c = make(3, 4, 4, 0, "dense", 0)
    with pytest.raises(capi.AhipError) as e:
        run(emu_lib, c, 0)
    assert e.value.code == capi.AHIP_ERR_UNSUPPORTED


def test_bars_respect_the_cap():
    assert SILU_REL <= CAP_REL and DSILU_REL <= CAP_REL and DSILU_ABS <= CAP_ABS


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", KN)
def test_gemm_against_float64(hip_lib, K, N):
    """The MFMA is exact float32: |C - C_ref| <= (K + 2) 2^-24 sum_k |a||w| per element (a chain of K fused multiply-adds, the store), plus
    2^-24 |C_in| when accumulating.  Columns beyond N stay untouched."""
    worst = 0.0
    for E, transB, acc, layout, k in cases(K, N):
        c = make(E, K, N, transB, layout, k)
        C, _ = run(hip_lib, c, acc)
        Cin = c["C_in"].reshape(E, c["ldc"])[:, :N].astype(np.float64)
        ref = c["Av"] @ c["B"] + (Cin if acc else 0.0)
        bar = (K + 2) * U24 * (np.abs(c["Av"]) @ np.abs(c["B"])) + (U24 * np.abs(Cin) if acc else 0.0)
        err = np.abs(C.astype(np.float64) - ref)
        worst = max(worst, float((err / bar).max()))
        assert np.all(err <= bar), (E, K, N, transB, acc, layout, float((err / bar).max()))
    print(f"\ngemm K {K} N {N}: worst error / bar {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", KN)
def test_silu_epilogue(hip_lib, K, N):
    """silu_out = silu(C) of the kernel's own C (which equals the plain call's bit for bit), stride ldc like C.
    Measured on an MI355X: largest |silu_out - silu64(C)| / |silu64(C)| = 4.30e-7 over all cases of this file (per (K, N): 2.3e-7 .. 4.3e-7); bar 1.72e-6."""
    worst, bad = 0.0, []
    for E, transB, acc, layout, k in cases(K, N):
        c = make(E, K, N, transB, layout, k)
        C0, _ = run(hip_lib, c, acc)
        C, S = run(hip_lib, c, acc, silu=True)
        np.testing.assert_array_equal(C, C0)
        ref = silu64(C.astype(np.float64))
        err = np.abs(S.astype(np.float64) - ref)
        nz = ref != 0.0
        assert np.all(err[~nz] == 0.0)
        rel = float((err[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0
        worst = max(worst, rel)
        if not np.all(err <= SILU_REL * np.abs(ref)):
            bad.append((E, transB, acc, layout, rel))
    print(f"\nsilu K {K} N {N}: largest relative deviation {worst:.3e}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", KN)
def test_dsilu_epilogue(hip_lib, K, N):
    """C = (A W (+ C_in)) * silu'(z), z [E][ldc] like C: against float64 silu' applied to the plain call's C.
    Measured on an MI355X: largest |C - C_plain silu'(z)| / |C_plain silu'(z)| over the elements with |silu'(z)| >= 0.05 = 5.02e-7
    (per (K, N): 3.9e-7 .. 5.0e-7); bar 2.01e-6 relative + 1e-7 absolute; near the zero of silu' (z = -1.278) the largest absolute deviation was 8.0e-8."""
    worst, worst_abs, bad = 0.0, 0.0, []
    for E, transB, acc, layout, k in cases(K, N):
        c = make(E, K, N, transB, layout, k)
        z = (1.5 * np.random.default_rng([7, E, K, N, k]).standard_normal(E * c["ldc"])).astype(np.float32)
        C0, _ = run(hip_lib, c, acc)
        C, _ = run(hip_lib, c, acc, z=z)
        d = dsilu64(z.reshape(E, c["ldc"])[:, :N].astype(np.float64))
        ref = C0.astype(np.float64) * d
        err = np.abs(C.astype(np.float64) - ref)
        far = (np.abs(d) >= 0.05) & (ref != 0.0)
        worst = max(worst, float((err[far] / np.abs(ref[far])).max()) if far.any() else 0.0)
        worst_abs = max(worst_abs, float(err[~far].max()) if (~far).any() else 0.0)
        allowed = DSILU_REL * np.abs(ref) + DSILU_ABS
        if not np.all(err <= allowed):
            bad.append((E, transB, acc, layout, float((err / allowed).max())))
    print(f"\ndsilu K {K} N {N}: largest relative deviation {worst:.3e}; largest absolute deviation near the zero of silu' {worst_abs:.3e}")
    assert not bad, bad


def test_both_load_instances_are_covered():
    """the cases above reach VECA = false (K or lda no multiple of 4) and VECA = true (aligned views included)"""
    for K, N in KN:
        for E, transB, acc, layout, k in cases(K, N):
            make(E, K, N, transB, layout, k)
    assert (False, 6, "view") in seen_veca and (True, 16, "view") in seen_veca and (False, 16, "padded") in seen_veca and (True, 300, "dense") in seen_veca


# ---- through the model: every width odd for the kernels ----
ODD = {
    "l1": dict(l_max=1, num_scalar_features=17, num_tensor_features=5, mlp_width=19, readout_width=7),
    "l2": dict(l_max=2, num_scalar_features=30, num_tensor_features=6, mlp_width=37, readout_width=10),
    "l3": dict(l_max=3, num_scalar_features=22, num_tensor_features=3, mlp_width=70, readout_width=1),
}


def odd_cfg(name, g):
    return model_file.model_S(type_names=["Ag", "Cu", "O"], avg_num_neighbors=float(g["nedges"]) / len(g["pos"]), **ODD[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ODD))
def test_odd_width_models_on_the_layer_kernels(hip_lib, model_dir, name):
    """S / U / MLP / read-out widths 17 / 5 / 19 / 7 (l_max 1), 30 / 6 / 37 / 10 (l_max 2), 22 / 3 / 70 / 1 (l_max 3) on Cu2AgO4: the VECA = false GEMM
    instances, sub-block views V + lm U that are not 16-byte aligned, K / N tails, odd-U tensor products and row reductions, against the float64 oracle."""
    g = util.load_golden("Cu2AgO4_r5")
    cfg = odd_cfg(name, g)
    w = model_file.init_weights(cfg)
    path = f"{model_dir}/odd_{name}.ahip"
    model_file.save_ahip(path, cfg, w)
    names = sorted(set(g["symbols"]))
    types = np.array([names.index(s) + 1 for s in g["symbols"]], dtype=np.int32)
    ref = util.oracle_run(dict(cfg, model_dtype="float64"), w, g["cell"], g["pos"], types, names)
    res = util.run_pair(hip_lib, path, g["cell"], g["pos"], types, names, options={"path": "generic"})
    assert res["info"]["path"] == "generic_f32", res["info"]
    df = np.abs(res["forces"] - ref["forces"]).max()
    print(f"\nodd widths {name}: max|dF| {df:.3e} (max|F| {np.abs(ref['forces']).max():.3f})")
    util.assert_close_to(res, ref, 5e-4, what=f"odd widths {name} vs f64 oracle")
    assert df < pc.NORTH_STAR_DF
