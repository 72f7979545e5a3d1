"""ctypes binding of liballegro_hip.so (include/allegro_hip.h).

The library is the product; this file is the thinnest possible Python view of its C-ABI, used by
the Python host mirror (pair.py), the mini-MD driver (md.py), bench.py and the tests.  It fails
loudly when the shared library is missing -- there is no Python/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "liballegro_hip.so")


def harness_pinned_copy_default() -> None:
    """For Python HARNESSES (tests/conftest.py, bench.py, the md workers), not for the library: torch moving large numpy arrays to the device goes
    through the HIP runtime's pin-on-the-fly path for pageable copies above 1 MiB, whose address-keyed cache went stale in long-lived processes
    (round 4: 4 of 10 whole-suite runs died in it).  Raising the runtime's threshold (MiB) sends those copies down its staged path.  The
    library does not depend on this -- every pageable copy of its own is staged through page-locked memory (csrc/engine.h: copy_h2d / copy_d2h) --
    and importing the binding no longer changes process-wide runtime behaviour.  Only effective before the first HIP call."""
    os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "4095")       # the largest value that also survives a 32-bit MiB -> bytes conversion


AHIP_OK, AHIP_ERR_ARG, AHIP_ERR_FILE, AHIP_ERR_DEVICE, AHIP_ERR_STATE, AHIP_ERR_UNSUPPORTED = range(6)

# every symbol declared in include/allegro_hip.h (tests check the .so exports all of them)
SYMBOLS = [
    "ahip_last_error", "ahip_device_count", "ahip_model_load", "ahip_model_free", "ahip_model_meta",
    "ahip_set_option", "ahip_get_timing_counts", "ahip_last_tile_occupancy", "ahip_neigh_update", "ahip_neigh_update_csr", "ahip_neigh_update_dev",
    "ahip_compute", "ahip_compute_dev", "ahip_output_register", "ahip_output_get", "ahip_get_edges", "ahip_debug_dump_edges", "ahip_get_timings",
    "ahip_compute_dev_range", "ahip_last_list_size", "ahip_neigh_update_dev_table", "ahip_map_types_dev", "ahip_reneighbor_flag_dev",
    "ahip_last_path", "ahip_last_max_degree", "ahip_last_heavy_centres", "ahip_debug_fused_linear", "ahip_debug_fused_edges", "ahip_build_neighbors_dev", "ahip_nve_dev", "ahip_nve_first_dev",
    "ahip_model_allow_tf32", "ahip_comm_unique_id", "ahip_comm_create_rccl", "ahip_comm_create_hosted", "ahip_comm_rccl_version", "ahip_comm_free", "ahip_comm_set_plan", "ahip_comm_set_plan_local",
    "ahip_comm_forward", "ahip_comm_reverse", "ahip_comm_allreduce", "ahip_comm_selftest", "ahip_fill_zero_dev", "ahip_borders_local_dev", "ahip_arith_note", "ahip_comm_borders", "ahip_comm_migrate",
    "ahip_debug_scan_i32", "ahip_debug_sum_columns_f64", "ahip_debug_max_i32", "ahip_debug_gemm_f32",
    "ahip_set_active_types", "ahip_get_active_types",
    "ahip_wrap_cell_dev", "ahip_borders_cell_dev", "ahip_compute_cell", "ahip_last_cell_rows",
    "ahip_compute_cells", "ahip_last_cells_ghosts",
    "ahip_comm_migrate_cell", "ahip_comm_borders_cell",
    "ahip_compute_cell_reuse", "ahip_cell_reuse_reset", "ahip_cell_reuse_stats",
    "ahip_relax_params_default", "ahip_relax_cell",
    "ahip_vcell_params_default", "ahip_relax_vcell",
    "ahip_md_params_default", "ahip_md_cell", "ahip_debug_md_noise",
    "ahip_npt_params_default", "ahip_npt_cell", "ahip_debug_npt_noise",
]


class RelaxParams(C.Structure):
    """ahip_relax_params (include/allegro_hip.h)"""
    _fields_ = [("fmax", C.c_double), ("max_steps", C.c_int), ("check_every", C.c_int), ("dt_start", C.c_double), ("dt_max", C.c_double), ("max_step", C.c_double),
                ("n_min", C.c_int), ("f_inc", C.c_double), ("f_dec", C.c_double), ("alpha_start", C.c_double), ("f_alpha", C.c_double)]


class VcellParams(C.Structure):
    """ahip_vcell_params (include/allegro_hip.h)"""
    _fields_ = [("fire", RelaxParams), ("smax", C.c_double), ("pressure", C.c_double), ("cell_factor", C.c_double), ("hydrostatic", C.c_int), ("mask", C.c_int * 6)]


class MdParams(C.Structure):
    """ahip_md_params (include/allegro_hip.h)"""
    _fields_ = [("nsteps", C.c_int), ("check_every", C.c_int), ("sample_every", C.c_int), ("frame_every", C.c_int), ("dt", C.c_double), ("ftm2v", C.c_double),
                ("mvv2e", C.c_double), ("gamma", C.c_double), ("kT", C.c_double), ("seed", C.c_ulonglong), ("step0", C.c_ulonglong)]


class NptParams(C.Structure):
    """ahip_npt_params (include/allegro_hip.h)"""
    _fields_ = [("md", MdParams), ("pressure", C.c_double), ("compressibility", C.c_double), ("tau_p", C.c_double)]


class XferOp(C.Structure):
    _fields_ = [("kind", C.c_int), ("peer", C.c_int), ("ptr", C.c_void_p), ("bytes", C.c_longlong)]


XFER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(XferOp))


class AhipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[ahip {code}] {msg}")
        self.code = code
        self.msg = msg


def _p(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


class Library:
    def __init__(self, path: Optional[str] = None):
        path = path or os.environ.get("ALLEGRO_HIP_LIB") or DEFAULT_LIB
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  allegro-hip has no CPU fallback.")
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        L.ahip_last_error.restype = C.c_char_p
        L.ahip_last_path.restype = C.c_char_p
        L.ahip_last_path.argtypes = [C.c_void_p]
        L.ahip_arith_note.restype = C.c_char_p
        L.ahip_arith_note.argtypes = [C.c_void_p]
        L.ahip_last_max_degree.argtypes = [C.c_void_p]
        L.ahip_last_heavy_centres.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        L.ahip_output_register.argtypes = [C.c_void_p, C.c_char_p]
        L.ahip_output_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_longlong)]
        L.ahip_device_count.argtypes = [C.POINTER(C.c_int)]
        L.ahip_model_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ahip_model_free.argtypes = [C.c_void_p]
        L.ahip_model_free.restype = None
        L.ahip_model_meta.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                      C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        L.ahip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.ahip_model_allow_tf32.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.ahip_neigh_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.POINTER(C.c_int)), C.c_int]
        L.ahip_neigh_update_csr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong),
                                            C.POINTER(C.c_int), C.c_int]
        L.ahip_neigh_update_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        L.ahip_compute.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ahip_compute_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ahip_compute_dev_range.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ahip_last_list_size.argtypes = [C.c_void_p]
        L.ahip_neigh_update_dev_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong,
                                                  C.c_int, C.c_void_p]
        L.ahip_reneighbor_flag_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.ahip_map_types_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        L.ahip_last_list_size.restype = C.c_longlong
        L.ahip_set_active_types.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.ahip_get_active_types.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ahip_get_edges.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
        L.ahip_debug_dump_edges.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.ahip_get_timings.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int)]
        L.ahip_get_timing_counts.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int)]
        L.ahip_build_neighbors_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_double, C.c_void_p]
        L.ahip_nve_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_double), C.c_double, C.c_double, C.c_void_p]

        L.ahip_debug_fused_linear.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.ahip_debug_scan_i32.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.ahip_debug_sum_columns_f64.argtypes = [C.POINTER(C.c_double), C.c_longlong, C.c_int, C.POINTER(C.c_double)]
        L.ahip_debug_max_i32.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        L.ahip_debug_gemm_f32.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int,
                                          C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.ahip_comm_unique_id.argtypes = [C.c_char_p]
        L.ahip_comm_create_rccl.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ahip_comm_create_hosted.argtypes = [C.c_int, C.c_int, XFER_FN, C.c_void_p, C.POINTER(C.c_void_p)]
        L.ahip_comm_free.argtypes = [C.c_void_p]
        L.ahip_comm_free.restype = None
        L.ahip_comm_set_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        L.ahip_comm_set_plan_local.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.ahip_comm_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ahip_comm_reverse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ahip_comm_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ahip_comm_migrate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        L.ahip_comm_borders.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        L.ahip_comm_selftest.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ahip_comm_migrate_cell.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        L.ahip_comm_borders_cell.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                             C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        L.ahip_fill_zero_dev.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]

    def debug_fused_linear(self, W: np.ndarray, x: np.ndarray) -> np.ndarray:
        W = np.ascontiguousarray(W, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float32)
        K, N = W.shape
        assert x.shape == (32, K)
        out = np.zeros((32, N), dtype=np.float32)
        self.check(self.lib.ahip_debug_fused_linear(K, N, _p(W, C.c_double), _p(x, C.c_float), _p(out, C.c_float)))
        return out

    def debug_scan_i32(self, v: np.ndarray, warm_n: int = 0) -> np.ndarray:
        """exclusive prefix sum of v through prim_exclusive_scan_i32, [n + 1] (the last entry is the total); warm_n: a small scan first (scratch re-grow)"""
        v = np.ascontiguousarray(v, dtype=np.int32)
        out = np.full(len(v) + 1, -1, dtype=np.int32)
        self.check(self.lib.ahip_debug_scan_i32(_p(v, C.c_int), len(v), warm_n, _p(out, C.c_int)))
        return out

    def debug_sum_columns_f64(self, a: np.ndarray, ncol: Optional[int] = None) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float64)
        nrow, ncol = (a.shape[0], a.shape[1]) if ncol is None else (a.size // ncol, ncol)
        out = np.full(ncol, np.nan)
        self.check(self.lib.ahip_debug_sum_columns_f64(_p(a, C.c_double), nrow, ncol, _p(out, C.c_double)))
        return out

    def debug_max_i32(self, v: np.ndarray) -> int:
        v = np.ascontiguousarray(v, dtype=np.int32)
        out = np.full(1, -1, dtype=np.int32)
        self.check(self.lib.ahip_debug_max_i32(_p(v, C.c_int), len(v), _p(out, C.c_int)))
        return int(out[0])

    def debug_gemm_f32(self, E: int, K: int, N: int, A: np.ndarray, lda: int, a_off: int, W: np.ndarray, ldw: int, transB: bool, Cbuf: np.ndarray, ldc: int,
                       accumulate: bool, silu_out: Optional[np.ndarray] = None, dsilu_z: Optional[np.ndarray] = None) -> None:
        """gemm_f32 of the layer-at-a-time path on flat float32 buffers; Cbuf [E * ldc] and silu_out are updated in place"""
        for a in (A, W, Cbuf, silu_out, dsilu_z):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous)
        assert A.size >= a_off + (E - 1) * lda + K and W.size >= ((N if transB else K) - 1) * ldw + (K if transB else N)
        assert Cbuf.size == E * ldc and (silu_out is None or silu_out.size == E * ldc) and (dsilu_z is None or dsilu_z.size == E * ldc)
        self.check(self.lib.ahip_debug_gemm_f32(E, K, N, _p(A, C.c_float), lda, a_off, _p(W, C.c_float), ldw, int(transB), _p(Cbuf, C.c_float), ldc,
                                                int(accumulate), _p(silu_out, C.c_float), _p(dsilu_z, C.c_float)))

    def debug_md_noise(self, seed: int, step: int, n: int) -> np.ndarray:
        """xi of atoms 0 .. n-1 at one step [n][3], by the device function the Langevin move of ahip_md_cell uses (ahip_debug_md_noise)"""
        out = np.zeros((n, 3))
        self.lib.ahip_debug_md_noise.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.POINTER(C.c_double)]
        self.check(self.lib.ahip_debug_md_noise(int(seed), int(step), n, _p(out, C.c_double)))
        return out

    def debug_npt_noise(self, seed: int, step: int) -> float:
        """xi_V of one step, by the device function the decision of ahip_npt_cell uses (ahip_debug_npt_noise)"""
        out = np.zeros(1)
        self.lib.ahip_debug_npt_noise.argtypes = [C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_double)]
        self.check(self.lib.ahip_debug_npt_noise(int(seed), int(step), _p(out, C.c_double)))
        return float(out[0])

    def check(self, rc: int) -> None:
        if rc != 0:
            raise AhipError(rc, self.lib.ahip_last_error().decode(errors="replace"))

    def device_count(self) -> int:
        n = C.c_int(0)
        self.check(self.lib.ahip_device_count(C.byref(n)))
        return n.value


_default: Optional[Library] = None


def default_library() -> Library:
    global _default
    if _default is None:
        _default = Library()
    return _default


class Model:
    """Owning handle of an ahip_model."""

    def __init__(self, path: str, device: int = 0, lib: Optional[Library] = None):
        self.L = lib or default_library()
        h = C.c_void_p()
        self.L.check(self.L.lib.ahip_model_load(os.fsencode(path), device, C.byref(h)))
        self.h = h
        self._keep = []
        r = C.c_double(); nt = C.c_int(); tn = C.c_char_p(); pc = C.POINTER(C.c_double)()
        lm = C.c_int(); U = C.c_int(); S = C.c_int(); nl = C.c_int(); dt = C.c_char_p()
        self.L.check(self.L.lib.ahip_model_meta(h, C.byref(r), C.byref(nt), C.byref(tn), C.byref(pc), C.byref(lm),
                                                 C.byref(U), C.byref(S), C.byref(nl), C.byref(dt)))
        self.r_max = r.value
        self.num_types = nt.value
        self.type_names = tn.value.decode().split()
        self.per_edge_type_cutoff = (np.ctypeslib.as_array(pc, shape=(nt.value, nt.value)).copy() if pc else None)
        self.l_max, self.num_tensor_features, self.num_scalar_features = lm.value, U.value, S.value
        self.num_layers, self.model_dtype = nl.value, dt.value.decode()
        tf = C.c_int(0)
        self.L.check(self.L.lib.ahip_model_allow_tf32(h, C.byref(tf)))
        self.allow_tf32 = bool(tf.value)

    def close(self):
        if getattr(self, "h", None):
            self.L.lib.ahip_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key: str, value) -> None:
        self.L.check(self.L.lib.ahip_set_option(self.h, key.encode(), str(value).encode()))

    # ---- active types (include/allegro_hip.h: ahip_set_active_types) -------------------------------
    def set_active_types(self, model_types) -> None:
        """Name the model types in use explicitly (any order, repeats allowed); an empty list returns to the automatic rule."""
        t = np.ascontiguousarray(model_types, dtype=np.int32).reshape(-1)
        self.L.check(self.L.lib.ahip_set_active_types(self.h, len(t), _p(t, C.c_int) if len(t) else None))

    def get_active_types(self) -> list:
        """The model types the last evaluation's fused side was restricted to, ascending; [] = no subset."""
        n = C.c_int(0)
        out = np.zeros(max(self.num_types, 1), dtype=np.int32)
        self.L.check(self.L.lib.ahip_get_active_types(self.h, C.byref(n), _p(out, C.c_int)))
        return [int(v) for v in out[:n.value]]

    # ---- neighbor lists ----------------------------------------------------------------------
    def neigh_update_csr(self, nall: int, ilist: np.ndarray, offsets: np.ndarray, neigh: np.ndarray,
                         neighmask: int = 0x1FFFFFFF) -> None:
        ilist = np.ascontiguousarray(ilist, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        self.L.check(self.L.lib.ahip_neigh_update_csr(self.h, len(ilist), nall, _p(ilist, C.c_int),
                                                       _p(offsets, C.c_longlong), _p(neigh, C.c_int), neighmask))

    def neigh_update_paged(self, nall: int, ilist: np.ndarray, numneigh: np.ndarray, rows: Sequence[np.ndarray],
                           neighmask: int = 0x1FFFFFFF) -> None:
        """LAMMPS-shaped call: numneigh[i] and firstneigh[i] indexed by atom index."""
        ilist = np.ascontiguousarray(ilist, dtype=np.int32)
        numneigh = np.ascontiguousarray(numneigh, dtype=np.int32)
        rows = [np.ascontiguousarray(r, dtype=np.int32) for r in rows]
        first = (C.POINTER(C.c_int) * len(rows))(*[_p(r, C.c_int) for r in rows])
        self.L.check(self.L.lib.ahip_neigh_update(self.h, len(ilist), nall, _p(ilist, C.c_int), _p(numneigh, C.c_int),
                                                   first, neighmask))

    def neigh_update_dev(self, inum: int, nall: int, ilist_ptr: int, off_ptr: int, neigh_ptr: int, total: int) -> None:
        self.L.check(self.L.lib.ahip_neigh_update_dev(self.h, inum, nall, ilist_ptr, off_ptr, neigh_ptr, total))

    def neigh_update_dev_table(self, inum: int, nall: int, ilist_ptr: int, numneigh_ptr: int, table_ptr: int, stride_atom: int,
                               stride_slot: int, neighmask: int = 0x1FFFFFFF, stream: int = 0) -> None:
        """Device-resident KOKKOS-layout list (padded 2-D table) -> the library's CSR rows."""
        self.L.check(self.L.lib.ahip_neigh_update_dev_table(self.h, inum, nall, ilist_ptr, numneigh_ptr, table_ptr, stride_atom, stride_slot,
                                                             neighmask, stream))

    def map_types_dev(self, n: int, type_ptr: int, type_mapper: np.ndarray, mtype_ptr: int, stream: int = 0) -> None:
        tm = np.ascontiguousarray(type_mapper, dtype=np.int32)
        self.L.check(self.L.lib.ahip_map_types_dev(self.h, n, type_ptr, len(tm), _p(tm, C.c_int), mtype_ptr, stream))

    def reneighbor_flag_dev(self, n: int, x_ptr: int, xhold_ptr: int, v_ptr: int, dt: float, half_skin: float, flag_ptr: int, stream: int = 0) -> None:
        self.L.check(self.L.lib.ahip_reneighbor_flag_dev(self.h, n, x_ptr, xhold_ptr, v_ptr, dt, half_skin, flag_ptr, stream or None))

    def build_neighbors_dev(self, nlocal: int, nall: int, x_ptr: int, lo, hi, rc_list: float, stream: int = 0) -> None:
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        self.L.check(self.L.lib.ahip_build_neighbors_dev(self.h, nlocal, nall, x_ptr, _p(lo, C.c_double),
                                                          _p(hi, C.c_double), rc_list, stream))

    # ---- compute ------------------------------------------------------------------------------
    def compute(self, nlocal: int, nghost: int, x: np.ndarray, type_: np.ndarray, type_mapper: np.ndarray,
                cutoff_matrix: np.ndarray, f: np.ndarray, eatom: Optional[np.ndarray] = None, want_virial: bool = True):
        """f is accumulated in place; returns (eng, virial[6] or None)."""
        assert x.dtype == np.float64 and x.flags.c_contiguous and f.dtype == np.float64 and f.flags.c_contiguous
        type_ = np.ascontiguousarray(type_, dtype=np.int32)
        type_mapper = np.ascontiguousarray(type_mapper, dtype=np.int32)
        cutoff_matrix = np.ascontiguousarray(cutoff_matrix, dtype=np.float64)
        ntypes = len(type_mapper)
        eng = C.c_double(0)
        vir = np.zeros(6) if want_virial else None
        self.L.check(self.L.lib.ahip_compute(self.h, nlocal, nghost, _p(x, C.c_double), _p(type_, C.c_int), ntypes,
                                              _p(type_mapper, C.c_int), _p(cutoff_matrix, C.c_double),
                                              _p(f, C.c_double), _p(eatom, C.c_double), C.byref(eng),
                                              _p(vir, C.c_double)))
        return eng.value, vir

    def compute_dev(self, nlocal: int, nghost: int, x_ptr: int, mtype_ptr: int, f_ptr: int, eatom_ptr: int,
                    engvir_ptr: int, cutoff_matrix_model: Optional[np.ndarray] = None, stream: int = 0) -> None:
        cm = None
        if cutoff_matrix_model is not None:
            cm = np.ascontiguousarray(cutoff_matrix_model, dtype=np.float64)
        self.L.check(self.L.lib.ahip_compute_dev(self.h, nlocal, nghost, x_ptr, mtype_ptr, _p(cm, C.c_double), f_ptr,
                                                  eatom_ptr or None, engvir_ptr, stream or None))

    def compute_dev_range(self, c0: int, c1: int, nlocal: int, nghost: int, x_ptr: int, mtype_ptr: int, f_ptr: int, eatom_ptr: int,
                          engvir_ptr: int, cutoff_matrix_model: Optional[np.ndarray] = None, stream: int = 0) -> None:
        cm = None
        if cutoff_matrix_model is not None:
            cm = np.ascontiguousarray(cutoff_matrix_model, dtype=np.float64)
        self.L.check(self.L.lib.ahip_compute_dev_range(self.h, c0, c1, nlocal, nghost, x_ptr, mtype_ptr, _p(cm, C.c_double), f_ptr,
                                                        eatom_ptr or None, engvir_ptr, stream or None))

    def borders_local_dev(self, nlocal: int, x_ptr: int, mtype_ptr: int, lo, hi, box, rc: float, capacity: int, xg_ptr: int, mtg_ptr: int,
                          src_ptr: int, shift_ptr: int, stream: int = 0) -> int:
        """periodic images of a single rank's own atoms inside the halo (ahip_borders_local_dev); returns their number (> capacity: retry with larger arrays)"""
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, box)]
        ng = C.c_int(0)
        self.L.lib.ahip_borders_local_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                      C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        self.L.check(self.L.lib.ahip_borders_local_dev(self.h, nlocal, x_ptr or None, mtype_ptr or None, _p(a[0], C.c_double), _p(a[1], C.c_double), _p(a[2], C.c_double),
                                                        float(rc), capacity, xg_ptr or None, mtg_ptr or None, src_ptr or None, shift_ptr or None, C.byref(ng), stream or None))
        return int(ng.value)

    # ---- any periodic cell (include/allegro_hip.h: cell = rows of lattice vectors, pbc = three flags) ----------
    @staticmethod
    def _cell_args(cell, pbc):
        c = np.ascontiguousarray(cell, dtype=np.float64)
        if c.shape != (3, 3):
            raise ValueError(f"cell must be a 3x3 matrix of lattice vectors (rows), got shape {c.shape}")
        p = np.ascontiguousarray([1 if b else 0 for b in pbc], dtype=np.int32)
        if p.shape != (3,):
            raise ValueError("pbc must have three entries")
        return c, p

    def wrap_cell_dev(self, n: int, x_ptr: int, cell, pbc=(True, True, True), stream: int = 0) -> None:
        """positions back into the cell along its periodic axes, in place, no host synchronisation (ahip_wrap_cell_dev)"""
        c, p = self._cell_args(cell, pbc)
        self.L.lib.ahip_wrap_cell_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p]
        self.L.check(self.L.lib.ahip_wrap_cell_dev(self.h, n, x_ptr or None, _p(c, C.c_double), _p(p, C.c_int), stream or None))

    def borders_cell_dev(self, nlocal: int, x_ptr: int, mtype_ptr: int, cell, pbc, rc: float, capacity: int, xg_ptr: int, mtg_ptr: int,
                         src_ptr: int, shift_ptr: int, stream: int = 0) -> int:
        """periodic images of a single rank's own atoms within rc of a general cell (ahip_borders_cell_dev); returns their number (> capacity: retry with larger arrays)"""
        c, p = self._cell_args(cell, pbc)
        ng = C.c_int(0)
        self.L.lib.ahip_borders_cell_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_double, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        self.L.check(self.L.lib.ahip_borders_cell_dev(self.h, nlocal, x_ptr or None, mtype_ptr or None, _p(c, C.c_double), _p(p, C.c_int), float(rc), capacity,
                                                       xg_ptr or None, mtg_ptr or None, src_ptr or None, shift_ptr or None, C.byref(ng), stream or None))
        return int(ng.value)

    def compute_cell(self, x: np.ndarray, mtype: np.ndarray, cell, pbc=(True, True, True), skin: float = 0.0, want_eatom: bool = True):
        """One evaluation from host arrays (ahip_compute_cell): returns (energy, forces [n][3], atomic energies [n] or None, virial [6])."""
        c, p = self._cell_args(cell, pbc)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        if len(mt) != len(x):
            raise ValueError("positions and types differ in length")
        n = len(x)
        f = np.zeros((n, 3))
        ea = np.zeros(n) if want_eatom else None
        eng = C.c_double(0)
        vir = np.zeros(6)
        self.L.lib.ahip_compute_cell.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_double,
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        self.L.check(self.L.lib.ahip_compute_cell(self.h, n, _p(x, C.c_double), _p(mt, C.c_int), _p(c, C.c_double), _p(p, C.c_int), float(skin),
                                                   _p(f, C.c_double), _p(ea, C.c_double), C.byref(eng), _p(vir, C.c_double)))
        return eng.value, f, ea, vir

    def compute_cell_reuse(self, x: np.ndarray, mtype: np.ndarray, cell, pbc=(True, True, True), skin: float = 1.0, want_eatom: bool = True):
        """compute_cell that keeps ghosts and neighbor list from call to call (ahip_compute_cell_reuse) and rebuilds them only when the criterion of
        include/allegro_hip.h says the held list may miss a pair.  Returns (energy, forces, atomic energies or None, virial [6], rebuilt)."""
        c, p = self._cell_args(cell, pbc)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        if len(mt) != len(x):
            raise ValueError("positions and types differ in length")
        n = len(x)
        f = np.zeros((n, 3))
        ea = np.zeros(n) if want_eatom else None
        eng = C.c_double(0)
        vir = np.zeros(6)
        rebuilt = C.c_int(-1)
        self.L.lib.ahip_compute_cell_reuse.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_double,
                                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        self.L.check(self.L.lib.ahip_compute_cell_reuse(self.h, n, _p(x, C.c_double), _p(mt, C.c_int), _p(c, C.c_double), _p(p, C.c_int), float(skin),
                                                         _p(f, C.c_double), _p(ea, C.c_double), C.byref(eng), _p(vir, C.c_double), C.byref(rebuilt)))
        return eng.value, f, ea, vir, bool(rebuilt.value)

    def relax_params(self, **fire) -> RelaxParams:
        """the library's defaults (ahip_relax_params_default) with the named fields replaced; an unknown name is a TypeError"""
        p = RelaxParams()
        self.L.lib.ahip_relax_params_default.argtypes = [C.POINTER(RelaxParams)]
        self.L.check(self.L.lib.ahip_relax_params_default(C.byref(p)))
        names = {n for n, _ in RelaxParams._fields_}
        for k, v in fire.items():
            if k not in names:
                raise TypeError(f"unknown FIRE parameter {k!r} (known: {', '.join(n for n, _ in RelaxParams._fields_)})")
            setattr(p, k, v)
        return p

    def relax_cell(self, x: np.ndarray, mtype: np.ndarray, cell, pbc=(True, True, True), skin: float = 1.0, fixed=None, want_eatom: bool = True,
                   x_inout: Optional[np.ndarray] = None, f: Optional[np.ndarray] = None, **fire):
        """FIRE relaxation at fixed cell on the device (ahip_relax_cell).  `fire`: fields of ahip_relax_params (fmax, max_steps, check_every, dt_start, ...).
        Returns (positions, energy, forces, atomic energies or None, virial [6], info) with info = dict(steps, converged, fmax, evaluations, rebuilds).  The
        positions are never wrapped.  `x_inout` / `f` (C-contiguous float64 [n][3]): the arrays the library itself reads and writes, instead of copies of `x`."""
        c, p = self._cell_args(cell, pbc)
        xr = np.array(x, dtype=np.float64).reshape(-1, 3) if x_inout is None else x_inout
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        n = len(xr)
        if len(mt) != n:
            raise ValueError("positions and types differ in length")
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.int32).reshape(-1)
            if len(fx) != n:
                raise ValueError("positions and the fixed mask differ in length")
        f = np.zeros((n, 3)) if f is None else f
        for a in (xr, f):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != (n, 3):
                raise ValueError("x_inout and f must be C-contiguous float64 arrays of shape [n][3]")
        par = self.relax_params(**fire)
        ea = np.zeros(n) if want_eatom else None
        eng, fmax = C.c_double(0), C.c_double(0)
        vir = np.zeros(6)
        steps, conv, nev, nreb = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self.L.lib.ahip_relax_cell.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_double,
                                               C.POINTER(C.c_int), C.POINTER(RelaxParams), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.L.check(self.L.lib.ahip_relax_cell(self.h, n, _p(xr, C.c_double), _p(mt, C.c_int), _p(c, C.c_double), _p(p, C.c_int), float(skin), _p(fx, C.c_int),
                                                 C.byref(par), _p(f, C.c_double), _p(ea, C.c_double), C.byref(eng), _p(vir, C.c_double), C.byref(steps),
                                                 C.byref(conv), C.byref(fmax), C.byref(nev), C.byref(nreb)))
        info = dict(steps=steps.value, converged=bool(conv.value), fmax=fmax.value, evaluations=nev.value, rebuilds=nreb.value)
        return xr, eng.value, f, ea, vir, info

    def vcell_params(self, **par) -> VcellParams:
        """the library's defaults (ahip_vcell_params_default) with the named fields replaced: those of ahip_vcell_params (smax, pressure, cell_factor,
        hydrostatic, mask) and those of its ahip_relax_params; an unknown name is a TypeError"""
        p = VcellParams()
        self.L.lib.ahip_vcell_params_default.argtypes = [C.POINTER(VcellParams)]
        self.L.check(self.L.lib.ahip_vcell_params_default(C.byref(p)))
        fire = {n for n, _ in RelaxParams._fields_}
        own = {n for n, _ in VcellParams._fields_} - {"fire"}
        for k, v in par.items():
            if k == "mask":
                v = [int(bool(e)) for e in v]
                if len(v) != 6:
                    raise ValueError("mask has six flags: xx, yy, zz, xy, xz, yz")
                p.mask = (C.c_int * 6)(*v)
            elif k in own:
                setattr(p, k, v)
            elif k in fire:
                setattr(p.fire, k, v)
            else:
                raise TypeError(f"unknown relaxation parameter {k!r} (known: {', '.join(sorted(own | fire))})")
        return p

    def relax_vcell(self, x: np.ndarray, mtype: np.ndarray, cell, pbc=(True, True, True), skin: float = 1.0, fixed=None, want_eatom: bool = True,
                    x_inout: Optional[np.ndarray] = None, f: Optional[np.ndarray] = None, params: Optional[VcellParams] = None, **par):
        """FIRE relaxation of positions and cell on the device (ahip_relax_vcell).  `par`: fields of ahip_vcell_params and of its ahip_relax_params (fmax, smax,
        pressure, mask, hydrostatic, cell_factor, max_steps, check_every, dt_start, ...); `params`: a ready VcellParams instead, or False for a NULL pointer.  Returns (positions, energy, forces, atomic energies or None, virial [6],
        info, cell [3][3]) with info = dict(steps, converged, fmax, smax, evaluations, rebuilds).  The positions are never wrapped."""
        c, p = self._cell_args(cell, pbc)
        xr = np.array(x, dtype=np.float64).reshape(-1, 3) if x_inout is None else x_inout
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        n = len(xr)
        if len(mt) != n:
            raise ValueError("positions and types differ in length")
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.int32).reshape(-1)
            if len(fx) != n:
                raise ValueError("positions and the fixed mask differ in length")
        f = np.zeros((n, 3)) if f is None else f
        for a in (xr, f):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != (n, 3):
                raise ValueError("x_inout and f must be C-contiguous float64 arrays of shape [n][3]")
        par_p = C.byref(self.vcell_params(**par)) if params is None else (None if params is False else C.byref(params))
        ea = np.zeros(n) if want_eatom else None
        eng, fmax, smax = C.c_double(0), C.c_double(0), C.c_double(0)
        vir, cell_out = np.zeros(6), np.zeros((3, 3))
        steps, conv, nev, nreb = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
        self.L.lib.ahip_relax_vcell.argtypes = [C.c_void_p, C.c_int, D, I, D, I, C.c_double, I, C.POINTER(VcellParams), D, D, D, D, D, I, I, D, D, I, I]
        self.L.check(self.L.lib.ahip_relax_vcell(self.h, n, _p(xr, C.c_double), _p(mt, C.c_int), _p(c, C.c_double), _p(p, C.c_int), float(skin), _p(fx, C.c_int),
                                                  par_p, _p(cell_out, C.c_double), _p(f, C.c_double), _p(ea, C.c_double), C.byref(eng), _p(vir, C.c_double),
                                                  C.byref(steps), C.byref(conv), C.byref(fmax), C.byref(smax), C.byref(nev), C.byref(nreb)))
        info = dict(steps=steps.value, converged=bool(conv.value), fmax=fmax.value, smax=smax.value, evaluations=nev.value, rebuilds=nreb.value)
        return xr, eng.value, f, ea, vir, info, cell_out

    def md_params(self, **par) -> MdParams:
        """the library's defaults (ahip_md_params_default) with the named fields replaced; an unknown name is a TypeError"""
        p = MdParams()
        self.L.lib.ahip_md_params_default.argtypes = [C.POINTER(MdParams)]
        self.L.check(self.L.lib.ahip_md_params_default(C.byref(p)))
        names = {n for n, _ in MdParams._fields_}
        for k, v in par.items():
            if k not in names:
                raise TypeError(f"unknown MD parameter {k!r} (known: {', '.join(n for n, _ in MdParams._fields_)})")
            setattr(p, k, v)
        return p

    def md_cell(self, x: np.ndarray, v: np.ndarray, mtype: np.ndarray, mass: np.ndarray, cell, pbc=(True, True, True), skin: float = 1.0, fixed=None,
                want_eatom: bool = True, want_thermo: bool = True, x_inout: Optional[np.ndarray] = None, v_inout: Optional[np.ndarray] = None,
                f: Optional[np.ndarray] = None, params=None, **par):
        """MD on the device (ahip_md_cell): NVE, or Langevin dynamics by BAOAB when gamma > 0.  `par`: fields of ahip_md_params (nsteps, dt, gamma, kT, seed, step0,
        check_every, sample_every, frame_every, ftm2v, mvv2e); `params`: a ready MdParams instead, or False for a NULL pointer.  Returns (x, v, energy, forces,
        atomic energies or None, virial [6], thermo [nsteps / sample_every + 1][8] or None, frames [nsteps / frame_every + 1][n][3] or None, info) with info =
        dict(steps, evaluations, rebuilds).  The positions are never wrapped.  `x_inout` / `v_inout` / `f` (C-contiguous float64 [n][3]): the arrays the library
        itself reads and writes, instead of copies of `x` and `v`."""
        c, p = self._cell_args(cell, pbc)
        xr = np.array(x, dtype=np.float64).reshape(-1, 3) if x_inout is None else x_inout
        vr = np.array(v, dtype=np.float64).reshape(-1, 3) if v_inout is None else v_inout
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        ms = np.ascontiguousarray(mass, dtype=np.float64).reshape(-1)
        n = len(xr)
        if len(mt) != n or len(ms) != n:
            raise ValueError("positions, types and masses differ in length")
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.int32).reshape(-1)
            if len(fx) != n:
                raise ValueError("positions and the fixed mask differ in length")
        f = np.zeros((n, 3)) if f is None else f
        for a in (xr, vr, f):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != (n, 3):
                raise ValueError("x_inout, v_inout and f must be C-contiguous float64 arrays of shape [n][3]")
        mp = self.md_params(**par) if params is None else params
        if mp is False:
            mp_ref, thermo, frames, nsteps = None, None, None, 0
        else:
            mp_ref, nsteps = C.byref(mp), int(mp.nsteps)
            ok = nsteps >= 0 and mp.sample_every >= 1 and mp.frame_every >= 0          # (a range the library refuses: no buffer can be sized, it gets none)
            thermo = np.zeros((nsteps // mp.sample_every + 1, 8)) if want_thermo and ok else None
            frames = np.zeros((nsteps // mp.frame_every + 1, n, 3)) if ok and mp.frame_every > 0 else None
        ea = np.zeros(n) if want_eatom else None
        eng = C.c_double(0)
        vir = np.zeros(6)
        nev, nreb = C.c_int(0), C.c_int(0)
        D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
        self.L.lib.ahip_md_cell.argtypes = [C.c_void_p, C.c_int, D, D, I, D, D, I, C.c_double, I, C.POINTER(MdParams), D, D, D, D, D, D, I, I]
        self.L.check(self.L.lib.ahip_md_cell(self.h, n, _p(xr, C.c_double), _p(vr, C.c_double), _p(mt, C.c_int), _p(ms, C.c_double), _p(c, C.c_double), _p(p, C.c_int),
                                              float(skin), _p(fx, C.c_int), mp_ref, _p(f, C.c_double), _p(ea, C.c_double), C.byref(eng), _p(vir, C.c_double),
                                              _p(thermo, C.c_double), _p(frames, C.c_double), C.byref(nev), C.byref(nreb)))
        info = dict(steps=nsteps, evaluations=nev.value, rebuilds=nreb.value)
        return xr, vr, eng.value, f, ea, vir, thermo, frames, info

    def debug_md_noise(self, seed: int, step: int, n: int) -> np.ndarray:
        """xi of atoms 0 .. n-1 at one step [n][3], by the device function the Langevin move uses (ahip_debug_md_noise; the call needs no model)"""
        return self.L.debug_md_noise(seed, step, n)

    def npt_params(self, **par) -> NptParams:
        """the library's defaults (ahip_npt_params_default) with the named fields replaced: pressure, compressibility, tau_p and those of its ahip_md_params; an
        unknown name is a TypeError"""
        p = NptParams()
        self.L.lib.ahip_npt_params_default.argtypes = [C.POINTER(NptParams)]
        self.L.check(self.L.lib.ahip_npt_params_default(C.byref(p)))
        md = {n for n, _ in MdParams._fields_}
        own = {n for n, _ in NptParams._fields_} - {"md"}
        for k, v in par.items():
            if k in own:
                setattr(p, k, v)
            elif k in md:
                setattr(p.md, k, v)
            else:
                raise TypeError(f"unknown NPT parameter {k!r} (known: {', '.join(sorted(own | md))})")
        return p

    def npt_cell(self, x: np.ndarray, v: np.ndarray, mtype: np.ndarray, mass: np.ndarray, cell, pbc=(True, True, True), skin: float = 1.0, fixed=None,
                 want_eatom: bool = True, want_thermo: bool = True, want_frame_cells: bool = True, x_inout: Optional[np.ndarray] = None,
                 v_inout: Optional[np.ndarray] = None, f: Optional[np.ndarray] = None, cell_out: Optional[np.ndarray] = None, params=None, **par):
        """MD at constant pressure on the device (ahip_npt_cell): the BAOAB of md_cell inside an isotropic stochastic cell rescaling.  `par`: pressure,
        compressibility, tau_p and the fields of ahip_md_params; `params`: a ready NptParams instead, or False for a NULL pointer.  Returns (x, v, energy, forces,
        atomic energies or None, virial [6], thermo [nsteps / sample_every + 1][10] or None, frames or None, info, cell [3][3], frame_cells [.][3][3] or None) with
        info = dict(steps, evaluations, rebuilds).  The positions are never wrapped.  `x_inout` / `v_inout` / `f` / `cell_out`: the arrays the library itself reads
        and writes; `cell_out=False` passes a NULL pointer."""
        c, p = self._cell_args(cell, pbc)
        xr = np.array(x, dtype=np.float64).reshape(-1, 3) if x_inout is None else x_inout
        vr = np.array(v, dtype=np.float64).reshape(-1, 3) if v_inout is None else v_inout
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        ms = np.ascontiguousarray(mass, dtype=np.float64).reshape(-1)
        n = len(xr)
        if len(mt) != n or len(ms) != n:
            raise ValueError("positions, types and masses differ in length")
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.int32).reshape(-1)
            if len(fx) != n:
                raise ValueError("positions and the fixed mask differ in length")
        f = np.zeros((n, 3)) if f is None else f
        for a in (xr, vr, f):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != (n, 3):
                raise ValueError("x_inout, v_inout and f must be C-contiguous float64 arrays of shape [n][3]")
        co = None if cell_out is False else (np.zeros((3, 3)) if cell_out is None else cell_out)
        if co is not None and (co.dtype != np.float64 or not co.flags.c_contiguous or co.shape != (3, 3)):
            raise ValueError("cell_out must be a C-contiguous float64 array of shape [3][3]")
        mp = self.npt_params(**par) if params is None else params
        if mp is False:
            mp_ref, thermo, frames, fcells, nsteps = None, None, None, None, 0
        else:
            mp_ref, nsteps, md = C.byref(mp), int(mp.md.nsteps), mp.md
            ok = nsteps >= 0 and md.sample_every >= 1 and md.frame_every >= 0          # (a range the library refuses: no buffer can be sized, it gets none)
            thermo = np.zeros((nsteps // md.sample_every + 1, 10)) if want_thermo and ok else None
            frames = np.zeros((nsteps // md.frame_every + 1, n, 3)) if ok and md.frame_every > 0 else None
            fcells = np.zeros((nsteps // md.frame_every + 1, 3, 3)) if ok and md.frame_every > 0 and want_frame_cells else None
        ea = np.zeros(n) if want_eatom else None
        eng = C.c_double(0)
        vir = np.zeros(6)
        nev, nreb = C.c_int(0), C.c_int(0)
        D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
        self.L.lib.ahip_npt_cell.argtypes = [C.c_void_p, C.c_int, D, D, I, D, D, I, C.c_double, I, C.POINTER(NptParams), D, D, D, D, D, D, D, D, I, I]
        self.L.check(self.L.lib.ahip_npt_cell(self.h, n, _p(xr, C.c_double), _p(vr, C.c_double), _p(mt, C.c_int), _p(ms, C.c_double), _p(c, C.c_double), _p(p, C.c_int),
                                               float(skin), _p(fx, C.c_int), mp_ref, _p(co, C.c_double), _p(f, C.c_double), _p(ea, C.c_double), C.byref(eng),
                                               _p(vir, C.c_double), _p(thermo, C.c_double), _p(frames, C.c_double), _p(fcells, C.c_double), C.byref(nev), C.byref(nreb)))
        info = dict(steps=nsteps, evaluations=nev.value, rebuilds=nreb.value)
        return xr, vr, eng.value, f, ea, vir, thermo, frames, info, co, fcells

    def debug_npt_noise(self, seed: int, step: int) -> float:
        """xi_V of one step (ahip_debug_npt_noise; the call needs no model)"""
        return self.L.debug_npt_noise(seed, step)

    def cell_reuse_reset(self) -> None:
        """drop the held list (and the counters): the next compute_cell_reuse rebuilds"""
        self.L.lib.ahip_cell_reuse_reset.argtypes = [C.c_void_p]
        self.L.check(self.L.lib.ahip_cell_reuse_reset(self.h))

    def cell_reuse_stats(self):
        """(successful compute_cell_reuse calls, how many of them rebuilt) since the model was loaded or cell_reuse_reset was called"""
        a = C.c_longlong(0); b = C.c_longlong(0)
        self.L.lib.ahip_cell_reuse_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        self.L.check(self.L.lib.ahip_cell_reuse_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_cell_rows(self) -> np.ndarray:
        """atom index of every row (atoms, then ghosts) of the last compute_cell (ahip_last_cell_rows)"""
        n = C.c_int(0)
        self.L.lib.ahip_last_cell_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        self.L.check(self.L.lib.ahip_last_cell_rows(self.h, C.byref(n), None))
        out = np.zeros(n.value, dtype=np.int64)
        if n.value:
            self.L.check(self.L.lib.ahip_last_cell_rows(self.h, C.byref(n), _p(out, C.c_longlong)))
        return out

    def compute_cells(self, first, x: np.ndarray, mtype: np.ndarray, cells, pbc, skin: float = 0.0, want_eatom: bool = True, f: Optional[np.ndarray] = None):
        """A batch of structures in one call (ahip_compute_cells).  `first` [B + 1] (first[0] = 0, non-decreasing): structure s owns the atoms first[s] .. first[s+1] - 1
        of `x` / `mtype`; `cells` [B][3][3] (rows are lattice vectors), `pbc` [B][3].  Returns (energies [B], forces [n][3], atomic energies [n] or None, virials [B][6]).
        `f`: an own C-contiguous float64 [n][3] array to receive the forces (an argument error leaves it as it was)."""
        first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        if len(first) < 1:
            raise ValueError("first needs at least one entry (first[0] = 0)")
        B = len(first) - 1
        c = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1)
        p = np.ascontiguousarray(np.asarray(pbc).astype(bool), dtype=np.int32).reshape(-1)
        if c.size != 9 * B or p.size != 3 * B:
            raise ValueError(f"cells must be [{B}][3][3] and pbc [{B}][3]")
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
        mt = np.ascontiguousarray(mtype, dtype=np.int32).reshape(-1)
        if len(mt) != len(x) or len(x) != max(int(first[-1]), 0):
            raise ValueError("positions, types and first[-1] differ in length")
        n = len(x)
        if f is None:
            f = np.zeros((n, 3))
        elif f.dtype != np.float64 or f.shape != (n, 3) or not f.flags.c_contiguous:
            raise ValueError("f must be a C-contiguous float64 array of shape [n][3]")
        ea = np.zeros(n) if want_eatom else None
        eng = np.zeros(B)
        vir = np.zeros((B, 6))
        self.L.lib.ahip_compute_cells.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                                  C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        self.L.check(self.L.lib.ahip_compute_cells(self.h, B, _p(first, C.c_int), _p(x, C.c_double), _p(mt, C.c_int), _p(c, C.c_double), _p(p, C.c_int), float(skin),
                                                    _p(f, C.c_double), _p(ea, C.c_double), _p(eng, C.c_double), _p(vir, C.c_double)))
        return eng, f, ea, vir

    def last_cells_ghosts(self) -> np.ndarray:
        """ghost images per structure of the last compute_cells (ahip_last_cells_ghosts)"""
        n = C.c_int(0)
        self.L.lib.ahip_last_cells_ghosts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        self.L.check(self.L.lib.ahip_last_cells_ghosts(self.h, C.byref(n), None))
        out = np.zeros(n.value, dtype=np.int64)
        if n.value:
            self.L.check(self.L.lib.ahip_last_cells_ghosts(self.h, C.byref(n), _p(out, C.c_longlong)))
        return out

    def nve_dev(self, mode: int, n: int, x_ptr: int, v_ptr: int, f_ptr: int, mtype_ptr: int, mass_by_mtype,
                dt: float, ftm2v: float, stream: int = 0) -> None:
        mass = np.ascontiguousarray(mass_by_mtype, dtype=np.float64)
        self.L.check(self.L.lib.ahip_nve_dev(self.h, mode, n, x_ptr, v_ptr, f_ptr, mtype_ptr, _p(mass, C.c_double),
                                              dt, ftm2v, stream or None))

    def nve_first_dev(self, nlocal: int, nall: int, x_ptr: int, v_ptr: int, f_ptr: int, mtype_ptr: int, mass_by_mtype,
                      dt: float, ftm2v: float, stream: int = 0) -> None:
        mass = np.ascontiguousarray(mass_by_mtype, dtype=np.float64)
        self.L.lib.ahip_nve_first_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_double), C.c_double, C.c_double, C.c_void_p]
        self.L.check(self.L.lib.ahip_nve_first_dev(self.h, nlocal, nall, x_ptr, v_ptr, f_ptr, mtype_ptr, _p(mass, C.c_double),
                                                    dt, ftm2v, stream or None))

    # ---- introspection -----------------------------------------------------------------------
    def nedges(self) -> int:
        n = C.c_longlong(0)
        self.L.check(self.L.lib.ahip_get_edges(self.h, C.byref(n), None, None))
        return int(n.value)

    def nneigh(self) -> int:
        return int(self.L.lib.ahip_last_list_size(self.h))

    def get_edges(self):
        n = C.c_longlong(0)
        self.L.check(self.L.lib.ahip_get_edges(self.h, C.byref(n), None, None))
        E = n.value
        ei = np.zeros((2, E), dtype=np.int64)
        r = np.zeros(E)
        if E:
            self.L.check(self.L.lib.ahip_get_edges(self.h, C.byref(n), _p(ei, C.c_longlong), _p(r, C.c_double)))
        return ei, r

    def debug_dump_edges(self, tag: Optional[np.ndarray] = None) -> None:
        t = np.ascontiguousarray(tag, dtype=np.int32) if tag is not None else None
        self.L.check(self.L.lib.ahip_debug_dump_edges(self.h, _p(t, C.c_int)))

    def timings(self) -> dict:
        names = C.c_char_p(); ms = C.POINTER(C.c_double)(); n = C.c_int(0)
        self.L.check(self.L.lib.ahip_get_timings(self.h, C.byref(names), C.byref(ms), C.byref(n)))
        if n.value == 0:
            return {}
        return dict(zip(names.value.decode().split(";"), [ms[k] for k in range(n.value)]))

    def tile_occupancy(self):
        """(slots holding an edge, slots of all tiles) of the last fused evaluation."""
        a = C.c_longlong(0); b = C.c_longlong(0)
        self.L.lib.ahip_last_tile_occupancy.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        self.L.check(self.L.lib.ahip_last_tile_occupancy(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timings_and_counts(self):
        """({stage: summed ms}, {stage: launches}) since the previous timings() / timings_and_counts() call."""
        names = C.c_char_p(); ms = C.POINTER(C.c_double)(); n = C.c_int(0)
        self.L.check(self.L.lib.ahip_get_timings(self.h, C.byref(names), C.byref(ms), C.byref(n)))
        if n.value == 0:
            return {}, {}
        cnt = C.POINTER(C.c_double)(); n2 = C.c_int(0)
        self.L.check(self.L.lib.ahip_get_timing_counts(self.h, C.byref(cnt), C.byref(n2)))
        keys = names.value.decode().split(";")
        return dict(zip(keys, [ms[k] for k in range(n.value)])), dict(zip(keys, [int(cnt[k]) for k in range(n2.value)]))

    @property
    def last_path(self) -> str:
        return self.L.lib.ahip_last_path(self.h).decode()

    @property
    def arith_note(self) -> str:
        """What fused_arith=auto decided for this model and why (empty before the first evaluation)."""
        return self.L.lib.ahip_arith_note(self.h).decode()

    @property
    def last_max_degree(self) -> int:
        return int(self.L.lib.ahip_last_max_degree(self.h))

    @property
    def last_heavy_centres(self):
        """(centres, their edges) the last evaluation handed to the layer-at-a-time kernels beside a fused kernel; (0, 0) when none or not a fused path."""
        n = C.c_int(0); e = C.c_longlong(0)
        self.L.check(self.L.lib.ahip_last_heavy_centres(self.h, C.byref(n), C.byref(e)))
        return n.value, e.value

    # ---- `compute allegro` outputs (pair_nequip_allegro.cpp:403-406,681-684) ---------------------
    def output_register(self, name: str) -> None:
        self.L.check(self.L.lib.ahip_output_register(self.h, name.encode()))

    def output_get(self, name: str) -> np.ndarray:
        n = C.c_longlong(0)
        self.L.check(self.L.lib.ahip_output_get(self.h, name.encode(), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float64)
        self.L.check(self.L.lib.ahip_output_get(self.h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return out


class Comm:
    """Owning handle of an ahip_comm: the ghost exchange of a decomposed system (csrc/comm.hip).  Transports: "rccl" (unique id from
    rank 0, handed over by the caller) or "hosted" (a Python callable moves the packed buffers: CPU tests, ranks sharing one GPU)."""

    def __init__(self, lib: Library, rank: int, nranks: int, rccl_id: Optional[bytes] = None, device: int = 0, xfer=None):
        self.L = lib
        self.rank, self.nranks = rank, nranks
        self.h = C.c_void_p()
        self._keep = []
        self._cb = None
        if rccl_id is not None:
            assert len(rccl_id) == 128
            self.L.check(self.L.lib.ahip_comm_create_rccl(rank, nranks, rccl_id, device, C.byref(self.h)))
            self.transport = "rccl"
        else:
            if xfer is not None:
                def _cb(user, nops, ops):
                    try:
                        xfer([(ops[k].kind, ops[k].peer, ops[k].ptr, ops[k].bytes) for k in range(nops)])
                        return 0
                    except Exception as e:          # never let an exception cross the C boundary
                        import traceback
                        traceback.print_exc()
                        return 1
                self._cb = XFER_FN(_cb)
            else:
                self._cb = C.cast(None, XFER_FN)
            self.L.check(self.L.lib.ahip_comm_create_hosted(rank, nranks, self._cb, None, C.byref(self.h)))
            self.transport = "hosted"

    @staticmethod
    def unique_id(lib: Library) -> bytes:
        buf = C.create_string_buffer(128)
        lib.check(lib.lib.ahip_comm_unique_id(buf))
        return buf.raw

    def close(self):
        if getattr(self, "h", None):
            self.L.lib.ahip_comm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_plan(self, dims, sendranks, recvranks, shifts, nsend, nrecv, first_recv, idx_ptrs) -> None:
        n = len(dims)
        ai = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        a = [ai(dims), ai(sendranks), ai(recvranks), np.ascontiguousarray(shifts, dtype=np.float64), ai(nsend), ai(nrecv), ai(first_recv)]
        ptrs = (C.c_void_p * max(n, 1))(*[int(p) for p in idx_ptrs])
        self._keep = a + [ptrs]
        self.L.check(self.L.lib.ahip_comm_set_plan(self.h, n, _p(a[0], C.c_int), _p(a[1], C.c_int), _p(a[2], C.c_int), _p(a[3], C.c_double),
                                                   _p(a[4], C.c_int), _p(a[5], C.c_int), _p(a[6], C.c_int), ptrs))

    def set_plan_local(self, nlocal: int, nghost: int, src_ptr: int, shift_ptr: int) -> None:
        self.L.check(self.L.lib.ahip_comm_set_plan_local(self.h, nlocal, nghost, src_ptr or None, shift_ptr or None))

    def forward(self, x_ptr: int, stream: int = 0) -> None:
        self.L.check(self.L.lib.ahip_comm_forward(self.h, x_ptr, stream or None))

    def reverse(self, f_ptr: int, stream: int = 0) -> None:
        self.L.check(self.L.lib.ahip_comm_reverse(self.h, f_ptr, stream or None))

    def migrate(self, nlocal: int, x_ptr: int, v_ptr: int, tag_ptr: int, mtype_ptr: int, capacity: int, box, grid, coord, stream: int = 0) -> int:
        """Comm::exchange inside the library (csrc/comm.hip: comm_migrate); returns the new owned count, negative = rows some brick would need."""
        b = np.ascontiguousarray(box, dtype=np.float64); g = np.ascontiguousarray(grid, dtype=np.int32); c = np.ascontiguousarray(coord, dtype=np.int32)
        out = C.c_int(0)
        self.L.check(self.L.lib.ahip_comm_migrate(self.h, nlocal, C.c_void_p(x_ptr), C.c_void_p(v_ptr), C.c_void_p(tag_ptr), C.c_void_p(mtype_ptr), capacity,
                                                  _p(b, C.c_double), _p(g, C.c_int), _p(c, C.c_int), C.byref(out), stream or None))
        return out.value

    def borders(self, nlocal: int, x_ptr: int, mtype_ptr: int, capacity: int, lo, hi, box, rc: float, grid, coord, stream: int = 0) -> int:
        """Comm::borders inside the library (comm_borders): ghosts behind the owned rows, the exchange plan installed; returns owned + ghost rows (> capacity: retry)."""
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, box)]
        g = np.ascontiguousarray(grid, dtype=np.int32); c = np.ascontiguousarray(coord, dtype=np.int32)
        out = C.c_int(0)
        self.L.check(self.L.lib.ahip_comm_borders(self.h, nlocal, C.c_void_p(x_ptr), C.c_void_p(mtype_ptr), capacity, _p(a[0], C.c_double), _p(a[1], C.c_double),
                                                  _p(a[2], C.c_double), float(rc), _p(g, C.c_int), _p(c, C.c_int), C.byref(out), stream or None))
        return out.value

    def migrate_cell(self, nlocal: int, x_ptr: int, v_ptr: int, tag_ptr: int, mtype_ptr: int, capacity: int, cell, pbc, grid, coord, stream: int = 0) -> int:
        """Comm::exchange for any cell, bricks of fractional coordinates (ahip_comm_migrate_cell); returns the new owned count, negative = rows some brick would need."""
        h = np.ascontiguousarray(cell, dtype=np.float64).reshape(9); p = np.ascontiguousarray([1 if b else 0 for b in pbc], dtype=np.int32)
        g = np.ascontiguousarray(grid, dtype=np.int32); c = np.ascontiguousarray(coord, dtype=np.int32)
        out = C.c_int(0)
        self.L.check(self.L.lib.ahip_comm_migrate_cell(self.h, nlocal, C.c_void_p(x_ptr), C.c_void_p(v_ptr), C.c_void_p(tag_ptr), C.c_void_p(mtype_ptr), capacity,
                                                       _p(h, C.c_double), _p(p, C.c_int), _p(g, C.c_int), _p(c, C.c_int), C.byref(out), stream or None))
        return out.value

    def borders_cell(self, nlocal: int, x_ptr: int, mtype_ptr: int, capacity: int, cell, pbc, rc: float, grid, coord, stream: int = 0) -> int:
        """Comm::borders for any cell (ahip_comm_borders_cell): ghosts behind the owned rows, the exchange plan installed; returns owned + ghost rows (> capacity: retry)."""
        h = np.ascontiguousarray(cell, dtype=np.float64).reshape(9); p = np.ascontiguousarray([1 if b else 0 for b in pbc], dtype=np.int32)
        g = np.ascontiguousarray(grid, dtype=np.int32); c = np.ascontiguousarray(coord, dtype=np.int32)
        out = C.c_int(0)
        self.L.check(self.L.lib.ahip_comm_borders_cell(self.h, nlocal, C.c_void_p(x_ptr), C.c_void_p(mtype_ptr), capacity, _p(h, C.c_double), _p(p, C.c_int),
                                                       float(rc), _p(g, C.c_int), _p(c, C.c_int), C.byref(out), stream or None))
        return out.value

    def allreduce(self, ptr: int, count: int, kind: int, stream: int = 0) -> None:
        self.L.check(self.L.lib.ahip_comm_allreduce(self.h, ptr, count, kind, stream or None))

    def selftest(self, n: int = 1024, stream: int = 0) -> None:
        self.L.check(self.L.lib.ahip_comm_selftest(self.h, n, stream or None))
