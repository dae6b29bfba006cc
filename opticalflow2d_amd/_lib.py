"""ctypes binding of libof2d.so (include/of2d.h and, for the test entries,
csrc/of2d_prims.h).

The shared library is built in-tree (``opticalflow2d_amd/libof2d.so``) by
``opticalflow2d_amd/csrc/Makefile``.  There is no CPU fallback: if the library
is missing or fails to load, :func:`lib` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
# OF2D_LIB_PATH: another build of the same library (tools/ A/B runs only)
LIB_PATH = os.environ.get("OF2D_LIB_PATH") or os.path.join(PKG_DIR, "libof2d.so")

OF2D_OK = 0
OF2D_ERR_INVALID_ARGUMENT = 1
OF2D_ERR_RUNTIME = 2
OF2D_ERR_DEVICE = 3
OF2D_ERR_STATE = 4

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")


class _f32p_opt(_f32p):
    """A float32 array, or None for an optional (NULL) argument."""

    @classmethod
    def from_param(cls, obj):
        return None if obj is None else _f32p.from_param(obj)

PRINT_FN = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)

OF2D_F32 = 0
OF2D_F64 = 1


class DArray(C.Structure):
    """``of2d_darray``: a strided device array (include/of2d.h)."""
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("stride", C.c_longlong * 4)]


_darr = C.POINTER(DArray)

# name -> (restype, argtypes); the list IS the exported surface of include/of2d.h
PRODUCT_SIGNATURES = {
    "of2d_set_print_hook": (None, [PRINT_FN, C.c_void_p]),
    "of2d_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, _i32p, C.c_int, C.c_int,
                              _f32p, C.c_uint, C.c_int, C.c_int]),
    "of2d_set_images": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "of2d_estimate": (C.c_int, [C.c_void_p]),
    "of2d_get_motion": (C.c_int, [C.c_void_p, _f64p]),
    "of2d_warp": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "of2d_destroy": (C.c_int, [C.c_void_p]),
    "of2d_last_error": (C.c_char_p, [C.c_void_p]),
    "of2d_iterations_executed": (C.c_int, [C.c_void_p, _i32p, C.c_int]),
    "of2d_last_errors": (C.c_int, [C.c_void_p, _f32p, C.c_int]),
    "of2d_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "of2d_curvature_paths": (C.c_int, [C.c_void_p, _i32p, C.c_int]),
    "of2d_demons_paths": (C.c_int, [C.c_void_p, _i32p, C.c_int]),
    "of2d_gateway": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "of2d_gateway_output_numel": (C.c_size_t, [C.c_int, C.c_int]),
    "of2d_gateway_output_dims": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_int)]),
    "of2d_gateway_last_error": (C.c_char_p, []),
    "of2d_slab_bounds": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "of2d_rccl_unique_id_size": (C.c_int, []),
    "of2d_rccl_get_unique_id": (C.c_int, [C.c_void_p, C.c_int]),
    "of2d_slab_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float, C.c_int,
                                   C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "of2d_slab_set_images": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "of2d_slab_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "of2d_slab_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "of2d_slab_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "of2d_slab_get_motion": (C.c_int, [C.c_void_p, _f64p]),
    "of2d_slab_time_kernel": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "of2d_slab_last_run_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "of2d_slab_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "of2d_slab_last_run_kernel_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double),
                                                C.POINTER(C.c_int)]),
    "of2d_slab_last_run_halo_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double),
                                              C.POINTER(C.c_int)]),
    "of2d_slab_last_errors": (C.c_int, [C.c_void_p, _f32p, C.c_int]),
    "of2d_slab_destroy": (C.c_int, [C.c_void_p]),
    "of2d_slab_last_error": (C.c_char_p, [C.c_void_p]),
    "of2d_slab_group_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "of2d_slab_group_destroy": (C.c_int, [C.c_void_p]),
    "of2d_slab_create_local": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float,
                                         C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "of2d_field_jacobian": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_void_p, _f64p]),
    "of2d_jacobian": (C.c_int, [C.c_void_p, C.c_void_p, _f64p]),
    "of2d_field_invert": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, C.c_double, _f32p, _f64p,
                                    C.c_void_p]),
    "of2d_invert_motion": (C.c_int, [C.c_void_p, C.c_int, C.c_double, _f64p, _f64p]),
    "of2d_image_similarity": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, _f64p]),
    "of2d_quality": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p]),
    "of2d_batch_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, _i32p,
                                    C.c_int, C.c_int, _f32p, C.c_uint, C.c_int]),
    "of2d_batch_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "of2d_batch_set_images": (C.c_int, [C.c_void_p, _f64p, C.c_int, _f64p]),
    "of2d_batch_estimate": (C.c_int, [C.c_void_p]),
    "of2d_batch_get_motion": (C.c_int, [C.c_void_p, _f64p]),
    "of2d_batch_warp": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "of2d_batch_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "of2d_batch_iterations": (C.c_int, [C.c_void_p, _i32p, C.c_int]),
    "of2d_batch_last_errors": (C.c_int, [C.c_void_p, C.c_int, _f32p, C.c_int]),
    "of2d_batch_fluid_log": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _f32p, C.c_int]),
    "of2d_batch_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "of2d_batch_destroy": (C.c_int, [C.c_void_p]),
    "of2d_batch_last_error": (C.c_char_p, [C.c_void_p]),
    "of2d_set_images_device": (C.c_int, [C.c_void_p, _darr, _darr, C.c_void_p]),
    "of2d_get_motion_device": (C.c_int, [C.c_void_p, _darr, C.c_void_p]),
    "of2d_warp_device": (C.c_int, [C.c_void_p, _darr, _darr, C.c_void_p]),
    "of2d_batch_set_images_device": (C.c_int, [C.c_void_p, _darr, C.c_int, _darr, C.c_void_p]),
    "of2d_batch_get_motion_device": (C.c_int, [C.c_void_p, _darr, C.c_void_p]),
    "of2d_batch_warp_device": (C.c_int, [C.c_void_p, _darr, _darr, C.c_void_p]),
    "of2d_batch_jacobian": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "of2d_batch_invert_motion": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                           C.c_void_p]),
    "of2d_batch_quality": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "of2d_batch_jacobian_device": (C.c_int, [C.c_void_p, _darr, C.c_void_p, C.c_void_p]),
    "of2d_batch_invert_motion_device": (C.c_int, [C.c_void_p, C.c_int, C.c_double, _darr,
                                                  C.c_void_p, C.c_void_p]),
    "of2d_batch_quality_device": (C.c_int, [C.c_void_p, _darr, C.c_int, _darr, C.c_void_p,
                                            C.c_void_p]),
    "of2d_set_motion": (C.c_int, [C.c_void_p, C.c_void_p]),
    "of2d_set_motion_device": (C.c_int, [C.c_void_p, _darr, C.c_void_p]),
    "of2d_reset_motion": (C.c_int, [C.c_void_p]),
    "of2d_batch_set_motion": (C.c_int, [C.c_void_p, C.c_void_p]),
    "of2d_batch_set_motion_device": (C.c_int, [C.c_void_p, _darr, C.c_void_p]),
    "of2d_batch_reset_motion": (C.c_int, [C.c_void_p]),
    "of2d_version": (C.c_char_p, []),
    "of2d_device_count": (C.c_int, [C.POINTER(C.c_int)]),
}

# the test and diagnostic entries of the same library (csrc/of2d_prims.h)
PRIM_SIGNATURES = {
    "of2d_motion_norms": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p]),
    "of2d_motion_norms_chain": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _i32p]),
    "of2d_dct2d": (C.c_int, [_f64p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p]),
    "of2d_dct_time_passes": (C.c_int, [C.c_int, C.c_int, C.c_int, _f64p]),
    "of2d_prim_warp": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, _f32p]),
    "of2d_prim_accumulate": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, _f32p]),
    "of2d_prim_regrid": (C.c_int, [_f32p, _f32p, _f32p, C.c_int, C.c_int, _f32p, _f32p, _f32p]),
    "of2d_prim_compose_zero": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "of2d_prim_add_motion": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, _f32p]),
    "of2d_prim_resample": (C.c_int, [C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int]),
    "of2d_prim_gradients": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p,
                                      _f32p]),
    "of2d_prim_demons_force": (C.c_int, [_f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_float,
                                         C.c_float, _f32p, C.POINTER(C.c_uint)]),
    "of2d_prim_smooth_compose": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_int, _f32p, C.POINTER(C.c_double), C.c_int,
                                           C.POINTER(C.c_int)]),
    "of2d_prim_smooth_norm": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_float,
                                        _f32p, C.POINTER(C.c_double), C.c_int,
                                        C.POINTER(C.c_int)]),
    "of2d_prim_demons_update": (C.c_int, [_f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_float,
                                          C.c_float, C.c_int, C.c_float, C.c_int, _f32p,
                                          C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int)]),
    "of2d_prim_motion_exp": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_float, C.c_float,
                                       C.POINTER(C.c_int), C.POINTER(C.c_uint)]),
    "of2d_prim_d2f": (C.c_int, [_f64p, C.c_int, C.c_int, _f32p]),
    "of2d_prim_f2d": (C.c_int, [_f32p, C.c_int, C.c_int, _f64p]),
    "of2d_prim_motion_to_planar": (C.c_int, [_f32p, C.c_int, C.c_int, _f64p]),
    "of2d_prim_curv_rhs": (C.c_int, [_f32p, _f32p, _f32p, C.c_float, C.c_int, C.c_int, _f64p,
                                     _f64p]),
    "of2d_prim_curv_eigen": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _f64p]),
    "of2d_prim_curv_dct2d": (C.c_int, [_f64p, _f64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_float, C.c_float, _i32p]),
    "of2d_prim_curv_construct": (C.c_int, [_f64p, _f64p, _f32p, C.c_float, C.c_int, C.c_int,
                                           _f32p, _f64p]),
    "of2d_prim_sor_pack": (C.c_int, [_f32p, _f32p, _f32p, _f32p_opt, C.c_int, C.c_int, C.c_int,
                                     C.c_uint, _f32p, _f32p, _u32p]),
    "of2d_prim_regrid_pack": (C.c_int, [_f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_uint,
                                        _f32p, _f32p, _f32p, _u32p]),
    "of2d_prim_sor_sweep": (C.c_int, [_f32p, _f32p, _f32p_opt, C.c_int, C.c_int, C.c_float,
                                      C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_uint, _f32p, _f32p_opt, _f32p_opt, _f32p_opt,
                                      C.POINTER(C.c_int), _u64p, C.POINTER(C.c_uint)]),
    "of2d_prim_fluid_increment": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, C.c_int, _f32p,
                                            _f32p, _f32p]),
    "of2d_prim_fluid_step": (C.c_int, [_f32p, _f32p, _f32p_opt, _f32p, _f32p, _f32p, C.c_float,
                                       C.c_int, C.c_int, C.c_int, C.c_uint, _f32p, _f64p,
                                       C.POINTER(C.c_float), _f32p, _u32p]),
    "of2d_prim_fluid_decide": (C.c_int, [_f64p, _f32p, C.c_int, _f32p_opt, C.c_double, C.c_int,
                                         C.c_int, _f32p, _u32p, _f64p, _f32p, _u32p]),
    "of2d_prim_elastic_logger": (C.c_int, [_f32p, _f32p, C.c_int, C.c_int, _f32p, _f32p, _f64p]),
    "of2d_analysis_time_kernels": (C.c_int, [C.c_int, C.c_int, C.c_int, _f64p]),
    "of2d_prim_pack_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_int)]),
    "of2d_prim_pack_image": (C.c_int, [_darr, C.c_int, C.c_int, C.c_int, _f32p, _f32p_opt]),
    "of2d_prim_unpack_image": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, _darr]),
    "of2d_prim_unpack_motion": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, _darr]),
    "of2d_prim_pack_motion": (C.c_int, [_darr, C.c_int, C.c_int, C.c_int, _f32p, _f32p_opt]),
    "of2d_prim_planar_to_motion": (C.c_int, [_f64p, C.c_int, C.c_int, C.c_int, _f32p,
                                             _f32p_opt]),
    "of2d_prim_batch_jacobian": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, _f32p_opt, _f64p]),
    "of2d_prim_batch_invert": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                         _f32p, _f64p, _f32p_opt]),
    "of2d_prim_batch_similarity": (C.c_int, [_f32p, C.c_int, _f32p, C.c_int, C.c_int, C.c_int,
                                             _f64p]),
}

SIGNATURES = {**PRODUCT_SIGNATURES, **PRIM_SIGNATURES}  # everything lib() binds

_lib = None


def build(jobs: int = 8) -> str:
    """Compile libof2d.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, f"-j{jobs}"])
    return LIB_PATH


def lib():
    """Load libof2d.so (raises if it is missing: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libof2d.so not found at {LIB_PATH}: build it with "
            "`make -C opticalflow2d_amd/csrc` (or __graft_entry__.build())")
    # One HIP runtime per process: when torch is importable, let it load its
    # libamdhip64.so.7 first so that ours resolves to the same soname.
    try:  # pragma: no cover - environment dependent
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class Of2dError(RuntimeError):
    """Raised for a non-zero status; .status holds the OF2D_ERR_* code."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


class InvalidArgument(Of2dError, ValueError):
    pass


def check(status: int, message: str) -> None:
    if status == OF2D_OK:
        return
    if status == OF2D_ERR_INVALID_ARGUMENT:
        raise InvalidArgument(status, message)
    raise Of2dError(status, message)
