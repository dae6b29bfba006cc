"""The SOR / Fluid / Elastic per-launch entries on the CPU (include/of2d.h):
every documented refusal comes back as OF2D_ERR_INVALID_ARGUMENT with its
reason, before any device work, and the new names are exported.  No kernel is
launched here."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
INVALID = 1  # OF2D_ERR_INVALID_ARGUMENT
NAMES = ("of2d_prim_sor_pack", "of2d_prim_regrid_pack", "of2d_prim_sor_sweep",
         "of2d_prim_fluid_increment", "of2d_prim_fluid_step", "of2d_prim_fluid_decide",
         "of2d_prim_elastic_logger")
P, I, U, FL, D = C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_double

# name -> (all-pointers-as-void* argtypes, a valid argument list builder);
# "a" stands for a readable and writable array large enough for 4 x 4
RAW = {
    "of2d_prim_sor_pack": ([P, P, P, P, I, I, I, U, P, P, P],
                           ["a", "a", "a", "a", 0, 4, 4, 1, "a", "a", "a"]),
    "of2d_prim_regrid_pack": ([P, P, P, I, I, I, U, P, P, P, P],
                              ["a", "a", "a", 1, 4, 4, 1, "a", "a", "a", "a"]),
    "of2d_prim_sor_sweep": ([P, P, P, I, I, FL, FL, FL, I, I, I, I, I, U, P, P, P, P, P, P, P],
                            ["a", "a", "a", 4, 4, 0.25, 0.0, 0.66, 1, 1, 0, -1, 0, 0,
                             "a", "a", "a", "a", "a", "a", "a"]),
    "of2d_prim_fluid_increment": ([P, P, I, I, I, P, P, P], ["a", "a", 4, 4, 0, "a", "a", "a"]),
    "of2d_prim_fluid_step": ([P, P, P, P, P, P, FL, I, I, I, U, P, P, P, P, P],
                             ["a", "a", "a", "a", "a", "a", 0.5, 0, 4, 4, 1,
                              "a", "a", "a", "a", "a"]),
    "of2d_prim_fluid_decide": ([P, P, I, P, D, I, I, P, P, P, P, P],
                               ["a", "a", 2, "a", 16.0, 0, 0, "a", "a", "a", "a", "a"]),
    "of2d_prim_elastic_logger": ([P, P, I, I, P, P, P], ["a", "a", 4, 4, "a", "a", "a"]),
}
# pointer arguments that may be NULL (by position)
OPTIONAL = {"of2d_prim_fluid_step": {2}, "of2d_prim_fluid_decide": {3}}
# (name, position, bad value): sizes, modes and counts out of range
BAD_VALUES = [
    ("of2d_prim_sor_pack", 5, 0), ("of2d_prim_sor_pack", 6, -1), ("of2d_prim_sor_pack", 4, 2),
    ("of2d_prim_regrid_pack", 4, 1), ("of2d_prim_regrid_pack", 5, 0),
    ("of2d_prim_regrid_pack", 3, 2),
    ("of2d_prim_sor_sweep", 3, 0), ("of2d_prim_sor_sweep", 4, -3), ("of2d_prim_sor_sweep", 8, 2),
    ("of2d_prim_sor_sweep", 8, -1), ("of2d_prim_sor_sweep", 9, 0), ("of2d_prim_sor_sweep", 9, -2),
    ("of2d_prim_sor_sweep", 11, 1), ("of2d_prim_sor_sweep", 11, -2),
    ("of2d_prim_fluid_increment", 2, 0), ("of2d_prim_fluid_increment", 3, -4),
    ("of2d_prim_fluid_step", 8, 0), ("of2d_prim_fluid_step", 9, -1),
    ("of2d_prim_fluid_decide", 2, 0), ("of2d_prim_fluid_decide", 4, 0.0),
    ("of2d_prim_fluid_decide", 6, -1),
    ("of2d_prim_elastic_logger", 2, 0), ("of2d_prim_elastic_logger", 3, 0),
]


def refused(lib, status):
    assert status == INVALID
    assert lib.of2d_gateway_last_error() != b""


def raw_call(lib, name, change=None):
    """The entry with every pointer passed as void *; change = (position, value)."""
    types, args = RAW[name]
    buf = np.zeros(4096, np.float64)
    vals = [buf.ctypes.data if a == "a" else a for a in args]
    if change is not None:
        vals[change[0]] = change[1]
    fn = getattr(lib, name)
    saved = fn.argtypes
    fn.argtypes = types
    try:
        return fn(*vals)
    finally:
        fn.argtypes = saved


def test_names_are_exported(of2d_lib):
    from opticalflow2d_amd import _lib, prim
    for name in NAMES:
        assert hasattr(of2d_lib, name) and name in _lib.SIGNATURES, name
    for name in ("sor_pack", "regrid_pack", "sor_sweep", "fluid_increment", "fluid_step",
                 "fluid_decide", "elastic_logger"):
        assert callable(getattr(prim, name)), name
    assert prim.increment_nblocks(193, 224) == 28 and prim.increment_nblocks(193, 225) == 32


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers_are_refused(of2d_lib, name):
    types, _ = RAW[name]
    for k, t in enumerate(types):
        # (the cases are the force-only pack, which needs v0, and method 1 of
        # the sweep, which needs u, R, scal and part)
        if t is P and k not in OPTIONAL.get(name, ()):
            refused(of2d_lib, raw_call(of2d_lib, name, (k, None)))


@pytest.mark.parametrize("name,pos,value", BAD_VALUES)
def test_bad_values_are_refused(of2d_lib, name, pos, value):
    refused(of2d_lib, raw_call(of2d_lib, name, (pos, value)))


def test_python_wrappers_refuse(of2d_lib):
    from opticalflow2d_amd import prim
    m, img = np.zeros((4, 4, 2), F), np.zeros((4, 4), F)
    with pytest.raises(ValueError):
        prim.sor_sweep(m, m, 0.25, 0.0, 0.66, nsweeps=0)
    with pytest.raises(ValueError):
        prim.sor_sweep(m, m, 0.25, 0.0, 0.66, method=2, u=m)
    with pytest.raises(ValueError):
        prim.sor_sweep(m, m, 0.25, 0.0, 0.66, nsweeps=2, skip_at=2)
    with pytest.raises(ValueError):
        prim.sor_sweep(m, np.zeros((4, 5, 2), F), 0.25, 0.0, 0.66)
    with pytest.raises(ValueError):
        prim.sor_pack(m, m, np.zeros((4, 5), F))
    with pytest.raises(ValueError):
        prim.regrid_pack(img, img, m, 1, m, img, m, np.zeros((3, 4), np.uint32))
    with pytest.raises(ValueError):
        prim.regrid_pack(img[:1], img[:1], m[:1], 1, m[:1], img[:1], m[:1],
                         np.zeros((1, 4), np.uint32))
    with pytest.raises(ValueError):
        prim.fluid_decide(np.zeros((2, 2)), np.zeros(3, F), 16.0, 0, 0, (0, 0, 0, 0))
    with pytest.raises(ValueError):
        prim.fluid_decide(np.zeros((2, 2)), np.zeros(2, F), 16.0, 0, 0, (0, 0, 0))
