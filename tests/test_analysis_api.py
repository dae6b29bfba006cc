"""The deformation-analysis entry points on the CPU (include/of2d.h,
"deformation analysis"): every documented refusal comes back as
OF2D_ERR_INVALID_ARGUMENT with its reason, before any device work, through the
C-ABI and as a ValueError / Of2dError from Python; the wrappers reject wrong
shapes; the new names are exported.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
INVALID = 1  # OF2D_ERR_INVALID_ARGUMENT


@pytest.fixture()
def reg(of2d_lib):
    from opticalflow2d_amd import ImageRegistration, set_print_sink
    set_print_sink(lambda s: None)
    r = ImageRegistration((8, 6), [3], 0, 0, [0.1])
    yield r
    r.close()
    set_print_sink(None)


def refused(lib, status, ctx=None):
    assert status == INVALID
    assert lib.of2d_gateway_last_error() != b""
    if ctx is not None:
        assert lib.of2d_last_error(ctx) != b""


def test_names_are_exported(of2d_lib):
    import opticalflow2d_amd as M
    from opticalflow2d_amd import registration as R
    assert "field" in M.__all__ and "field" in R.__all__
    for name in ("jacobian", "invert", "similarity"):
        assert callable(getattr(M.field, name))
    for name in ("jacobian", "inverse_motion", "quality"):
        assert callable(getattr(M.ImageRegistration, name))
    for name in ("of2d_field_jacobian", "of2d_jacobian", "of2d_field_invert",
                 "of2d_invert_motion", "of2d_image_similarity", "of2d_quality"):
        assert hasattr(of2d_lib, name), name
    assert R.INVERT_CHUNK >= 2


def test_chunk_constant_matches_header():
    import os
    import re
    from conftest import ROOT
    from opticalflow2d_amd.registration import INVERT_CHUNK
    src = open(os.path.join(ROOT, "include", "of2d.h")).read()
    assert int(re.search(r"#define OF2D_INVERT_CHUNK (\d+)", src).group(1)) == INVERT_CHUNK


@pytest.mark.parametrize("dimx,dimy", [(1, 8), (8, 1), (1, 1), (0, 4), (4, -1)])
def test_field_jacobian_refuses_thin_fields(of2d_lib, dimx, dimy):
    u = np.zeros(64, F)
    st = np.zeros(5)
    refused(of2d_lib, of2d_lib.of2d_field_jacobian(u, dimx, dimy, None, st))


def test_field_jacobian_refuses_null(of2d_lib):
    fn = of2d_lib.of2d_field_jacobian
    u, st = np.zeros(64, F), np.zeros(5)
    saved = fn.argtypes
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    try:
        refused(of2d_lib, fn(None, 4, 4, None, st.ctypes.data))
        refused(of2d_lib, fn(u.ctypes.data, 4, 4, None, None))
    finally:
        fn.argtypes = saved


@pytest.mark.parametrize("dimx,dimy,max_iter,tol", [
    (4, 4, 0, 1e-3), (4, 4, -5, 1e-3), (4, 4, 10, 0.0), (4, 4, 10, -1e-3),
    (4, 4, 10, float("nan")), (4, 4, 10, float("inf")), (4, 4, 10, float("-inf")),
    (1, 4, 10, 1e-3), (4, 1, 10, 1e-3)])
def test_field_invert_refusals(of2d_lib, dimx, dimy, max_iter, tol):
    u, v, info = np.zeros(32, F), np.zeros(32, F), np.zeros(4)
    refused(of2d_lib, of2d_lib.of2d_field_invert(u, dimx, dimy, max_iter, tol, v, info, None))


def test_field_invert_refuses_null(of2d_lib):
    fn = of2d_lib.of2d_field_invert
    u, v, info = np.zeros(32, F), np.zeros(32, F), np.zeros(4)
    saved = fn.argtypes
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                   C.c_void_p]
    try:
        for a, b, c in [(None, v, info), (u, None, info), (u, v, None)]:
            p = [x.ctypes.data if x is not None else None for x in (a, b, c)]
            refused(of2d_lib, fn(p[0], 4, 4, 10, 1e-3, p[1], p[2], None))
    finally:
        fn.argtypes = saved


def test_similarity_refusals(of2d_lib):
    fn = of2d_lib.of2d_image_similarity
    a, out = np.zeros(16, F), np.zeros(2)
    refused(of2d_lib, fn(a, a, 0, 4, out))
    refused(of2d_lib, fn(a, a, 4, 0, out))
    saved = fn.argtypes
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    try:
        refused(of2d_lib, fn(None, a.ctypes.data, 4, 4, out.ctypes.data))
        refused(of2d_lib, fn(a.ctypes.data, None, 4, 4, out.ctypes.data))
        refused(of2d_lib, fn(a.ctypes.data, a.ctypes.data, 4, 4, None))
    finally:
        fn.argtypes = saved


def test_context_entries_refuse(of2d_lib, reg):
    L, h = of2d_lib, reg._h
    n = reg.dimx * reg.dimy
    out, info, st, img = np.zeros(2 * n), np.zeros(4), np.zeros(5), np.zeros(n)
    for max_iter, tol in [(0, 1e-3), (10, 0.0), (10, float("nan")), (10, float("inf"))]:
        refused(L, L.of2d_invert_motion(h, max_iter, tol, out, info), h)
    refused(L, L.of2d_invert_motion(None, 10, 1e-3, out, info))
    refused(L, L.of2d_jacobian(None, None, st))
    refused(L, L.of2d_quality(None, img, img, np.zeros(4)))
    for fn, types, args in [
            (L.of2d_jacobian, [C.c_void_p] * 3, (h, None, None)),
            (L.of2d_invert_motion, [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p],
             (h, 10, 1e-3, None, info.ctypes.data)),
            (L.of2d_invert_motion, [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p],
             (h, 10, 1e-3, out.ctypes.data, None)),
            (L.of2d_quality, [C.c_void_p] * 4, (h, None, img.ctypes.data, out.ctypes.data)),
            (L.of2d_quality, [C.c_void_p] * 4, (h, img.ctypes.data, None, out.ctypes.data)),
            (L.of2d_quality, [C.c_void_p] * 4, (h, img.ctypes.data, img.ctypes.data, None))]:
        saved = fn.argtypes
        fn.argtypes = types
        try:
            refused(L, fn(*args), h)
        finally:
            fn.argtypes = saved


def test_context_entries_refuse_thin_grids(of2d_lib):
    from opticalflow2d_amd import ImageRegistration, InvalidArgument, set_print_sink
    set_print_sink(lambda s: None)
    try:
        with ImageRegistration((1, 6), [3], 0, 0, [0.1]) as r:
            out, info, st = np.zeros(12), np.zeros(4), np.zeros(5)
            refused(of2d_lib, of2d_lib.of2d_jacobian(r._h, None, st), r._h)
            refused(of2d_lib, of2d_lib.of2d_invert_motion(r._h, 10, 1e-3, out, info), r._h)
            with pytest.raises(InvalidArgument):
                r.jacobian()
            with pytest.raises(InvalidArgument):
                r.inverse_motion()
    finally:
        set_print_sink(None)


def test_python_refusals(of2d_lib, reg):
    from opticalflow2d_amd import Of2dError, field
    u = np.zeros((6, 8, 2), F)
    for kw in [dict(max_iter=0), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")),
               dict(tol=float("inf"))]:
        with pytest.raises((ValueError, Of2dError)):
            field.invert(u, **kw)
        with pytest.raises((ValueError, Of2dError)):
            reg.inverse_motion(**kw)
    for bad in [np.zeros((6, 8), F), np.zeros((6, 8, 3), F), np.zeros((1, 8, 2), F),
                np.zeros((6, 1, 2), F), np.zeros((2, 6, 8, 2), F)]:
        with pytest.raises(ValueError):
            field.jacobian(bad)
        with pytest.raises(ValueError):
            field.invert(bad)
    img = np.zeros((6, 8), F)
    for a, b in [(img, np.zeros((8, 6), F)), (img, np.zeros((6, 9), F)), (np.zeros(48, F), img),
                 (np.zeros((0, 8), F), np.zeros((0, 8), F)), (u, u)]:
        with pytest.raises(ValueError):
            field.similarity(a, b)
    with pytest.raises(ValueError):
        reg.quality(np.zeros((8, 5)), np.zeros((8, 6)))
    with pytest.raises(ValueError):
        reg.quality(np.zeros((8, 6)), np.zeros((8, 7)))
