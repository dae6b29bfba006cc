"""The "curvature_dct" option on the host (include/of2d.h of2d_set_option):
0 and 1 are accepted, anything else is refused with invalid_argument, and
nothing here touches a device (create + set_option only, as in test_capi)."""
import pytest


def test_curvature_dct_option_values(of2d_lib):
    from opticalflow2d_amd import ImageRegistration, InvalidArgument, set_print_sink
    set_print_sink(lambda s: None)
    try:
        r = ImageRegistration((32, 24), [3], 0, 1, [0.5, 0.2])
        try:
            for v in (0, 1, 0):
                r.set_option("curvature_dct", v)
            for v in (2, -1, 0.5):
                with pytest.raises(InvalidArgument, match="curvature_dct"):
                    r.set_option("curvature_dct", v)
            # no estimate has run: no loops to report
            assert r.curvature_paths() == []
        finally:
            r.close()
        # as a constructor keyword, like the other options
        ImageRegistration((32, 24), [3], 0, 1, [0.5, 0.2], curvature_dct=1).close()
        with pytest.raises(InvalidArgument):
            ImageRegistration((32, 24), [3], 0, 1, [0.5, 0.2], curvature_dct=2)
    finally:
        set_print_sink(None)


def test_dct2d_refuses_bad_arguments(of2d_lib):
    """of2d_dct2d validates kind and method before any device work."""
    import numpy as np
    from opticalflow2d_amd import InvalidArgument, dct2d
    a = np.zeros((8, 8))
    with pytest.raises(InvalidArgument):
        dct2d(a, kind=2)
    with pytest.raises(InvalidArgument):
        dct2d(a, kind=10, method=2)
    with pytest.raises(ValueError):
        dct2d(np.zeros(8), kind=10)


def test_documented_transform_lengths():
    """The Python constants mirror include/of2d.h."""
    import os
    import re
    from conftest import ROOT
    from opticalflow2d_amd import registration as R
    src = open(os.path.join(ROOT, "include", "of2d.h")).read()
    assert int(re.search(r"#define OF2D_DCT_NMIN (\d+)", src).group(1)) == R.DCT_NMIN
    assert int(re.search(r"#define OF2D_DCT_NMAX (\d+)", src).group(1)) == R.DCT_NMAX
    assert R.DCT_NMAX >= 4096
