"""The "demons_separable" option on the host (include/of2d.h of2d_set_option):
0 and 1 are accepted, anything else is refused with invalid_argument, the
method argument of the Demons primitives is validated before any device work,
and nothing here touches a device (create + set_option only, as in test_capi)."""
import numpy as np
import pytest

# reg 3 (Thirion's Demons): sigma_i, sigma_x, sigma_diffusion, sigma_fluid, kw, accumulation
PARAMS = [1.0, 0.25, 2.0, 2.0, 5, 0]


def test_demons_separable_option_values(of2d_lib):
    from opticalflow2d_amd import ImageRegistration, InvalidArgument, set_print_sink
    set_print_sink(lambda s: None)
    try:
        r = ImageRegistration((32, 24), [3], 0, 3, PARAMS)
        try:
            for v in (0, 1, 0):
                r.set_option("demons_separable", v)
            for v in (2, -1, 0.5):
                with pytest.raises(InvalidArgument, match="demons_separable"):
                    r.set_option("demons_separable", v)
            # no estimate has run: no loops to report
            assert r.demons_paths() == []
        finally:
            r.close()
        # as a constructor keyword, like the other options
        ImageRegistration((32, 24), [3], 0, 3, PARAMS, demons_separable=1).close()
        with pytest.raises(InvalidArgument, match="demons_separable"):
            ImageRegistration((32, 24), [3], 0, 3, PARAMS, demons_separable=2)
        # accepted (and ignored) by a solver that is not Demons
        with ImageRegistration((32, 24), [3], 0, 0, [0.1], demons_separable=1) as h:
            assert h.demons_paths() == []
    finally:
        set_print_sink(None)


@pytest.mark.parametrize("method", [2, -1])
def test_primitives_refuse_bad_method(of2d_lib, method):
    """The *_m entries validate the method before any device work."""
    from opticalflow2d_amd import InvalidArgument, prim
    f = np.zeros((8, 16, 2), np.float32)
    img = np.zeros((8, 16), np.float32)
    with pytest.raises(InvalidArgument):
        prim.smooth_compose(f, f, 5, 2.0, 3, method=method)
    with pytest.raises(InvalidArgument):
        prim.smooth_norm(f, f, 5, 2.0, method=method)
    with pytest.raises(InvalidArgument):
        prim.demons_update(img, img, f, 1.0, 0.25, 5, 2.0, 0, method=method)


def test_documented_separable_width():
    """The Python constant mirrors include/of2d.h."""
    import os
    import re
    from conftest import ROOT
    from opticalflow2d_amd import registration as R
    src = open(os.path.join(ROOT, "include", "of2d.h")).read()
    assert int(re.search(r"#define OF2D_SEP_KW_MAX (\d+)", src).group(1)) == R.SEP_KW_MAX
    assert R.SEP_KW_MAX == 15
