"""``fixed_iters`` switched on a live batch handle: the error buffer is allocated
by the first ``register`` that runs with convergence on, which may be a later
one than the handle's first, and is not read by one that runs without.  After
every call the handle gives what a fresh handle created with that option
gives: the motion bit for bit, ``iterations()`` and ``last_errors()``, which is
empty with ``fixed_iters``.  Diffusion at 16 x 16 and Elastic at 65 x 9, the
smallest width whose workgroup is two waves (a barrier between the sweep's
steps instead of the one-wave ordering).  The ``fluid`` 0/1 toggle is
test_gpu_batch_fluid.py's."""
import numpy as np
import pytest

from test_gpu_batch import make_pairs

pytestmark = pytest.mark.gpu

B = 2
NITER = [5]
CASES = {
    "diffusion": dict(dims=(16, 16), reg=0, params=[0.1]),
    "elastic": dict(dims=(65, 9), reg=2, params=[0.5, 0.25, 0.9]),
}


def result(b):
    return {"motion": b.motion(), "iters": b.iterations(),
            "errs": [b.last_errors(k) for k in range(B)]}


def same(got, want, fixed, what):
    assert np.array_equal(got["motion"], want["motion"]), what
    assert np.array_equal(got["iters"], want["iters"]), what
    for k in range(B):
        assert np.array_equal(got["errs"][k], want["errs"][k]), (what, k)
        if fixed:
            assert got["errs"][k].size == 0, (what, k)
        else:
            assert got["errs"][k].size == got["iters"][k][-1] > 0, (what, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixed_iters_toggle_matches_fresh_handles(name):
    from opticalflow2d_amd import BatchRegistration
    case = CASES[name]
    refs, movs = make_pairs(case["dims"], B)

    def handle(fixed):
        return BatchRegistration(B, case["dims"], NITER, 0, case["params"], reg=case["reg"],
                                 device=0, fixed_iters=fixed)

    fresh = {}
    for fixed in (1, 0):
        with handle(fixed) as b:
            b.register(refs, movs)
            fresh[fixed] = result(b)
    assert not np.array_equal(fresh[1]["motion"], 0 * fresh[1]["motion"])  # the pairs moved
    with handle(1) as b:
        b.register(refs, movs)
        same(result(b), fresh[1], True, "created with fixed_iters=1")
        b.set_option("fixed_iters", 0)
        b.register(refs, movs)
        same(result(b), fresh[0], False, "fixed_iters 1 -> 0")
        b.set_option("fixed_iters", 1)
        b.register(refs, movs)
        same(result(b), fresh[1], True, "fixed_iters 0 -> 1")
