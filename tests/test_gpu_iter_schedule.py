"""The single-step exact loop's replay (Registration::run_chunked_exact,
reached by the solvers without a triple): a break late in a chunk that is
longer than the iterate ring, so that iteration t's buffer was rewritten by
iteration t + kRing before the host saw the break, and the iterations up to
the break are replayed from the chunk's start buffer
(sched::Ring::replay_needed, opticalflow2d_amd/csrc/iter_schedule.h).

Thirion's Demons, convergence on, default Logger, against the live oracle as
test_gpu_logger_errors.py compares: iteration count, motion and the last
loop's errors bit for bit.
"""
import numpy as np

import pytest

from opticalflow2d_amd import ImageRegistration
from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

K_RING = 15  # OF2D_SN_RING (of2d_host.h)
CHUNK = 40
NITER = 200
DIMS = (64, 48)
PARAMS = [1.0, 0.25, 2.0, 2.0, 5, 0]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_demons_break_past_the_ring_is_replayed(gpu, oracle):
    ref, mov = S.texture_pair(DIMS[0], seed=4, ny=DIMS[1])
    o = oracle.Registration(DIMS, [NITER], 0, 3, PARAMS, 1, 0)
    o.register(ref, mov)
    want = dict(motion=o.motion(), iters=o.iterations(), errs=o.last_errors())
    o.close()
    # the oracle's break, chunk-local: iteration k = t of the chunk [k0, k0 + C)
    k = want["iters"][0] - 1
    assert k + 1 < NITER, "the oracle takes no break: the pair no longer reaches the replay"
    t, k0 = k % CHUNK, k - k % CHUNK
    C = min(CHUNK, NITER - k0)
    assert t + K_RING <= C - 1, (
        f"break at chunk-local {t} of {C}: iteration {t}'s buffer is still intact, no replay")
    with ImageRegistration(DIMS, [NITER], 0, 3, PARAMS, 1, chunk=CHUNK) as r:
        r.register(ref, mov)
        got = dict(motion=r.motion(), iters=r.iterations(), errs=r.last_errors())
    assert got["iters"] == want["iters"]
    assert np.array_equal(got["motion"], want["motion"])
    assert len(got["errs"]) == len(want["errs"]) > 0
    assert bits(got["errs"]) == bits(want["errs"])
