"""vcp_point_features_dev on a caller's non-blocking stream, under the scheme of tests/test_stream_gpu.py (its docstring has
the argument and the measured margins): the input buffers hold cloud A and neighbour rows A; on the caller's stream a
filler kernel, then the copy of cloud B and rows B over the inputs and a poison over the outputs; the entry point is called
while the filler still runs, blocks until its work on that stream is done, and must give the restatement's answer for B,
which differs from its answer for A.  A launch sent to the context's own stream reads A or is overwritten by the
poison."""
import numpy as np
import pytest
import torch

import point_features_ref as R
from test_stream_gpu import Rig, dev, host
from vtkcloudpoint_amd import features as FT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.mark.parametrize("D,k", [(3, 16), (2, 33)])
def test_point_features_dev(rig, D, k):
    n = 3000
    A, B = R.generic_rows(n, D, 60), R.generic_rows(n, D, 61)
    nA, nB = R.mixed_nbr(n, k, 62), R.mixed_nbr(n, k, 63)
    nB[100:164] = -1                                       # rows that are valid under A and not under B
    vp = np.array([0.5, -0.25, 2.0][:D])
    wA, wB = R.features(A, nA, vp), R.features(B, nB, vp)
    assert all(not R.same(wA[key], wB[key]) for key in R.KEYS)
    buf, dB, nbuf, dnB = dev(A), dev(B), dev(nA), dev(nB)
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(normal=torch.zeros((n, D), **f64), eval=torch.zeros((n, D), **f64), variation=torch.zeros(n, **f64),
               mean_dist=torch.zeros(n, **f64), count=torch.zeros(n, dtype=torch.int32, device="cuda"),
               valid=torch.zeros(n, dtype=torch.uint8, device="cuda"))
    rig.run(lambda: rig.ctx._chk(FT._L().vcp_point_features_dev(rig.ctx._h, buf.data_ptr(), D, D, n, nbuf.data_ptr(), k,
                                                                vp.ctypes.data, *[out[key].data_ptr() for key in R.KEYS])),
            [(buf, dB), (nbuf, dnB)], [(out[key], 9 if key == "valid" else -7) for key in R.KEYS])
    d = R.differs({key: host(v) for key, v in out.items()}, wB)
    assert d is None, d
