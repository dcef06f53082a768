"""rpt_probe which = 8 on the MI355X: the thermal point sources' colour operator T_f on 10^6 inputs per flag value — D from
1e-3 to 1e3 and next to 1, x_G from the whole temperature range through the host's conversion, 0, next to 0 and at the range's ends,
colours zero, in [0, 1] and above — must equal tests/thermal_cases.py's numpy float32 restatement bit for bit (which the CPU suite holds
against the C restatement, and that against the float64 model within the derived bound)."""
import numpy as np
import pytest

import thermal_cases as tc
from relativitypathtracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

N = 1000000


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("flags", tc.FLAGS)
def test_the_device_operator_equals_the_numpy_float32_restatement_bit_for_bit(renderer, flags):
    D, c, xg = tc.probe_inputs(N, np.random.default_rng(60 + flags))
    assert len(D) == N and (xg == 0).sum() > 1000 and (D == 1).sum() > 10 and (c == 0).all(axis=1).sum() > 1000
    got = renderer.probe(8, tc.probe_records(D, c, flags, xg), 3)
    want = tc.T32(D, c, flags, xg)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        k = int(np.nonzero(~same.all(axis=1))[0][0])
        raise AssertionError(f"flags {flags}: {int((~same).sum())} of {same.size} channels differ; first at input {k}: D {D[k]!r} c {c[k].tolist()} "
                             f"x_G {xg[k]!r}: device {got[k].tolist()}, numpy {want[k].tolist()}")
    if flags & 1:           # the inputs exercise both arms: S_f (x_G = 0) and Planck, and both of 1 - e^-z's
        thermal = (xg != 0) & (D != 1)
        assert thermal.sum() > 0.8 * N and ((xg[thermal] / D[thermal]) > 0.5).sum() > 1000 and ((xg[thermal] / D[thermal]) <= 0.5).sum() > 1000
