"""GPU: the point layer between the formulas and the public calls (csrc/sign.hpp, recover.hpp, pmsm.hpp, the GLV rounding of
wit.hpp) on the device, function by function, against Python integers.  The device build of
tests/probe_point/p2e_probe_point.hip instantiates one kernel per (op, curve) with the library's own flags, so the code only
the device compiles -- the DPP quad_perm exchanges of sign_quad_level and SignArith::xchg -- runs, and the complete additions
meet what a whole call cannot choose: one point under two Z, opposite points under two Z, empty operands that carry a
pattern, tight non-canonical limb forms.  Points are compared as points (x = X / Z^2, y = Y / Z^3), values word for word;
there is no tolerance.  test_point_probe_cpu.py asserts on the CPU that the batches contain the classes they claim."""
import pytest

import point_probe_inputs as PP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return PP.PointProbe(device=True)


def test_table_is_the_one_the_vectors_cover(probe):
    assert set(probe.table) == set(PP.PAIRS), (set(probe.table) ^ set(PP.PAIRS))


@pytest.mark.parametrize("name,field", PP.PAIRS, ids=PP.IDS)
def test_device_matches_big_integers(probe, name, field):
    PP.run_case(probe, name, field)
