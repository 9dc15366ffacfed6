"""GPU: the field and curve-formula layers (csrc/fe.hpp, fe29.hpp, ec.hpp, ec29.hpp, quad.hpp, quad29.hpp) on the device,
function by function, against Python integers.  The device build of tests/probe/p2e_probe.hip instantiates one kernel per
(op, field) with the library's own flags, so the branches only the device compiles -- the inline-asm column accumulators of
mul_wide / mul_lo, sqr_wide8's cross sum and doubling, the eighteen-scalar noinline call, __umul64hi, the DPP exchanges of
the four-lane levels and of quad_store_form -- run on the constructed vectors of tests/probe_inputs.py (the rare branches by
construction, n = 1 mod 64).  Every output word of every element and of every lane is compared; there is no tolerance.
test_field_probe_cpu.py asserts on the CPU that the batches contain the classes they claim."""
import pytest

import probe_inputs as PI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return PI.Probe(device=True)


def test_table_is_the_one_the_vectors_cover(probe):
    assert set(probe.table) == set(PI.PAIRS), (set(probe.table) ^ set(PI.PAIRS))


@pytest.mark.parametrize("name,field", PI.PAIRS, ids=PI.IDS)
def test_device_matches_big_integers(probe, name, field):
    PI.run_case(probe, name, field)
