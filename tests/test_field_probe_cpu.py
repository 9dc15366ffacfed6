"""CPU: the host build of the field / curve-formula probe (tests/probe/p2e_probe.hip compiled by g++ with the limb-bound
tracker on) over the vectors of tests/probe_inputs.py, every output word of every element against Python integers.  It runs
the host branches of csrc/fe.hpp, fe29.hpp, ec.hpp, ec29.hpp, quad.hpp and quad29.hpp, proves the vectors lie inside every
function's contract (the tracker aborts otherwise) and that they reach the rare branches they were built for;
test_gpu_field_probe.py runs the same batches through the device build."""
import pytest

import probe_inputs as PI


@pytest.fixture(scope="module")
def probe():
    return PI.Probe(device=False)


def test_table_is_the_one_the_vectors_cover(probe):
    """the op table the C side describes (probe_ops) and the Python table of cases name the same (op, field) pairs"""
    assert set(probe.table) == set(PI.PAIRS), (set(probe.table) ^ set(PI.PAIRS))
    assert len({op for op, _i, _o, _l in probe.table.values()}) == len(PI.TABLE)
    assert {lanes for _op, _i, _o, lanes in probe.table.values()} == {1, 4}


def test_bad_arguments_are_refused(probe):
    op, inw, outw, lanes = probe.table["fe_mul", 0]
    assert probe.L.probe_run(10**6, 0, None, 64, None, 32, 0) == -1
    assert probe.L.probe_run(op, 7, None, 64, None, 32, 0) == -1
    assert probe.L.probe_run(op, 0, None, 60, None, 32, 0) == -2
    assert probe.L.probe_run(op, 0, None, 64, None, 32, 1) == -3
    assert probe.L.probe_run(op, 0, None, 64, None, 32, 0) == 0


def test_derived_constants():
    """what the vectors lean on: the borrowed-limb multiples of p lie in their class, `top` of the P-256 reduction spans an
    interval, the 29-bit multiplication ceilings sit exactly at the tracker's edge"""
    for k in (1, 2, 3, 4):
        c = PI.f29_subc(k)
        assert PI.limb_value(c) == (32 * k + 1) * PI.P and all(k * PI.F29_T <= x < k * PI.F29_T + (1 << 29) for x in c)
    assert PI.f29_subc(1)[:2] == [0x3FFF820F, 0x3FFFFEF6] and PI.f29_subc(4)[8] == 0x80FFFFFB
    tops = PI.solinas_top_range()
    assert tops[0] < 0 < tops[-1] and len(tops) >= 8
    assert len(PI.mul_ceilings()) == 5 and PI.sqr_ceiling() < 1 << 31
    # Barrett over the two P-256 moduli: the estimate's loss stays below one, so no 512-bit input needs the second of
    # HAC 14.42's two corrections (the class "two corrections" is provably empty and no vector is asked for it)
    assert all(PI.barrett_loss_bound(m) < 1 << 63 for m in (PI.P256, PI.N256))


@pytest.mark.parametrize("name,field", PI.PAIRS, ids=PI.IDS)
def test_host_build_matches_big_integers(probe, name, field):
    PI.run_case(probe, name, field)
