"""CPU: the host build of the point-layer probe (tests/probe_point/p2e_probe_point.hip compiled by g++ with the limb-bound
tracker on) over the vectors of tests/point_probe_inputs.py.  It runs sign.hpp, recover.hpp, pmsm.hpp and the GLV rounding of
wit.hpp function by function against Python integers, proves that the operands (the tight limb forms among them) lie inside
every function's contract (the tracker aborts otherwise) and asserts that every batch holds the classes it claims;
test_gpu_point_probe.py runs the same batches through the device build."""
import pytest

import point_probe_inputs as PP
import p2e_ref as R


@pytest.fixture(scope="module")
def probe():
    return PP.PointProbe(device=False)


def test_table_is_the_one_the_vectors_cover(probe):
    """the op table the C side describes (probe_ops) and the Python table of cases name the same (op, field) pairs"""
    assert set(probe.table) == set(PP.PAIRS), (set(probe.table) ^ set(PP.PAIRS))
    assert len({op for op, _i, _o, _l in probe.table.values()}) == len(PP.TABLE)
    assert {lanes for _op, _i, _o, lanes in probe.table.values()} == {1, 4}
    assert {f"msm_for_digits_c{c}" for c in range(4, 13)} <= set(PP.TABLE)


def test_bad_arguments_are_refused(probe):
    op, inw, outw, lanes = probe.table["msm_on_curve", 0]
    assert probe.L.probe_run(10**6, 0, None, 64, None, 4, 0) == -1
    assert probe.L.probe_run(op, 1, None, 64, None, 4, 0) == -1
    assert probe.L.probe_run(op, 0, None, 60, None, 4, 0) == -2
    assert probe.L.probe_run(op, 0, None, 64, None, 4, 1) == -3
    assert probe.L.probe_run(op, 0, None, 64, None, 4, 0) == 0
    assert probe.L.probe_aux(1, None, 0) == -1 and probe.L.probe_aux(0, None, 8) == -2


def test_fixed_base_table_and_group_patterns():
    """what the sign vectors lean on: slot 0 of every row is slot 1, row w is 16^w times row 0, and the 16 empty / non-empty
    patterns of the four 64-bit groups are all there, the six with exactly two empty groups among them"""
    for field in PP.CURVE_FIELDS:
        cv = PP.curve(field)
        t = PP.fb_table(field)
        assert t.shape == (66 * 16, 16) and (t[0::16] == t[1::16]).all()
        xs, ys = PP.unpack(t[:, :8]), PP.unpack(t[:, 8:])
        assert (xs[1], ys[1]) == cv.g and all(cv.on_curve(pt) for pt in zip(xs, ys))
        assert (xs[16 * 3 + 5], ys[16 * 3 + 5]) == cv.mul(5 << 12, cv.g)
        masks = [m for m, _k in PP.group_pattern_scalars(field // 2)]
        assert sorted(set(masks)) == list(range(16)) and sum(1 for m in set(masks) if bin(m).count("1") == 2) == 6
        assert all(PP.group_mask(k) == m and k < cv.n for m, k in PP.group_pattern_scalars(field // 2))


def test_rounding_scalars_hit_their_remainders():
    rems = PP.rounding_rems()
    got = PP.rounding_scalars()
    assert len(got) == 16
    for kind, cn, k in got:
        assert PP.GLV_CONSTS[cn] * k % R.N == rems[kind.split("_rem_")[1]] and 0 <= k < R.N


@pytest.mark.parametrize("name,field", PP.PAIRS, ids=PP.IDS)
def test_batches_hold_their_classes(name, field):
    PP.check_counts(name, field)


@pytest.mark.parametrize("name,field", PP.PAIRS, ids=PP.IDS)
def test_host_build_matches_big_integers(probe, name, field):
    PP.run_case(probe, name, field)
