"""CPU: the trajectory semantics restated in tests/traj_ref.py against hand-computed answers (the
quirks of TStatsQuery.java:148-189 pinned), and the binding's new entry points."""
import math

import pytest

import traj_ref as R


@pytest.mark.parametrize("name,points,want", R.KNOWN, ids=[k[0] for k in R.KNOWN])
def test_tstats_known_answers(name, points, want):
    s, t, avg = R.tstats_one(points)
    assert (s, t) == want[:2]
    assert (math.isnan(avg) and math.isnan(want[2])) or avg == want[2]


def test_leading_zero_run_drops_earlier_points():
    # the first two points never contribute: the result is that of the tail alone
    tail = [(0.0, 0.0, 5), (6.0, 8.0, 7)]
    assert R.tstats_one([(50.0, 50.0, 0), (60.0, 60.0, 0)] + tail)[:2] == R.tstats_one(tail)[:2] == (10.0, 2)


def test_grouping_first_appearance_and_arrival_order():
    g = R.group(["b", "a", "b", "ab", "a", "b"])
    assert g["ids"] == ["b", "a", "ab"]
    assert g["traj_of"] == [0, 1, 0, 2, 1, 0]
    assert g["traj_first"] == [0, 1, 3]
    assert g["traj_off"] == [0, 3, 5, 6]
    assert g["perm"] == [0, 2, 5, 1, 4, 3]


def test_empty_set_null_key_error():
    with pytest.raises(R.NullKeyError):
        R.group(["a", None, "b"])
    assert R.group([])["traj_off"] == [0]


def test_nulls_ignored_under_a_non_empty_set():
    g = R.group(["a", None, "b", "a", None], {"a", "zz"})
    assert g["traj_of"] == [0, R.UNSELECTED, R.UNSELECTED, 0, R.UNSELECTED]
    assert g["ids"] == ["a"] and g["perm"] == [0, 3] and g["traj_off"] == [0, 2]


def test_java_division():
    assert math.isnan(R.java_div(0.0, 0)) and math.isnan(R.java_div(math.nan, 0))
    assert R.java_div(2.0, 0) == math.inf and R.java_div(-2.0, 0) == -math.inf
    assert R.java_div(1.0, R.INT64_MAX) == 1.0 / 2.0 ** 63  # (double)Long.MAX_VALUE rounds to 2^63


def test_binding_has_the_trajectory_entry_points():
    from spatialflink_amd import _abi
    for name in ("geohip_traj_group", "geohip_tstats", "geohip_traj_gather", "geohip_traj_selected"):
        assert name in _abi.HEADER_SYMBOLS
    assert "geohip_debug_traj_group_masked" in _abi._SIGS
    assert "geohip_debug_traj_group_masked" not in _abi.HEADER_SYMBOLS
    assert _abi.lib.geohip_abi_version() == 2


def test_pack_strings_layout():
    import numpy as np
    from spatialflink_amd import _abi
    text, off = _abi.pack_strings(["a", None, "ab", "é"])
    assert bytes(text) == b"aab\xc3\xa9"
    assert off.tolist() == [0, (1 << 63) | 1, 1, 3, 5] and off.dtype == np.uint64
