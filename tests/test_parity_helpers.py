"""CPU checks of tests/parity.py, the comparisons every parity test goes through."""
import numpy as np
import pytest
from parity import assert_same_counters, assert_same_film, compared_counters


def _counters(pkg, **kw):
    c = pkg._abi.PtCounters().as_dict()
    c.update(kw)
    return c


def test_every_counter_but_the_schedule_is_compared(pkg, monkeypatch):
    fields = [name for name, _ in pkg._abi.PtCounters._fields_]
    monkeypatch.setenv("PT_TEST_TRACE_EXACT", "1")
    assert list(compared_counters()) == [f for f in fields if f != "wavefront_stages"]
    monkeypatch.setenv("PT_TEST_TRACE_EXACT", "0")
    assert list(compared_counters()) == [f for f in fields if f not in ("wavefront_stages", "bvh_nodes_visited")]


def test_a_sphere_test_count_apart_fails(pkg):
    with pytest.raises(AssertionError, match="sphere_tests: 7 != 8"):
        assert_same_counters(_counters(pkg, sphere_tests=7), _counters(pkg, sphere_tests=8))
    assert_same_counters(_counters(pkg, sphere_tests=7), _counters(pkg, sphere_tests=8), skip={"sphere_tests": "(this check)"})
    assert_same_counters(_counters(pkg, wavefront_stages=3), _counters(pkg))
    with pytest.raises(AssertionError):
        assert_same_counters(_counters(pkg), _counters(pkg), skip={"no_such_counter": "(a typo)"})


def test_the_histogram_is_compared_as_a_list(pkg):
    hist = [0] * 16; hist[3] = 5
    assert_same_counters(_counters(pkg, path_length_hist=np.array(hist)), _counters(pkg, path_length_hist=hist))
    hist2 = list(hist); hist2[15] = 1
    with pytest.raises(AssertionError, match="path_length_hist"):
        assert_same_counters(_counters(pkg, path_length_hist=hist2), _counters(pkg, path_length_hist=hist))


def test_film_weights_exact_or_relative():
    ref = np.ones((2, 3, 4), np.float32)
    near = ref.copy(); near[0, 0, 3] = np.nextafter(np.float32(1), np.float32(2))
    with pytest.raises(AssertionError, match="weights"):
        assert_same_film(near, ref)
    assert_same_film(near, ref, weights=1e-6)
    far = ref.copy(); far[1, 2, 0] = 1.01
    with pytest.raises(AssertionError):
        assert_same_film(far, ref)
    with pytest.raises(AssertionError):
        assert_same_film(ref, ref * 2, resolved=(lambda f: f, lambda f: f, 1e-3), rtol=10.0)
