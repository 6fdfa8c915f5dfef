"""ref_cache.memo: the key holds an array's dtype, shape and bytes, the canonical form makes equal
contents one entry, and the shared result cannot be written."""
import numpy as np
import pytest

from ref_cache import array, memo


def counting():
    calls = []

    @memo(x=array(np.float32), scale=float, lock=bool)
    def ref(x, N, scale, lock, frames=None):
        calls.append((x.dtype, x.shape, x.flags.c_contiguous, type(scale), type(lock), frames))
        return np.asarray(x, np.float64).reshape(-1) * scale + N
    return ref, calls


def test_different_contents_of_equal_shape_are_two_results():
    ref, calls = counting()
    a = ref(np.array([1, 2, 3, 4], np.float32), 8, 0.5, True)
    b = ref(np.array([1, 2, 3, 5], np.float32), 8, 0.5, True)
    assert a is not b and len(calls) == 2
    assert np.array_equal(a, [8.5, 9, 9.5, 10]) and np.array_equal(b, [8.5, 9, 9.5, 10.5])


def test_same_contents_are_the_identical_object():
    ref, calls = counting()
    x = np.array([1, 2, 3, 4], np.float32)
    a = ref(x, 8, 0.5, True)
    strided = np.stack([x, x], axis=1)[:, 0]
    assert not strided.flags.c_contiguous
    assert ref(x.copy(), 8, 0.5, True) is a
    assert ref(strided, 8, 0.5, True) is a
    assert ref(x.astype(np.float64), 8, 0.5, True) is a          # float64 where float32 is canonical
    assert ref([1, 2, 3, 4], N=8, scale=np.float32(0.5), lock=1, frames=None) is a   # scalars normalised, keywords
    assert len(calls) == 1
    # the function saw the canonical values
    assert calls[0] == (np.dtype(np.float32), (4,), True, float, bool, None)
    # every other argument is part of the key
    assert ref(x, 8, 0.5, False) is not a and ref(x, 16, 0.5, True) is not a and ref(x, 8, 0.25, True) is not a
    assert ref(x, 8, 0.5, True, 3) is not a
    assert len(calls) == 5


def test_the_result_is_read_only():
    ref, _ = counting()
    a = ref(np.ones(4, np.float32), 8, 0.5, True)
    assert not a.flags.writeable
    with pytest.raises(ValueError):
        a[0] = 0.0


def test_the_shape_is_part_of_the_key():
    ref, calls = counting()
    flat = np.arange(6, dtype=np.float32)
    a = ref(flat, 8, 0.5, True)
    b = ref(flat.reshape(2, 3), 8, 0.5, True)
    c = ref(flat.reshape(3, 2), 8, 0.5, True)
    assert flat.tobytes() == flat.reshape(2, 3).tobytes()
    assert a is not b and b is not c and len(calls) == 3
    assert [s for _, s, *_ in calls] == [(6,), (2, 3), (3, 2)]


def test_the_dtype_is_part_of_the_key():
    """an array argument without a normaliser keeps its dtype: the same bytes and shape as int64
    and as float64 are two entries"""
    @memo()
    def ref(a):
        return a.copy()
    ints = np.array([1, 2], np.int64)
    i, f = ref(ints), ref(ints.view(np.float64))
    assert i is not f and i.dtype == np.int64 and f.dtype == np.float64 and i.tobytes() == f.tobytes()
    assert ref(ints.copy()) is i
