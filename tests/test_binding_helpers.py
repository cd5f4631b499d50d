"""The helpers the array-taking methods of the binding share (raytracer-rs_amd/__init__.py): the check of `want`, the making of a new output, the taking of
one from `into`, and the reconciliation of max_distance with `into`.  numpy only: no handle, no library call, no GPU."""
import ctypes as C

import numpy as np
import pytest

N = 8
ALLOWED = ("n", "hits", "sh")


class Outputs(C.Structure):
    _fields_ = [("n", C.c_void_p), ("ok", C.c_void_p), ("sum", C.c_void_p), ("sh", C.c_void_p)]


# the four kinds of output the methods make
KINDS = {"n": ((N,), np.uint32), "ok": ((N,), np.uint8), "sum": ((N, 3), np.float32), "sh": ((N, 9, 3), np.float32)}


def test_want_is_a_non_empty_selection_without_repeats(pkg):
    assert pkg._check_want(["sh", "n"], ALLOWED) == ("sh", "n")            # any iterable, the caller's order kept
    for bad in ((), ("n", "rgb"), ("n", "sh", "n")):
        with pytest.raises(ValueError) as e:
            pkg._check_want(bad, ALLOWED)
        assert str(e.value) == "want: a non-empty selection of %s without repeats, not %r" % (ALLOWED, bad)
    assert pkg._check_want((), ALLOWED, empty_ok=True) == ()
    with pytest.raises(ValueError) as e:
        pkg._check_want(("rgb",), ALLOWED, empty_ok=True)
    assert str(e.value) == "want: a selection of %s without repeats, not %r" % (ALLOWED, ("rgb",))


@pytest.mark.parametrize("field", sorted(KINDS))
def test_a_new_output_has_its_shape_and_dtype_and_is_zero(pkg, field):
    shape, dtype = KINDS[field]
    a = pkg._new_output(shape, dtype)
    assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.dtype(dtype) and a.flags["C_CONTIGUOUS"] and not a.any()
    o = Outputs()
    b = pkg._output(o, field, shape, dtype, None)
    assert b.shape == shape and b.dtype == np.dtype(dtype) and not b.any()
    assert getattr(o, field) == b.ctypes.data
    assert [getattr(o, f) for f in KINDS if f != field] == [None] * 3


@pytest.mark.parametrize("field", sorted(KINDS))
def test_an_output_is_taken_from_into_as_it_is(pkg, field):
    shape, dtype = KINDS[field]
    into = {field: np.full(shape, 7, dtype)}
    o = Outputs()
    assert pkg._output(o, field, shape, dtype, None, into) is into[field]
    assert getattr(o, field) == into[field].ctypes.data and (into[field] == 7).all()


@pytest.mark.parametrize("field", sorted(KINDS))
def test_an_into_entry_that_does_not_fit_is_refused_by_name(pkg, field):
    shape, dtype = KINDS[field]
    name = "into[%r]" % field
    wrong_dtype = np.float64 if dtype == np.float32 else np.int64
    longer = np.zeros((N + 1,) + shape[1:], dtype)
    strided = np.zeros((2 * N,) + shape[1:], dtype)[::2]
    assert strided.shape == shape and not strided.flags["C_CONTIGUOUS"]
    for bad, error, text in ((longer, ValueError, "shape"), (np.zeros(shape[::-1] + (1,), dtype), ValueError, "shape"), (np.zeros(shape, wrong_dtype), TypeError, "dtype"),
                             (strided, ValueError, "C-contiguous"), (list(range(N)), TypeError, "a numpy array or a torch tensor")):
        o = Outputs()
        with pytest.raises(error) as e:
            pkg._output(o, field, shape, dtype, None, {field: bad})
        assert str(e.value).startswith(name + ":") and text in str(e.value), str(e.value)
        assert getattr(o, field) is None                                   # nothing is bound on a refusal
    with pytest.raises(ValueError) as e:
        pkg._output(Outputs(), field, shape, dtype, None, {"other": np.zeros(shape, dtype)})
    assert str(e.value) == "into: holds no %r" % field


def test_max_distance_is_reconciled_with_into(pkg):
    rec = pkg._reconcile_max_distance
    assert rec(2.5, None) == 2.5
    assert rec(0.1, None) == float(np.float32(0.1))                        # the f32 value the library takes
    assert rec(None, dict(max_distance=2.5)) == 2.5                        # None takes into's
    assert rec(np.float32(0.1), dict(max_distance=0.1)) == float(np.float32(0.1))      # equal as f32
    with pytest.raises(ValueError, match="into: its survey has max_distance 2.5, not 3.0"):
        rec(3.0, dict(max_distance=2.5))
    with pytest.raises(ValueError, match="max_distance: give one"):
        rec(None, None)
    with pytest.raises(ValueError, match="into: holds no max_distance"):
        rec(None, dict(n=np.zeros(N, np.uint32)))
    for bad in (0.0, -1.0, float("inf"), float("nan"), 2e12):
        with pytest.raises(ValueError, match="max_distance: finite, > 0 and <= 1e12"):
            rec(bad, None)
    # with a depth film: its res belongs to the agreement
    film = dict(depth_res=8, max_distance=2.5)
    assert rec(None, film, 8) == 2.5 and rec(2.5, None, 8) == 2.5
    with pytest.raises(ValueError, match="into: its depth film has res 8 and max_distance 2.5, not 4 and 2.5"):
        rec(2.5, film, 4)
    with pytest.raises(ValueError, match="into: its depth film has res 8 and max_distance 2.5, not 8 and 3.0"):
        rec(3.0, film, 8)
    with pytest.raises(ValueError, match=r"into: holds no depth film \(depth_res, max_distance\)"):
        rec(2.5, dict(max_distance=2.5), 8)
    with pytest.raises(ValueError, match="res: 2 .. 16, not 17"):
        rec(2.5, None, 17)
