"""tests/analysis_gpu.py on the CPU: the rule ``Guarded.collect`` holds every raw call to, and ``frozen``.  The "library call" is a Python function
that writes float64 / int32 values at the addresses it is handed, as the library does; nothing here needs a GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

import analysis_gpu as A

SPEC = {"a": ((2, 3, 4), torch.float64), "n": ((2, 3), torch.int32), "empty": ((2, 0, 4), torch.float64)}
CTYPE = {"a": ctypes.c_double, "n": ctypes.c_int32}


def at(address, name, count, offset=0):
    """``count`` elements of output ``name``'s type at ``address`` + ``offset`` elements, as a writable numpy view."""
    t = CTYPE[name]
    return np.ctypeslib.as_array((t * count).from_address(address + offset * ctypes.sizeof(t)))


def call(null=(), write=(), stray=()):
    """A call that fills the outputs named in ``write`` with 1, 2, 3 ... and writes 5 at each (name, element offset) of ``stray``."""
    out = A.Guarded(SPEC, null, device="cpu")
    whole = {k: out.out[k][0].data_ptr() + A.M * ctypes.sizeof(CTYPE[k]) for k in CTYPE}         # (the payload's address, NULL or not)
    assert all(out.ptr(k) == (None if k in null else whole[k]) for k in CTYPE), "the payload's address, or NULL where asked"
    for k in write:
        n = int(np.prod(SPEC[k][0]))
        at(whole[k], k, n)[:] = np.arange(1, n + 1)
    for k, offset in stray:
        at(whole[k], k, 1, offset)[0] = 5
    return out


def test_a_well_behaved_call_comes_back_as_written_and_null_as_none():
    got = call(write=("a", "n")).collect(0)
    assert np.array_equal(got["a"], np.arange(1.0, 25.0).reshape(2, 3, 4)) and got["a"].dtype == np.float64
    assert np.array_equal(got["n"], np.arange(1, 7).reshape(2, 3)) and got["n"].dtype == np.int32
    assert got["empty"].shape == (2, 0, 4) and list(got) == list(SPEC)
    got = call(null=("n",), write=("a",)).collect(0)
    assert got["n"] is None and got["a"][1, 2, 3] == 24.0


@pytest.mark.parametrize("name,offset", [("a", -1), ("a", 24), ("n", -1), ("n", 6), ("a", -A.M), ("n", 6 + A.M - 1)])
def test_a_write_into_a_margin_raises_and_names_the_output(name, offset):
    with pytest.raises(AssertionError, match=f"sentinel margin of d_{name}"):
        call(write=("a", "n"), stray=[(name, offset)]).collect(0)


def test_a_write_into_an_output_passed_as_null_raises():
    with pytest.raises(AssertionError, match="d_n was not asked for"):
        call(null=("n",), write=("a",), stray=[("n", 3)]).collect(0)


@pytest.mark.parametrize("name,offset", [("a", 0), ("a", 23), ("n", 5)])
def test_a_failed_call_that_wrote_an_element_raises(name, offset):
    with pytest.raises(AssertionError, match=f"d_{name} was not asked for \\(or the call failed\\)"):
        call(stray=[(name, offset)]).collect(1)


def test_a_failed_call_that_wrote_nothing_returns_none_for_every_output():
    assert call().collect(-3) == {"a": None, "n": None, "empty": None}


def test_fills_follow_the_dtype_unless_overridden():
    out = A.Guarded({"f": ((3,), torch.float32), "i": ((3,), torch.int32), "u": ((3,), torch.uint8), "back": ((3,), torch.uint8)}, fills={"back": 201},
                    device="cpu")
    assert [float(out.out[k][0][0]) for k in ("f", "i", "u", "back")] == [777.0, -777.0, 77.0, 201.0]
    assert all(out.out[k][0].numel() == 3 + 2 * A.M for k in out.out) and A.M == 64


def test_frozen_computes_once_and_sets_every_array_read_only():
    made, cache = [], {}

    def make():
        made.append(1)
        return {"d": np.zeros(3), "n": 7}, (np.ones(2), (np.ones(1), np.ones(1))), [np.zeros(4)]

    r = A.frozen(cache, "key", make)
    assert A.frozen(cache, "key", make) is r and len(made) == 1
    for a in (r[0]["d"], r[1][0], r[1][1][0], r[1][1][1], r[2][0]):
        with pytest.raises(ValueError):
            a[0] = 1.0
    assert A.frozen(cache, "other", lambda: np.arange(3)) is not r and len(cache) == 2
