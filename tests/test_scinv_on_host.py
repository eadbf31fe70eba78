"""CPU-only: the scalar inversion of the presentation tags - aeonflux_amd/csrc/tags.cuh sc_invert, tag_sum and tag_inverse_row, the
statements k_sc_invert runs per lane - compiled for the host (tests/hostsim/scinv_host.cpp) and compared with Python integers:

    sc_invert(s)          == pow(s, l - 2, l)            for every canonical s (0 for s == 0)
    tag_inverse_row(a, b) == pow(a + b, l - 2, l)        or l itself - no canonical scalar - where a + b == 0 (mod l)

on every named edge scalar of tests/edge_values.all_scalars(), on 1, 2, l - 1, (l + 1)/2 and 2^252, and on 300 random scalars."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import edge_values as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = EV.L


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scinv") / "libscinv_host.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out,
           os.path.join(ROOT, "tests", "hostsim", "scinv_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    h = C.CDLL(out)
    h.scinv_host_invert.restype = None
    h.scinv_host_invert.argtypes = [C.c_char_p, C.c_char_p]
    h.scinv_host_row.restype = None
    h.scinv_host_row.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    return h


def invert(lib, s):
    out = C.create_string_buffer(32)
    lib.scinv_host_invert(out, s.to_bytes(32, "little"))
    return int.from_bytes(out.raw, "little")


def row(lib, a, b):
    out = C.create_string_buffer(32)
    lib.scinv_host_row(out, a.to_bytes(32, "little"), b.to_bytes(32, "little"))
    return int.from_bytes(out.raw, "little")


def scalars():
    named = dict(EV.all_scalars())
    named.update({"one": 1, "two": 2, "l-1": L - 1, "(l+1)/2": (L + 1) // 2, "2^252": 2 ** 252})
    rnd = random.Random(20251)
    named.update(("random %d" % k, rnd.randrange(L)) for k in range(300))
    return named


def test_sc_invert_is_the_fermat_inverse(lib):
    for name, s in scalars().items():
        assert 0 <= s < L, name
        got = invert(lib, s)
        assert got == pow(s, L - 2, L), name
        if s:
            assert got * s % L == 1, name
    assert invert(lib, 0) == 0
    assert invert(lib, 1) == 1 and invert(lib, L - 1) == L - 1 and invert(lib, 2) == (L + 1) // 2


def test_the_row_of_a_sum(lib):
    rnd = random.Random(20252)
    for name, s in scalars().items():
        a = rnd.randrange(L)
        b = (s - a) % L                                   # a + b == s (mod l), the integer sum on either side of l
        want = pow(s, L - 2, L) if s else L
        assert row(lib, a, b) == want, name
        assert row(lib, b, a) == want, name
        assert row(lib, s, 0) == want and row(lib, 0, s) == want, name


def test_a_zero_sum_takes_the_failure_path(lib):
    # the row is l: not canonical, so the pass's canonicity test of the row fails the item
    for a in (0, 1, 2, L - 1, (L + 1) // 2, 2 ** 252, random.Random(3).randrange(L)):
        assert row(lib, a, (L - a) % L) == L, a
    assert row(lib, L - 1, 1) == L and row(lib, 0, 0) == L


def test_operands_that_are_not_canonical_still_give_the_inverse_of_their_sum(lib):
    # (the item has failed by then - its counter is tested for canonicity - but the lane computes on, like every other lane)
    for a, b in ((L, 1), (2 ** 256 - 1, 2 ** 256 - 1), (2 ** 255, L - 1), (L + 5, L + 7)):
        s = (a + b) % L
        assert row(lib, a, b) == (pow(s, L - 2, L) if s else L), (a, b)
