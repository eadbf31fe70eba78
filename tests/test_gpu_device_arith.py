"""GPU: the arithmetic headers as the MI355X runs them - hipcc -O3 for gfx950, AFX_PIN live - fed chosen limbs.
tests/gpu_arith/arith_device.hip runs the case list of tests/arith_cases.py one case per lane; every result must equal the plain
reference (Python integers, pyref, the oracle) bit for bit AND the g++ host build of the same case bodies word for word - limbs
included: integer arithmetic without overflow is deterministic, so a difference means one of the two builds does not compute what the
host build's bounds checker vetted.  The list is repeated past one block and ends in a partial wave; every repetition must give the
answers of the first."""
import ctypes as C
import time

import pytest

from tests import arith_cases

pytestmark = pytest.mark.gpu
_HIP_ERROR = []      # the first HIP error any launch of this module returned: after one, nothing more is launched


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """both builds of the case bodies, compiled once: (device library, host library)"""
    d = tmp_path_factory.mktemp("arith_device")
    dev, took = arith_cases.build_device_lib(d)
    print("\narith_device.hip compiled in %.1f s" % took)
    return dev, arith_cases.build_host_lib(d)


def lanes(cases, block):
    """the list repeated (in order) to more than one block and to a count that is no multiple of 64"""
    n = max(len(cases) + 37, block + 37)
    while n % 64 == 0 or n <= block:
        n += 1
    return [cases[i % len(cases)] for i in range(n)]


def test_the_two_builds_run_the_same_case_bodies(builds):
    dev, host = builds
    a, b = (C.c_uint32 * 16)(), (C.c_uint32 * 16)()
    dev.arith_dev_words(a)
    host.arith_host_words(b)
    assert list(a) == list(b) == [x for k in arith_cases.KINDS.values() for x in k]
    assert dev.arith_dev_block() == 256


@pytest.mark.parametrize("kind", list(arith_cases.KINDS))
def test_limit_cases_on_the_device_build(builds, kind):
    if _HIP_ERROR:
        pytest.fail("not launched: an earlier launch of this module returned HIP error %d (%s)" % _HIP_ERROR[0])
    dev, host = builds
    n_out = arith_cases.KINDS[kind][1]
    cases = arith_cases.rows(kind)
    rows = lanes(cases, dev.arith_dev_block())
    assert len(rows) % 64 and len(rows) > dev.arith_dev_block() and len(rows) >= len(cases)
    t0 = time.time()
    rc, out = arith_cases.run(getattr(dev, "arith_dev_" + kind), rows, n_out)
    print("\n%s: %d lanes, %.3f s" % (kind, len(rows), time.time() - t0))
    if rc != 0:
        _HIP_ERROR.append((rc, kind))
        pytest.fail("HIP error %d" % rc)
    # the plain reference, bit for bit, with the limb ranges the host test asserts
    arith_cases.check(kind, out[:len(cases)])
    # the bounds-checked host build, word for word: limbs of fe_mul, fe_mul_raw, fe_sq, fe_sq_raw, fe_carry, fe10_mul_raw, fe10_sq_raw,
    # fe10_carry, and every encoding
    before = host.arith_bounds_violations()
    _, want = arith_cases.run(getattr(host, "arith_host_" + kind), cases, n_out)
    assert host.arith_bounds_violations() == before, host.arith_last_violation()
    for i, (d, h) in enumerate(zip(out, want)):
        assert d == h, (kind, i, [k for k in range(n_out) if d[k] != h[k]])
    # the same answers in every lane position: the second block, the partial wave
    for i in range(len(cases), len(rows)):
        assert out[i] == out[i % len(cases)], (kind, i)
