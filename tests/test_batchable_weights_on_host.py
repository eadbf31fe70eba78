"""CPU-only: the weights of a batchable verification (include/aeonflux_gpu.h "Batchable presentation proofs") - the device draw under
AFX_DRAW_BATCH_WEIGHTS squeezed to 16 bytes per commitment, over several SHAKE256 blocks (aeonflux_amd/csrc/keccak.cuh
shake256_draw_words, what k_batch_weights runs) - compiled for the host (tests/hostsim/weights_host.cpp) and compared with hashlib's
SHAKE256 and with the restatement the GPU tests use (tests/batchable_ref.py weights)."""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess

import pytest

from tests.batchable_ref import DRAW_BATCH_WEIGHTS, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = b"aeonflux-amd/device-rng/v1"
M64 = 2 ** 64 - 1
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("weights") / "libweights_host.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out,
           os.path.join(ROOT, "tests", "hostsim", "weights_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    h = C.CDLL(out)
    h.weights_host_draw.restype = None
    h.weights_host_draw.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    return h


def got(lib, seed, stream, index, m, label=DRAW_BATCH_WEIGHTS):
    buf = C.create_string_buffer(16 * m + 16)
    lib.weights_host_draw(buf, seed, stream, index, label, m)
    assert buf.raw[16 * m:] == bytes(16)   # nothing written behind the last weight
    return buf.raw[:16 * m]


def want(seed, stream, index, m, label=DRAW_BATCH_WEIGHTS):
    msg = PREFIX + seed + struct.pack("<QQB", stream, index, label)
    assert len(msg) == 75
    return hashlib.shake_256(msg).digest(16 * m)


def test_the_label_lies_outside_what_afx_rng_expand_serves():
    assert DRAW_BATCH_WEIGHTS > 5 + 31 + 1   # AFX_DRAW_ENC_SEED(31) is the last label served; 37 is pinned as refused


def test_every_length_up_to_several_blocks(lib):
    # a block hands out 136 bytes = 8.5 weights: lengths around every block boundary, odd and even
    for m in list(range(1, 40)) + [51, 52, 68, 69, 166, 400]:
        assert got(lib, SEED, 3, 5, m) == want(SEED, 3, 5, m), m


def test_prefix_property_and_the_integer_layout(lib):
    long = got(lib, SEED, 1, 2, 60)
    for m in (1, 8, 9, 17, 26):
        assert got(lib, SEED, 1, 2, m) == long[:16 * m]
    assert weights(SEED, 1, 2, 26) == [int.from_bytes(long[16 * w:16 * w + 16], "little") for w in range(26)]


def test_edge_counters_and_random_inputs(lib):
    for stream in (0, M64):
        for index in (0, 2 ** 32 - 1, 2 ** 32, M64):
            assert got(lib, SEED, stream, index, 26) == want(SEED, stream, index, 26)
    r = random.Random(20261016)
    for _ in range(2000):
        seed, stream, index, m = r.randbytes(32), r.getrandbits(64), r.getrandbits(64), r.randrange(1, 70)
        assert got(lib, seed, stream, index, m) == want(seed, stream, index, m), (seed.hex(), stream, index, m)


def test_draws_differ_by_every_input(lib):
    base = got(lib, SEED, 1, 1, 26)
    assert got(lib, SEED[:31] + b"\x20", 1, 1, 26) != base
    assert got(lib, SEED, 2, 1, 26) != base
    assert got(lib, SEED, 1, 2, 26) != base
    assert got(lib, SEED, 1, 1, 26, label=4)[:32] != base[:32]
