"""CPU-only: the device draw of afx_device_rng (aeonflux_amd/csrc/keccak.cuh shake256_draw, what k_draw runs) compiled for the host
(tests/hostsim/rng_host.cpp) and compared with hashlib's SHAKE256 over the normative message of include/aeonflux_gpu.h:
"aeonflux-amd/device-rng/v1" || seed || u64le(stream) || u64le(index) || u8(label), truncated to the label's length."""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = b"aeonflux-amd/device-rng/v1"
M64 = 2 ** 64 - 1


def draw_len(label):
    return 64 if label in (0, 1, 3) else 32


def want(seed, stream, index, label):
    msg = PREFIX + seed + struct.pack("<QQB", stream, index, label)
    assert len(msg) == 75
    return hashlib.shake_256(msg).digest(draw_len(label))


@pytest.fixture(scope="module")
def rng(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rng") / "librng_host.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out,
           os.path.join(ROOT, "tests", "hostsim", "rng_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(out)
    lib.rng_host_draw.restype = C.c_uint32
    lib.rng_host_draw.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32]
    return lib


def got(lib, seed, stream, index, label):
    buf = C.create_string_buffer(64)
    n = lib.rng_host_draw(buf, seed, stream, index, label)
    assert n == draw_len(label)
    return buf.raw[:n]


SEED = bytes(range(32))


def test_known_answers(rng):
    assert got(rng, SEED, 0, 0, 0).hex() == (
        "52792efbfab0dd9c4071713f0ab70a0e4c2b7c49e97580aa62fdcd2cd4fda4a3"
        "cd71df4cfe45bfa5e4f13ddffe7114c46a2abe3e2e42416f034426d26cd7707f")
    assert got(rng, SEED, 7, 2 ** 32, 5).hex() == "5f980bec16e32296de32092938728e3f2906b4d66190f3097fd14718c0fe6da7"
    assert want(SEED, 7, 2 ** 32, 5) == got(rng, SEED, 7, 2 ** 32, 5)


def test_every_label_and_edge_counters(rng):
    for label in range(37):
        for stream in (0, M64):
            for index in (0, 2 ** 32 - 1, 2 ** 32, M64):
                assert got(rng, SEED, stream, index, label) == want(SEED, stream, index, label), (label, stream, index)
    ff = b"\xff" * 32
    assert got(rng, ff, M64, M64, 36) == want(ff, M64, M64, 36)
    assert got(rng, bytes(32), 0, 0, 4) == want(bytes(32), 0, 0, 4)


def test_random_inputs(rng):
    r = random.Random(20261016)
    for _ in range(10000):
        seed = r.randbytes(32)
        stream, index, label = r.getrandbits(64), r.getrandbits(64), r.randrange(37)
        assert got(rng, seed, stream, index, label) == want(seed, stream, index, label), (seed.hex(), stream, index, label)


def test_draws_differ_by_every_input(rng):
    base = got(rng, SEED, 1, 1, 2)
    assert got(rng, SEED[:31] + b"\x20", 1, 1, 2) != base
    assert got(rng, SEED, 2, 1, 2) != base
    assert got(rng, SEED, 1, 2, 2) != base
    assert got(rng, SEED, 1, 1, 4) != base
