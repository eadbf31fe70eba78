"""CPU-only: SHA-512 as the device runs it (aeonflux_amd/csrc/sha512.cuh, what k_sha512 runs per lane) compiled for the host
(tests/hostsim/sha512_host.cpp) and compared with hashlib.sha512, and encode_to_group's candidate writer against its byte rule
b[0] = 2 * (ctr % 128), b[1..31] = msg, b[31] = ctr / 128."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sha(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sha512") / "libsha512_host.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out,
           os.path.join(ROOT, "tests", "hostsim", "sha512_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(out)
    lib.sha512_host.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_int]
    lib.candidate_host.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32]
    return lib


def got(lib, msg, shift=0):
    """the digest by the dword path (the message 4-byte aligned) when shift == 0, by the byte path at an odd address otherwise"""
    room = C.create_string_buffer(len(msg) + 8)
    base = C.addressof(room)
    at = base + (-base) % 4 + shift
    C.memmove(at, msg, len(msg))
    out = C.create_string_buffer(64)
    lib.sha512_host(out, at, len(msg), 1 if shift == 0 else 0)
    return out.raw


def test_fips_180_4_vectors(sha):
    two_blocks = b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"
    assert len(two_blocks) == 112
    want = {
        b"": "cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e",
        b"abc": "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
        two_blocks: "8e959b75dae313da8cf4f72814fc143f8f7779c6eb9f7fa17299aeadb6889018501d289e4900f7e4331b99dec4b5433ac7d329eeb6dd26545e96e55b874be909",
    }
    for msg, hexd in want.items():
        assert hashlib.sha512(msg).hexdigest() == hexd
        for shift in (0, 1):
            assert got(sha, msg, shift).hex() == hexd, (msg, shift)


def test_every_length_across_the_padding_edges(sha):
    """0..260 covers 111/112 (the length field no longer fits the first block), 127/128 and 239/240"""
    src = hashlib.shake_256(b"afx-tests/sha512-lengths").digest(260)
    for n in range(261):
        for shift in (0, 1, 2, 3):
            assert got(sha, src[:n], shift) == hashlib.sha512(src[:n]).digest(), (n, shift)


def test_random_messages(sha):
    r = random.Random(20261017)
    for _ in range(10000):
        msg = r.randbytes(r.choice((30, 32, 64, r.randrange(0, 1025))))
        shift = r.randrange(4)
        assert got(sha, msg, shift) == hashlib.sha512(msg).digest(), (msg.hex(), shift)


def test_candidate_writer(sha):
    r = random.Random(5)
    for msg in (bytes(30), b"\xff" * 30, bytes(range(1, 31)), r.randbytes(30)):
        for ctr in (0, 1, 127, 128, 129, 8191):
            out = C.create_string_buffer(32)
            sha.candidate_host(out, msg, ctr)
            assert out.raw == bytes([2 * (ctr % 128)]) + msg + bytes([ctr // 128]), (msg.hex(), ctr)
