"""CPU-only: the plaintext / keypair / encryption / decryption entry points and afx_sha512 on the engine's host half, built against
the fake HIP runtime under ASan/UBSan like tests/test_hostsim.py, with its own source list: the engine's eight host sources,
tests/hostsim/fake_hip.cpp and the stand-ins for the three new launchers (tests/hostsim/fake_plaintext.cpp).  The four *_dev plans
are assembled with the plan self-check on, in the latency plan and the plan of large passes, in every secret mode; counts on and
across pass boundaries; null arguments and an over-long message are refused.  (The fake runtime keeps no log of its copies, so how
many bytes a host form stages is not checked here.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def hostsim_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_plaintext") / "libafx_hostsim.so")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_plaintext.cpp")]
    cmd = ["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fPIC", "-std=c++17",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-shared", "-pthread", "-o", out] + srcs
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


DRIVER = r"""
import os, sys, ctypes as C
sys.path.insert(0, %(root)r)
import numpy as np
import aeonflux_amd as afx
afx.LIB_PATH = %(lib)r
from aeonflux_amd import batch
from tests.helpers import make_credentials
L = afx.lib()
fake = C.CDLL(afx.LIB_PATH)
launches = lambda: [fake.fake_plaintext_launches(k, 1) for k in range(3)]
d = make_credentials(4, "SSPE", 1, b"hostsim-plaintext")
ctx = afx.Context(d["params"], d["key"], d["ip"])
rb = lambda *s: np.zeros(s, np.uint8)
p = lambda a: a.ctypes.data

def drive(cnt):
    msgs, ms = rb(max(cnt, 1), 30), rb(max(cnt, 1), 64)
    n = max(cnt, 1)
    M1, M2, m3, E1, E2 = (rb(n, 32) for _ in range(5))
    ctr, st = np.zeros(n, np.uint32), rb(n)
    kp = {f: rb(n, 32) for f in ("a", "a0", "a1", "pk")}
    soa = afx.KeypairsSoA(*(p(kp[f]) for f in ("a", "a0", "a1", "pk")))
    launches()
    # the four plans over "device" rows (the fake runtime's device memory is host memory), with and without the optional arrays
    assert L.afx_plaintexts_from_bytes_dev(ctx.h, p(msgs), cnt, p(M1), p(M2), p(m3), p(ctr), p(st)) == 0
    assert L.afx_plaintexts_from_bytes_dev(ctx.h, p(msgs), cnt, p(M1), p(M2), p(m3), None, p(st)) == 0
    assert L.afx_keypairs_derive_dev(ctx.h, p(ms), cnt, p(kp["a"]), p(kp["a0"]), p(kp["a1"]), p(kp["pk"])) == 0
    assert L.afx_encrypt_dev(ctx.h, C.byref(soa), p(M1), p(M2), p(m3), cnt, p(E1), p(E2), p(st)) == 0
    msg = rb(n, 30)
    assert L.afx_decrypt_dev(ctx.h, C.byref(soa), p(E1), p(E2), cnt, p(M1), p(M2), p(m3), p(msg), p(st)) == 0
    assert L.afx_decrypt_dev(ctx.h, C.byref(soa), p(E1), p(E2), cnt, p(M1), p(M2), p(m3), None, p(st)) == 0
    # the host forms take the same plans: derive hashes three times per pass, decrypt once, nothing through the direct launcher
    chunk = 256
    passes = (cnt + chunk - 1) // chunk if ctx_chunked else (1 if cnt else 0)
    got = launches()
    assert got == [(2 + 3 + 2) * passes, 0, 2 * passes], (cnt, got, passes)
    assert L.afx_keypairs_derive(ctx.h, p(ms), cnt, p(kp["a"]), p(kp["a0"]), p(kp["a1"]), p(kp["pk"])) == 0
    assert L.afx_encrypt(ctx.h, C.byref(soa), p(M1), p(M2), p(m3), cnt, p(E1), p(E2), p(st)) == 0
    assert L.afx_decrypt(ctx.h, C.byref(soa), p(E1), p(E2), cnt, p(M1), p(M2), p(m3), p(msg), p(st)) == 0
    assert launches() == [4 * passes, 0, 0], cnt
    # (the stub k_finish marks every item 0x5a: the host form reports that as the reference's panic - after the plan has run)
    rc = L.afx_plaintexts_from_bytes(ctx.h, p(msgs), cnt, p(M1), p(M2), p(m3), p(ctr))
    assert rc == (afx.E_BAD_ARGS if cnt else 0) and (cnt == 0 or b"no representative" in L.afx_last_error()), (cnt, rc, L.afx_last_error())
    assert launches() == [passes, 0, passes], cnt
    for mlen in (0, 1, 30, 111, 112, 1024):
        buf = rb(n, max(mlen, 1))
        out = rb(n, 64)
        assert L.afx_sha512(ctx.h, p(buf), mlen, cnt, p(out)) == 0, (cnt, mlen)
    assert launches() == [0, 6 * passes, 0], cnt

ctx_chunked = False
for small in (4096, 0):          # the latency plan and the plan of large passes
    ctx.set_small_batch_items(small)
    for secret in (0, 1, 2):
        ctx.set_secret_independent_addressing(secret)
        ctx.set_plan_variants(afx.VARIANT_SELFCHECK)
        drive(3)
        ctx.set_plan_variants(0)
        drive(5)
ctx.set_small_batch_items(4096)
ctx.set_secret_independent_addressing(2)
# counts on and across pass boundaries
ctx.set_chunk_items(256)
ctx_chunked = True
ctx.set_plan_variants(afx.VARIANT_SELFCHECK)
for cnt in (0, 1, 256, 3 * 256 + 5):
    drive(cnt)
ctx.set_plan_variants(0)

# null arguments, an over-long message
n = 3
a = [rb(n, 64) for _ in range(12)]
st = rb(n)
soa = afx.KeypairsSoA(p(a[0]), p(a[1]), p(a[2]), p(a[3]))
B = afx.E_BAD_ARGS
assert L.afx_sha512(ctx.h, p(a[0]), 1025, n, p(a[1])) == B
assert L.afx_sha512(ctx.h, None, 30, n, p(a[1])) == B and L.afx_sha512(ctx.h, p(a[0]), 30, n, None) == B and L.afx_sha512(None, p(a[0]), 30, n, p(a[1])) == B
assert L.afx_sha512(ctx.h, None, 0, n, p(a[1])) == 0        # (no bytes to read)
for k in (0, 2, 3, 4, 6):                                     # (5, the counters, may be missing)
    args = [p(a[0]), n, p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(st)]
    args[k] = None
    assert L.afx_plaintexts_from_bytes_dev(ctx.h, *args) == B, k
assert L.afx_plaintexts_from_bytes_dev(None, p(a[0]), n, p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(st)) == B
for k in range(5):
    args = [p(a[0]), n, p(a[1]), p(a[2]), p(a[3]), p(a[4])]
    args[(0, 2, 3, 4, 5)[k]] = None
    assert L.afx_keypairs_derive_dev(ctx.h, *args) == B, k
nokey = afx.KeypairsSoA(p(a[0]), None, p(a[2]), p(a[3]))
nopk = afx.KeypairsSoA(p(a[0]), p(a[1]), p(a[2]), None)      # pk is not read
for fn in (L.afx_encrypt, L.afx_encrypt_dev):
    assert fn(ctx.h, None, p(a[4]), p(a[5]), p(a[6]), n, p(a[7]), p(a[8]), p(st)) == B
    assert fn(ctx.h, C.byref(nokey), p(a[4]), p(a[5]), p(a[6]), n, p(a[7]), p(a[8]), p(st)) == B
    assert fn(ctx.h, C.byref(soa), p(a[4]), None, p(a[6]), n, p(a[7]), p(a[8]), p(st)) == B
    assert fn(ctx.h, C.byref(soa), p(a[4]), p(a[5]), p(a[6]), n, p(a[7]), p(a[8]), None) == B
    assert fn(ctx.h, C.byref(nopk), p(a[4]), p(a[5]), p(a[6]), n, p(a[7]), p(a[8]), p(st)) == 0
for fn in (L.afx_decrypt, L.afx_decrypt_dev):
    assert fn(ctx.h, None, p(a[4]), p(a[5]), n, p(a[6]), p(a[7]), p(a[8]), None, p(st)) == B
    assert fn(ctx.h, C.byref(nokey), p(a[4]), p(a[5]), n, p(a[6]), p(a[7]), p(a[8]), None, p(st)) == B
    assert fn(ctx.h, C.byref(soa), None, p(a[5]), n, p(a[6]), p(a[7]), p(a[8]), None, p(st)) == B
    assert fn(ctx.h, C.byref(soa), p(a[4]), p(a[5]), n, p(a[6]), None, p(a[8]), None, p(st)) == B
    assert fn(ctx.h, C.byref(soa), p(a[4]), p(a[5]), n, p(a[6]), p(a[7]), p(a[8]), None, None) == B
    assert fn(ctx.h, C.byref(nopk), p(a[4]), p(a[5]), n, p(a[6]), p(a[7]), p(a[8]), None, p(st)) == 0
# the python mirror over arrays
kp = batch.keypairs_derive(ctx, rb(4, 64))
assert set(kp) == {"a", "a0", "a1", "pk"} and kp["pk"].shape == (4, 32)
E1, E2, s1 = batch.encrypt(ctx, kp, rb(4, 32), rb(4, 32), rb(4, 32))
M1, M2, m3, msg, s2 = batch.decrypt(ctx, kp, E1, E2)
assert msg.shape == (4, 30) and len(s2) == 4 and batch.decrypt(ctx, kp, E1, E2, messages=False)[3] is None
assert batch.sha512(ctx, rb(4, 17)).shape == (4, 64)
ctx.close()
print("ok")
"""


def test_plaintext_entry_points_assemble_cleanly_under_asan(hostsim_lib):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    # AFX_PLAN_SELFCHECK: every plan is assembled twice against different provisional addresses and must relocate to identical bytes
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT, "lib": hostsim_lib}], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-5000:])
