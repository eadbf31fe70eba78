"""CPU-only: every launch kind of the engine's table (aeonflux_amd/csrc/launch_kinds.hpp) is assembled, relocated under the plan
self-check and dispatched on the engine's host half, built plain (no sanitizer, nothing preloaded) against the fake HIP runtime
with every stand-in launcher there is - tests/hostsim/fake_messages.cpp brings the last four.  The self-check (AFX_PLAN_SELFCHECK=1)
assembles every plan twice against different provisional bases and compares the relocated bytes: a pointer member missing from a
kind's table entry fails the call that launches the kind.  Issue, verify, show, the batchable verification, the blind flow, the
keypair / encryption / plaintext calls, the known-counter plaintexts and the whole-message calls run at 3 items in the latency plan
and at 5 items in the plan of large passes, with secret-independent addressing off and on the prover side; afterwards every name
of the table, "copy" included, must have counted launches."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
# the table's names as its entries spell them (`L_<KIND>, "<name>"`): the 24 kinds up to k_encode_at, and whatever is added behind them
with open(os.path.join(CSRC, "launch_kinds.hpp")) as _f:
    KIND_NAMES = re.findall(r'[({]\s*L_[A-Z0-9_]+, "([^"]+)"', _f.read())
assert KIND_NAMES[:24] == ["k_fill_u32", "k_decode", "k_sccheck", "k_pointop", "k_scalarop", "k_msm_window", "k_hash", "k_from_uniform", "k_reduce_wide", "copy",
                           "k_finish", "k_msm_fixed", "k_msm_naf", "k_msm_tables", "k_compress2x", "k_pointsum", "k_negenc", "k_table_affine", "k_powers", "k_coef",
                           "k_sha512", "k_encode_to_group", "k_mask_rows", "k_encode_at"], KIND_NAMES


@pytest.fixture(scope="module")
def hostsim_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_kinds") / "libafx_hostsim.so")
    srcs = [os.path.join(CSRC, f + ".cpp") for f in ("engine", "plans", "statements", "statements_prove", "statements_setup", "statements_blind",
                                                    "statements_messages", "group", "mixed", "wire")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_plaintext.cpp", "fake_blind.cpp", "fake_batchable.cpp", "fake_draw.cpp",
                                                                "fake_messages.cpp")]
    cmd = ["g++", "-O1", "-fPIC", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-shared", "-pthread", "-o", out] + srcs
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
rb = lambda *s: np.zeros(s, np.uint8)
p = lambda a: a.ctypes.data
N, HIDE, BLIND_KINDS = 4, [0, 3], [4, 2, 3, 1]
d = make_credentials(N, "SSPE", 5, b"launch-kinds-host")
ctx = afx.Context(d["params"], d["key"], d["ip"])
ctx.set_timing(True)
creds = d["creds"]
kinds = creds[0]["kinds"]
k2 = list(kinds)
for i in HIDE:
    k2[i] = 1 if k2[i] == 0 else 4          # a hidden scalar and a hidden encrypted point
nsp = sum(1 for k in k2 if k == 4)
h, hs = batch.blind_layout(BLIND_KINDS)

def no_representative(rc):
    # the stub k_finish marks every item 0x5a: the host forms of the plaintext calls report that as the reference's panic, after
    # the plan has run
    return rc == afx.E_BAD_ARGS and b"no representative" in L.afx_last_error()

def drive(cnt):
    values = np.stack([np.stack([np.frombuffer(c["values"][i][:32], np.uint8) for c in creds[:cnt]]) for i in range(N)])
    iss, st = batch.issue(ctx, kinds, values, rb(cnt, 64), rb(cnt, 64), rb(cnt, 32))
    batch.verify_issuances(ctx, kinds, values, iss)
    kp = {f: rb(cnt, 32) for f in ("a", "a0", "a1", "pk")}
    show_args = (k2, values, iss["t"], iss["U"], iss["V"], kp, rb(cnt, 64), rb(cnt, 32), rb(max(nsp, 1), cnt, 32), values, values)
    pres, shape, st = batch.show(ctx, *show_args)
    batch.verify_presentations(ctx, shape, pres)
    bpres, cm, bshape, st = batch.show_batchable(ctx, *show_args)
    batch.verify_presentations_batchable(ctx, bshape, bpres, cm, bytes(32))
    # the blind flow
    req, st = batch.blind_request(ctx, BLIND_KINDS, values, rb(cnt, 32), rb(h, cnt, 64), rb(cnt, 32))
    batch.verify_blind_requests(ctx, BLIND_KINDS, req)
    biss, st = batch.issue_blind(ctx, BLIND_KINDS, values, req, rb(cnt, 64), rb(cnt, 64), rb(cnt, 64), rb(cnt, 32))
    batch.unblind_issuances(ctx, BLIND_KINDS, values, rb(cnt, 32), req, biss)
    # keypairs, encryption, decryption, plaintexts: the host forms and the *_dev plans (the fake runtime's device memory is host memory)
    kp = batch.keypairs_derive(ctx, rb(cnt, 64))
    E1, E2, st = batch.encrypt(ctx, kp, rb(cnt, 32), rb(cnt, 32), rb(cnt, 32))
    batch.decrypt(ctx, kp, E1, E2)
    msgs, ctr, stt = rb(cnt, 30), np.zeros(cnt, np.uint32), rb(cnt)
    M1, M2, m3 = (rb(cnt, 32) for _ in range(3))
    rc = L.afx_plaintexts_from_bytes(ctx.h, p(msgs), cnt, p(M1), p(M2), p(m3), p(ctr))
    assert rc == 0 or no_representative(rc), (rc, L.afx_last_error())
    assert L.afx_plaintexts_from_bytes_dev(ctx.h, p(msgs), cnt, p(M1), p(M2), p(m3), p(ctr), p(stt)) == 0, L.afx_last_error()
    assert L.afx_plaintexts_from_bytes_at_dev(ctx.h, p(msgs), p(ctr), cnt, p(M1), p(M2), p(m3), p(stt)) == 0, L.afx_last_error()
    rc = L.afx_plaintexts_from_bytes_at(ctx.h, p(msgs), p(ctr), cnt, p(M1), p(M2), p(m3), p(stt))
    assert rc == 0 or no_representative(rc), (rc, L.afx_last_error())
    # whole messages: an empty one, an exact chunk, one that straddles two chunks (the 5-item run adds two of several chunks)
    messages = [b"", bytes(30), bytes(31), bytes(95), bytes(7)][:cnt]
    blob, offsets = batch.pack_messages(messages)
    cf = batch.chunk_table(offsets)
    nch = int(cf[-1])
    room = [rb(nch, 32) for _ in range(3)] + [np.zeros(nch, np.uint32)]
    rc = L.afx_plaintexts_from_messages(ctx.h, p(blob), p(offsets), cnt, *(p(a) for a in room))
    assert rc == 0 or no_representative(rc), (rc, L.afx_last_error())
    E1, E2, ctrs, cf2, st = batch.encrypt_messages(ctx, kp, messages)
    assert cf2.tolist() == cf.tolist() and E1.shape == (nch, 32)
    out, st = batch.decrypt_messages(ctx, kp, E1, E2, cf)
    assert [len(m) for m in out] == [30 * (int(cf[i + 1]) - int(cf[i])) for i in range(cnt)]

for cnt, small in ((3, 4096), (5, 0)):       # the latency plan and the plan of large passes
    ctx.set_small_batch_items(small)
    for secret in (0, 2):
        ctx.set_secret_independent_addressing(secret)
        drive(cnt)
# The pointers of a job into the call's STAGED arrays (a host-pointer call's inputs and outputs) are the same under both provisional
# bases; what checks them is a cached plan's reuse under another staging layout (the self-check compares the relocated plan with a
# fresh one).  So: one call large enough to move the lane's staging buffers, then the 3-item calls again, on their cached plans.
ctx.set_small_batch_items(4096)
hits = ctx.plan_cache_stats()["hits"]
batch.keypairs_derive(ctx, rb(40000, 64))
for secret in (0, 2):
    ctx.set_secret_independent_addressing(secret)
    drive(3)
assert ctx.plan_cache_stats()["hits"] > hits, ctx.plan_cache_stats()
missing =[name for name in %(names)r if ctx.get_timing(name)[1] == 0]
assert not missing, missing
fake = C.CDLL(afx.LIB_PATH)
assert all(fake.fake_messages_launches(k, 0) > 0 for k in range(4)), [fake.fake_messages_launches(k, 0) for k in range(4)]
ctx.close()
print("ok")
"""


def test_every_launch_kind_relocates_and_is_dispatched(hostsim_lib):
    env = dict(os.environ, AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT, "lib": hostsim_lib, "names": KIND_NAMES}], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-5000:])
