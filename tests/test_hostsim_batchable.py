"""CPU-only: the batchable entry points on the engine's host half, built against the fake HIP runtime under ASan/UBSan like
tests/test_hostsim.py, with its own source list: the engine's eight host sources, tests/hostsim/fake_hip.cpp and the stand-ins for
the two new launchers (tests/hostsim/fake_batchable.cpp).  Every layout that test drives, strict mode on and off, the latency and
the large-pass plans, null arguments - and the derived operation counts of the one-sum-per-item plan (afx_ctx_get_plan_stats is
computed on the host)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def hostsim_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_batchable") / "libafx_hostsim.so")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp")]
    srcs.append(os.path.join(CSRC, "wire_batchable.cpp"))
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_batchable.cpp", "fake_wire_issue.cpp")]
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
from aeonflux_amd import batch, wire
from tests.helpers import make_credentials
from tests.batchable_ref import LARGEST_COEF_JOB_16_STRICT
longest = {}
rb = lambda *s: np.zeros(s, np.uint8)
for strict in (0, 1):
    for n, layout, hide in ((4, "SSPE", [0, 3]), (16, "SSSSSSSSPPPPEEEE", [12, 13, 14, 15]), (8, "SSPPEEEE", [4, 5, 6, 7]), (1, "S", []), (3, "ESS", [0])):
        d = make_credentials(n, layout, 3, b"hostsim-batchable-%%d" %% n)
        ctx = afx.Context(d["params"], d["key"], d["ip"])
        ctx.set_strict(strict)
        creds = d["creds"]
        values = np.stack([np.stack([np.frombuffer(c["values"][i][:32], np.uint8) for c in creds]) for i in range(n)])
        k2 = list(creds[0]["kinds"])
        for i in hide:
            k2[i] = 1 if k2[i] == 0 else 4
        nsp = sum(1 for k in k2 if k == 4)
        kp = {f: rb(3, 32) for f in ("a", "a0", "a1", "pk")}
        args = (k2, values, rb(3, 32), rb(3, 32), rb(3, 32), kp, rb(3, 64), rb(3, 32), rb(max(nsp, 1), 3, 32), values, values)
        sh0 = batch.shape_of_kinds(k2)
        n_main = afx.lib().afx_batchable_main_commitments(ctx.h, C.byref(sh0))
        assert n_main >= 2, (strict, layout, n_main)
        pres, cm, shape, st = batch.show_batchable(ctx, *args)
        assert bytes(shape) == bytes(sh0) and cm["main"].shape == (n_main, 3, 32) and len(cm["enc"]) == nsp
        for small in (4096, 0):          # the latency plan and the plan of large passes
            ctx.set_small_batch_items(small)
            for secret in (0, 1, 2):
                ctx.set_secret_independent_addressing(secret)
                batch.verify_presentations_batchable(ctx, shape, pres, cm, bytes(32))
            ctx.set_fixed_key_schedule(1)
            batch.verify_presentations_batchable(ctx, shape, pres, cm, None)       # (a seed of the library's own)
            ctx.set_fixed_key_schedule(0)
            ctx.set_plan_variants(afx.VARIANT_SELFCHECK)
            batch.verify_presentations_batchable(ctx, shape, pres, cm, bytes(32))
            ctx.set_plan_variants(0)
        ctx.set_small_batch_items(4096)
        longest[(strict, layout)] = C.CDLL(afx.LIB_PATH).fake_coef_most_triples(1)     # the longest coefficient job of these plans
        # no challenge arrays at all
        nochal = dict(pres, challenge=None, enc=[dict(e, challenge=None) for e in pres["enc"]])
        batch.verify_presentations_batchable(ctx, shape, nochal, cm, bytes(32))
        # the challenge trace receives the squeezed challenges; too small a buffer is refused
        ctx.set_challenge_trace(1 + nsp, 3)
        batch.verify_presentations_batchable(ctx, shape, pres, cm, bytes(32))
        ctx.set_challenge_trace(1, 2)
        try:
            batch.verify_presentations_batchable(ctx, shape, pres, cm, bytes(32))
            raise SystemExit("trace overflow accepted")
        except afx.AfxError as e:
            assert e.rc == afx.E_BAD_ARGS
        ctx.set_challenge_trace(0, 0)
        # null arguments and arrays
        soa, keep = batch.presentation_soa({f: (pres[f] if f != "enc" else pres[f]) for f in pres})
        csoa, keep2 = batch.commitments_soa(cm)
        rng = batch.device_rng(bytes(32))
        stt = rb(3)
        L = afx.lib()
        assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), None, C.byref(rng), 3, stt.ctypes.data) == afx.E_BAD_ARGS
        assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), None, C.byref(csoa), C.byref(rng), 3, stt.ctypes.data) == afx.E_BAD_ARGS
        assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), 3, None) == afx.E_BAD_ARGS
        assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), C.byref(csoa), None, 3, stt.ctypes.data) == 0
        assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), 0, stt.ctypes.data) == 0
        nomain = afx.CommitmentsSoA(None, csoa.enc)
        assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), C.byref(nomain), C.byref(rng), 3, stt.ctypes.data) == afx.E_BAD_ARGS
        assert L.afx_batchable_main_commitments(None, C.byref(shape)) == 0 and L.afx_batchable_main_commitments(ctx.h, None) == 0
        # the *_dev entry points directly (the fake runtime's device memory is host memory), a missing proof's commitments, no commitments_out
        assert L.afx_verify_presentations_batchable_dev(ctx.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), 3, stt.ctypes.data) == 0
        if nsp:
            holes = (C.c_void_p * nsp)(*([None] + [a.ctypes.data for a in cm["enc"][1:]]))
            noenc = afx.CommitmentsSoA(csoa.main, C.cast(holes, C.POINTER(C.c_void_p)))
            assert L.afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), C.byref(noenc), C.byref(rng), 3, stt.ctypes.data) == afx.E_BAD_ARGS
            assert L.afx_verify_presentations_batchable_dev(ctx.h, C.byref(shape), C.byref(soa), C.byref(noenc), C.byref(rng), 3, stt.ctypes.data) == afx.E_BAD_ARGS
        cs, kpp, rnd, out, o, cnt, keep3 = batch._show_args(*args)
        sho = afx.Shape()
        for fn in (L.afx_show_batchable, L.afx_show_batchable_dev):
            assert fn(ctx.h, C.byref(cs), C.byref(kpp), C.byref(rnd), 3, C.byref(out), None, C.byref(sho), stt.ctypes.data) == afx.E_BAD_ARGS
            assert fn(ctx.h, C.byref(cs), C.byref(kpp), C.byref(rnd), 3, C.byref(out), C.byref(nomain), C.byref(sho), stt.ctypes.data) == afx.E_BAD_ARGS
        assert L.afx_show_batchable_dev(ctx.h, C.byref(cs), C.byref(kpp), C.byref(rnd), 3, C.byref(out), C.byref(csoa), C.byref(sho), stt.ctypes.data) == 0
        # the two wire doors: size query (out == NULL), the call, the stream back through the verifier's door, malformed streams
        item = dict(kinds=k2, values=values, t=rb(3, 32), U=rb(3, 32), V=rb(3, 32), keypairs=kp, z_wide=rb(3, 64), rng_seed=rb(3, 32),
                    enc_seeds=rb(max(nsp, 1), 3, 32), M2=values, m3=values)
        blob, shapes, stw = wire.show_batchable_wire(ctx, [item, dict(item, positions=[5, 4, 3])])
        assert len(stw) == 6 and bytes(shapes[0]) == bytes(shape) and blob[:4] == b"AFXB"
        assert len(blob) == 2 * len(wire.pack_batchable(shape, pres, cm))
        assert len(wire.verify_batchable_wire(ctx, blob, bytes(32))) == 6
        assert len(wire.verify_batchable_wire(ctx, blob, None)) == 6
        cntw = C.c_size_t(0)
        assert L.afx_verify_presentations_batchable_wire(ctx.h, blob[:-1], len(blob) - 1, C.byref(rng), stt.ctypes.data, 3, C.byref(cntw)) == afx.E_BAD_ARGS
        assert L.afx_verify_presentations_batchable_wire(ctx.h, blob, len(blob), C.byref(rng), stt.ctypes.data, 3, C.byref(cntw)) == afx.E_BAD_ARGS and cntw.value == 6
        assert L.afx_verify_presentations_batchable_wire(ctx.h, blob, len(blob), C.byref(rng), None, 0, None) == afx.E_BAD_ARGS
        assert L.afx_verify_presentations_batchable_wire(ctx.h, None, 0, C.byref(rng), stt.ctypes.data, 3, C.byref(cntw)) == afx.E_BAD_ARGS
        nokey = dict(item, keypairs=None)
        if nsp:
            b3, _, st3 = wire.show_batchable_wire(ctx, [nokey])
            assert st3.tolist() == [afx.ST_NO_SYMMETRIC_KEY] * 3 and not any(b3[L.afx_batchable_wire_header_bytes(C.byref(shape)):])
        # shapes every item fails on: answered without reading an array, and the prover has no batchable form for them
        bad = afx.Shape.from_buffer_copy(bytes(shape))
        bad.n_responses += 1
        assert L.afx_batchable_main_commitments(ctx.h, C.byref(bad)) == 0
        assert batch.verify_presentations_batchable(ctx, bad, pres, cm, bytes(32)).tolist() == [1, 1, 1]
        ctx.close()

# the job length tests/test_batchable_coef_on_host.py runs the kernel's arithmetic at is the plan's
assert longest[(1, "SSSSSSSSPPPPEEEE")] == LARGEST_COEF_JOB_16_STRICT == max(longest.values()), longest
print("longest coefficient jobs", longest)

# operation counts of the C3 shape in the plan of large passes: derived bounds, not measurements
d = make_credentials(8, "SSPPEEEE", 3, b"hostsim-batchable-counts")
ctx = afx.Context(d["params"], d["key"], d["ip"])
ctx.set_small_batch_items(0)
creds = d["creds"]
values = np.stack([np.stack([np.frombuffer(c["values"][i][:32], np.uint8) for c in creds]) for i in range(8)])
k2 = [0, 0, 2, 2, 4, 4, 4, 4]
kp = {f: rb(3, 32) for f in ("a", "a0", "a1", "pk")}
pres, cm, shape, st = batch.show_batchable(ctx, k2, values, rb(3, 32), rb(3, 32), rb(3, 32), kp, rb(3, 64), rb(3, 32), rb(4, 3, 32), values, values)
batch.verify_presentations(ctx, shape, pres)
compact = ctx.plan_stats()
batch.verify_presentations_batchable(ctx, shape, pres, cm, bytes(32))
b = ctx.plan_stats()
n_commitments = cm["main"].shape[0] + 5 * len(cm["enc"])
assert n_commitments == 26, n_commitments
J = b["msm_jobs"] - 1                       # the jobs the combined sum was split into (the other one is Z)
assert 1 <= J <= 3, b
print("compact", compact)
print("batchable", b)
assert b["doublings"] <= 252 * (1 + J), b
assert b["encodings"] <= compact["encodings"] - n_commitments + 1, (b, compact)
assert b["field_mul"] + b["field_sq"] < compact["field_mul"] + compact["field_sq"], (b, compact)
assert b["decodings"] == compact["decodings"] + n_commitments
ctx.close()
print("ok")
"""


def test_batchable_entry_points_and_operation_counts(hostsim_lib):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    # AFX_PLAN_SELFCHECK: every plan is assembled twice against different provisional addresses and must relocate to identical bytes
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT, "lib": hostsim_lib}], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-5000:])
