"""CPU-only: the blind-issuance entry points on the engine's host half, built against the fake HIP runtime under ASan/UBSan like
tests/test_hostsim_batchable.py, with its own source list: the engine's host sources plus statements_blind.cpp, tests/hostsim/fake_hip.cpp
and the stand-in for the output-masking launcher (tests/hostsim/fake_blind.cpp).  All four calls are assembled for every layout of
tests/test_blind_ref.py - the latency plan and the plan of large passes, every secret mode, the fixed key schedule, every plan variant,
AFX_VARIANT_SELFCHECK among them (and AFX_PLAN_SELFCHECK for the whole run: every plan is assembled twice and must relocate to the
same bytes) - and a table of bad arguments is refused."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def hostsim_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_blind") / "libafx_hostsim.so")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "statements_blind.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_blind.cpp", "fake_wire_issue.cpp")]
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
from tests.test_blind_ref import LAYOUTS
L = afx.lib()
fake = C.CDLL(afx.LIB_PATH)
fake.fake_mask_rows_seen.restype = C.c_uint64
rb = lambda *s: np.zeros(s, np.uint8)
CNT = 3
for n, kinds in LAYOUTS + [(2, [0, 2])]:
    d = make_credentials(n, "S" * n, 1, b"hostsim-blind-%%d" %% n)
    issuer = afx.Context(d["params"], d["key"], d["ip"])
    user = afx.Context(d["params"], None, d["ip"])
    h, hs = batch.blind_layout(kinds)
    values = rb(n, CNT, 32)

    def flow(passes=1, CNT=CNT):
        values = rb(n, CNT, 32)
        stats = {}
        fake.fake_mask_rows_seen(1)
        req, st = batch.blind_request(user, kinds, values, rb(CNT, 32), rb(h, CNT, 64), rb(CNT, 32))
        assert req["responses"].shape == (1 + h + hs, CNT, 32) and len(st) == CNT
        assert fake.fake_mask_rows_seen(1) == passes * (3 + 3 * h + hs)          # every output row of the call was given to the masking
        stats["request"] = user.plan_stats()["secret_terms"]
        batch.verify_blind_requests(user, kinds, req)
        stats["verify"] = user.plan_stats()["secret_terms"]
        assert fake.fake_mask_rows_seen(1) == 0
        iss, st = batch.issue_blind(issuer, kinds, values, req, rb(CNT, 64), rb(CNT, 64), rb(CNT, 64), rb(CNT, 32))
        assert iss["responses"].shape == (n + 6, CNT, 32)
        assert fake.fake_mask_rows_seen(1) == passes * (n + 11)
        stats["issue"] = issuer.plan_stats()["secret_terms"]
        V, st = batch.unblind_issuances(user, kinds, values, rb(CNT, 32), req, iss)
        assert fake.fake_mask_rows_seen(1) == passes
        stats["unblind"] = user.plan_stats()["secret_terms"]
        return req, iss, stats

    for small in (4096, 0):                    # the latency plan and the plan of large passes
        for c in (issuer, user):
            c.set_small_batch_items(small)
        for secret in (2, 1, 0):
            for c in (issuer, user):
                c.set_secret_independent_addressing(secret)
            req, iss, stats = flow()
            if secret == 2:
                assert stats["request"] > 0 and stats["issue"] > 0 and stats["unblind"] > 0 and stats["verify"] == 0, stats
            if secret == 0 and small == 0:
                assert not any(stats.values()), stats
        for c in (issuer, user):
            c.set_secret_independent_addressing(2)
        issuer.set_fixed_key_schedule(1)
        flow()
        issuer.set_fixed_key_schedule(0)
        for variants in (afx.VARIANT_SELFCHECK, 0x79, 0x7a, 0x7c, 0x01 | 0x40, 0x02 | 0x40, 0x04 | 0x08 | 0x40, 0x10 | 0x20 | 0x40):   # (0x79, 0x7a, 0x7c: AFX_VARIANT_ALL with one SEGMENTS choice)
            for c in (issuer, user):
                c.set_plan_variants(variants)
            req, iss, stats = flow()
            assert stats["request"] > 0 and stats["issue"] > 0 and stats["unblind"] > 0 and stats["verify"] == 0, (variants, stats)
        for c in (issuer, user):
            c.set_plan_variants(0)
    for c in (issuer, user):
        c.set_small_batch_items(4096)
    # two passes of one call
    for c in (issuer, user):
        c.set_chunk_items(256)
    flow(passes=2, CNT=300)
    for c in (issuer, user):
        c.set_chunk_items(0)

    # ---- the *_dev entry points directly (the fake runtime's device memory is host memory) and the table of bad arguments ----
    a = batch._blind_attrs(kinds, values, batch._hptr)
    rq = afx.BlindRequestSoA(*(batch._hptr(req[f]) for f in batch.REQUEST_FIELDS))
    rws, rseed = rb(h, CNT, 64), rb(CNT, 32)
    rr = afx.BlindRequestRandomness(batch._hptr(rws), rseed.ctypes.data)
    wides = [rb(CNT, 64) for _ in range(3)] + [rb(CNT, 32)]
    ir = afx.BlindIssueRandomness(*(w.ctypes.data for w in wides))
    io = afx.BlindIssuanceSoA(*(iss[f].ctypes.data for f in batch.BLIND_ISSUANCE_FIELDS))
    dd, V, stt = rb(CNT, 32), rb(CNT, 32), rb(CNT)
    nrq, nri = 1 + h + hs, n + 6
    for sfx in ("", "_dev"):
        f_req, f_ver, f_iss, f_unb = (getattr(L, name + sfx) for name in ("afx_blind_request", "afx_verify_blind_requests", "afx_issue_blind", "afx_unblind_issuances"))
        ok = [lambda: f_req(user.h, C.byref(a), dd.ctypes.data, C.byref(rr), CNT, C.byref(rq), stt.ctypes.data),
              lambda: f_ver(user.h, C.byref(a), C.byref(rq), nrq, CNT, stt.ctypes.data),
              lambda: f_iss(issuer.h, C.byref(a), C.byref(rq), nrq, C.byref(ir), CNT, C.byref(io), stt.ctypes.data),
              lambda: f_unb(user.h, C.byref(a), dd.ctypes.data, C.byref(rq), C.byref(io), nri, CNT, V.ctypes.data, stt.ctypes.data)]
        for call in ok:
            assert call() == 0, afx.last_error() if hasattr(afx, "last_error") else sfx
        bad = [
            # null arguments
            (lambda: f_req(None, C.byref(a), dd.ctypes.data, C.byref(rr), CNT, C.byref(rq), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_req(user.h, None, dd.ctypes.data, C.byref(rr), CNT, C.byref(rq), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_req(user.h, C.byref(a), None, C.byref(rr), CNT, C.byref(rq), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_req(user.h, C.byref(a), dd.ctypes.data, None, CNT, C.byref(rq), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_req(user.h, C.byref(a), dd.ctypes.data, C.byref(rr), CNT, None, stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_req(user.h, C.byref(a), dd.ctypes.data, C.byref(rr), CNT, C.byref(rq), None), afx.E_BAD_ARGS),
            (lambda: f_ver(user.h, C.byref(a), None, nrq, CNT, stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_ver(user.h, C.byref(a), C.byref(rq), nrq, CNT, None), afx.E_BAD_ARGS),
            (lambda: f_iss(issuer.h, C.byref(a), None, nrq, C.byref(ir), CNT, C.byref(io), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_iss(issuer.h, C.byref(a), C.byref(rq), nrq, None, CNT, C.byref(io), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_iss(issuer.h, C.byref(a), C.byref(rq), nrq, C.byref(ir), CNT, None, stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_unb(user.h, C.byref(a), None, C.byref(rq), C.byref(io), nri, CNT, V.ctypes.data, stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_unb(user.h, C.byref(a), dd.ctypes.data, C.byref(rq), C.byref(io), nri, CNT, None, stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_unb(user.h, C.byref(a), dd.ctypes.data, C.byref(rq), None, nri, CNT, V.ctypes.data, stt.ctypes.data), afx.E_BAD_ARGS),
            # a context without the key cannot issue
            (lambda: f_iss(user.h, C.byref(a), C.byref(rq), nrq, C.byref(ir), CNT, C.byref(io), stt.ctypes.data), afx.E_NO_KEY),
            # null arrays of a well-formed call
            (lambda: f_req(user.h, C.byref(a), dd.ctypes.data, C.byref(rr), CNT, C.byref(afx.BlindRequestSoA(None, rq.A, rq.B, rq.challenge, rq.responses)), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_ver(user.h, C.byref(a), C.byref(afx.BlindRequestSoA(rq.D, rq.A, rq.B, None, rq.responses)), nrq, CNT, stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_iss(issuer.h, C.byref(a), C.byref(rq), nrq, C.byref(afx.BlindIssueRandomness(ir.t_wide, ir.U_wide, None, ir.rng_seed)), CNT, C.byref(io), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_iss(issuer.h, C.byref(a), C.byref(rq), nrq, C.byref(ir), CNT, C.byref(afx.BlindIssuanceSoA(io.t, io.U, None, io.S2, io.challenge, io.responses)), stt.ctypes.data), afx.E_BAD_ARGS),
            (lambda: f_unb(user.h, C.byref(a), dd.ctypes.data, C.byref(rq), C.byref(afx.BlindIssuanceSoA(io.t, io.U, io.S1, None, io.challenge, io.responses)), nri, CNT, V.ctypes.data, stt.ctypes.data), afx.E_BAD_ARGS),
        ]
        if h:
            bad.append((lambda: f_ver(user.h, C.byref(a), C.byref(afx.BlindRequestSoA(rq.D, None, rq.B, rq.challenge, rq.responses)), nrq, CNT, stt.ctypes.data), afx.E_BAD_ARGS))
            bad.append((lambda: f_unb(user.h, C.byref(a), dd.ctypes.data, C.byref(afx.BlindRequestSoA(rq.D, rq.A, None, None, None)), C.byref(io), nri, CNT, V.ctypes.data, stt.ctypes.data), afx.E_BAD_ARGS))
        for k, (call, want) in enumerate(bad):
            got = call()
            assert got == want, (sfx, k, got, want)
        # an empty batch is no work
        assert f_ver(user.h, C.byref(a), C.byref(rq), nrq, 0, stt.ctypes.data) == 0

        # whole shapes: every item gets the call's code and zeros
        def every(code):
            if sfx == "_dev":          # the statuses of a plan come from the fake k_finish, which answers 0x5a for every item: only the
                code = 0x5a            # host-answered shapes show their code here; the outputs' zeros below are checked in both forms
            assert stt.tolist() == [code] * CNT, (sfx, stt.tolist(), code)
        short = batch._blind_attrs(kinds[:-1] if n > 1 else kinds + [0], values, batch._hptr)
        unknown = batch._blind_attrs(kinds[:-1] + [5], values, batch._hptr)
        for wrong in (short, unknown):
            for arr in (req["D"], iss["S1"], iss["S2"], V):
                arr[:] = 7
            stt[:] = 9
            assert f_req(user.h, C.byref(wrong), dd.ctypes.data, C.byref(rr), CNT, C.byref(rq), stt.ctypes.data) == 0
            every(afx.ST_MAC_CREATION)
            assert not req["D"].any()
            assert f_ver(user.h, C.byref(wrong), C.byref(rq), nrq, CNT, stt.ctypes.data) == 0
            every(afx.ST_VERIFICATION_FAILURE)
            assert f_iss(issuer.h, C.byref(wrong), C.byref(rq), nrq, C.byref(ir), CNT, C.byref(io), stt.ctypes.data) == 0
            every(afx.ST_MAC_CREATION)
            assert not iss["S1"].any() and not iss["S2"].any() and not iss["responses"].any()
            assert f_unb(user.h, C.byref(wrong), dd.ctypes.data, C.byref(rq), C.byref(io), nri, CNT, V.ctypes.data, stt.ctypes.data) == 0
            every(afx.ST_VERIFICATION_FAILURE)
            assert not V.any()
        # a wrong response count
        iss["S1"][:] = 7
        V[:] = 7
        assert f_ver(user.h, C.byref(a), C.byref(rq), nrq + 1, CNT, stt.ctypes.data) == 0
        every(afx.ST_VERIFICATION_FAILURE)
        assert f_iss(issuer.h, C.byref(a), C.byref(rq), nrq - 1, C.byref(ir), CNT, C.byref(io), stt.ctypes.data) == 0
        every(afx.ST_VERIFICATION_FAILURE)
        assert not iss["S1"].any()
        assert f_unb(user.h, C.byref(a), dd.ctypes.data, C.byref(rq), C.byref(io), nri - 1, CNT, V.ctypes.data, stt.ctypes.data) == 0
        every(afx.ST_VERIFICATION_FAILURE)
        assert not V.any()
    issuer.close()
    user.close()
print("ok")
"""


def test_blind_entry_points_assemble_and_refuse_bad_arguments(hostsim_lib):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    # AFX_PLAN_SELFCHECK: every plan is assembled twice against different provisional addresses and must relocate to identical bytes
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT, "lib": hostsim_lib}], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-5000:])
