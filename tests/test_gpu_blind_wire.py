"""Blind issuance on bytes on the device (aeonflux_amd/csrc/wire_blind.cpp): afx_issue_blind_wire and its _rng and group forms and
afx_verify_blind_requests_wire against the column path (afx_issue_blind + the packers), the yardstick tests/blind_ref.py and the
plain credential.  Requests are made on the GPU (batch.blind_request) from the 300-item cases of tests/test_gpu_blind.Case, one per
layout and shared by every test here; counts 1, 70 (more than a wave, no multiple of 64) and 300 (past the 256-item plan switch) take
their first items.

The passes test: afx_ctx_set_chunk_items refuses anything below 256 (statements.cpp), so 256 is the smallest pass there is: 300
requests make two slices - and, to run a third slice on the lane the first one used, 600 requests in two sections of one layout."""
import ctypes as C
import hashlib
import struct
import threading

import numpy as np
import pytest

from tests.test_gpu_blind import COUNTS, GPU_LAYOUTS, ISS, REQ, Case

pytestmark = pytest.mark.gpu

RND = (("t_wide", 64), ("U_wide", 64), ("rprime_wide", 64), ("rng_seed", 32))
DAMAGE_LAYOUT = (4, [4, 2, 3, 1])          # positions 0 - 2 hold points, position 3 a scalar
A_KINDS, A2_KINDS, B_KINDS = [4, 2, 3, 1], [2, 4, 3, 0], [3, 3, 2, 1]          # three layouts over the same values


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, kinds):
        key = (n, tuple(kinds))
        if key not in made:
            made[key] = Case(n, kinds)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def rnd_of(x, lo=0, hi=None):
    return {"t_wide": x["t_wide"][lo:hi], "U_wide": x["U_wide"][lo:hi], "rprime_wide": x["rprime_wide"][lo:hi], "rng_seed": x["iss_seed"][lo:hi]}


def issuer_view(case, values):
    """the values as the issuer gets them: 0xEE in the rows of hidden positions, which nothing reads"""
    v = values.copy()
    for i in case.H:
        v[i] = 0xEE
    return v


def records(blob, hdr, cells):
    return np.frombuffer(blob, np.uint8, offset=hdr).reshape(-1, cells * 32)


def column_path(ctx, kinds, values, req, rnd):
    from aeonflux_amd import batch, wire
    iss, st = batch.issue_blind(ctx, kinds, values, req, rnd["t_wide"], rnd["U_wide"], rnd["rprime_wide"], rnd["rng_seed"])
    return wire.pack_blind_issuances(kinds, iss), st, iss


def request_of(case, kinds, lo, hi):
    """requests of items [lo, hi) of `case` under `kinds` (a layout over the case's values), made on the GPU"""
    from aeonflux_amd import batch
    h = sum(1 for k in kinds if k in (1, 4))
    values = np.ascontiguousarray(case.values[:, lo:hi])
    req, st = batch.blind_request(case.user, kinds, values, case.d[lo:hi], np.ascontiguousarray(case.r_wide[:h, lo:hi]), case.req_seed[lo:hi])
    assert not st.any()
    return values, req


# ---- 1. byte equality with the column path, the yardstick and the plain credential ----
@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("n,kinds", GPU_LAYOUTS)
def test_bytes_equal_the_column_path_the_yardstick_and_the_plain_credential(cases, n, kinds, cnt):
    from aeonflux_amd import batch, wire
    case = cases(n, kinds)
    x = case.inputs(cnt)
    good = case.flow(cnt, keep=True)
    assert not good["st"][0].any()
    rnd = rnd_of(x)
    blob = wire.pack_blind_requests(kinds, issuer_view(case, x["values"]), good["req"])
    plain, st = batch.issue(case.issuer, kinds, x["values"], x["t_wide"], x["U_wide"], x["iss_seed"])
    assert not st.any()
    try:
        for mode in (2, 0):
            case.issuer.set_secret_independent_addressing(mode)
            want, st_col, _ = column_path(case.issuer, kinds, x["values"], good["req"], rnd)
            got, status = wire.issue_blind_wire(case.issuer, blob, rnd)
            assert status.tolist() == [0] * cnt and st_col.tolist() == [0] * cnt, mode
            assert got == want, mode
            rec = records(got, 32 if n <= 8 else 64, n + 11)
            for i in sorted({0, cnt - 1}):
                iss = case.reference(i)[1]
                assert rec[i].tobytes() == b"".join(iss[f] for f in ISS[:5]) + b"".join(iss["responses"]), (mode, i)
            k2, iss2 = wire.unpack_blind_issuances(got)
            assert k2 == list(kinds)
            V, st_unb = batch.unblind_issuances(case.user, kinds, x["values"], x["d"], good["req"], iss2)
            assert st_unb.tolist() == [0] * cnt and np.array_equal(V, plain["V"]), mode
            assert np.array_equal(iss2["t"], plain["t"]) and np.array_equal(iss2["U"], plain["U"]), mode
    finally:
        case.issuer.set_secret_independent_addressing(2)


# ---- 2. damaged requests: the column call's verdicts, zeros for the failed, the others untouched ----
def damaged(case, cnt=70):
    """70 requests of DAMAGE_LAYOUT, five of them damaged in one cell each -> (values as the issuer gets them, request, {item: what})"""
    x = case.inputs(cnt)
    good = case.flow(cnt, keep=True)
    req = {f: good["req"][f].copy() for f in REQ}
    values = issuer_view(case, x["values"])
    req["challenge"][3, 7] ^= 0x10
    req["A"][1, 10] = 0xFF          # s >= p: no canonical field element, so no point
    req["D"][20] = 0               # the identity's encoding: refused in a transcript
    req["responses"][2, 33] = 0xFF
    values[1, 47] = 0              # a revealed PUBLIC_POINT ...
    values[1, 47, 0] = 1           # ... whose s = 1 is negative (odd): ristretto255 decodes no such string
    return values, req, {3: "challenge bit", 10: "A", 20: "D zero", 33: "response ff", 47: "revealed point"}


def test_damaged_requests_fail_alone_and_get_zero_records(cases):
    from aeonflux_amd import wire
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 70
    x = case.inputs(cnt)
    rnd = rnd_of(x)
    good = case.flow(cnt, keep=True)
    clean, st0 = wire.issue_blind_wire(case.issuer, wire.pack_blind_requests(kinds, x["values"], good["req"]), rnd)
    assert not st0.any()
    values, req, done = damaged(case)
    got, status = wire.issue_blind_wire(case.issuer, wire.pack_blind_requests(kinds, values, req), rnd)
    want, st_col, _ = column_path(case.issuer, kinds, values, req, rnd)
    assert status.tolist() == st_col.tolist()
    assert [i for i in range(cnt) if status[i]] == sorted(done), status.tolist()
    assert {int(status[i]) for i in done} == {1}          # AFX_ST_VERIFICATION_FAILURE, whatever was wrong with the request
    assert got == want
    rec, ref = records(got, 32, n + 11), records(clean, 32, n + 11)
    for i in range(cnt):
        if i in done:
            assert not rec[i].any(), (i, done[i])
        else:
            assert np.array_equal(rec[i], ref[i]), i
    assert got[:32] == clean[:32]


# ---- 3. a mixed stream ----
class Mixed:
    """sections in order A(30), B(5), wrong-n(4), A'(3), A(30), a count-0 section of B, B(2), over the values of the DAMAGE_LAYOUT case"""

    def __init__(self, case):
        from aeonflux_amd import wire
        rng = np.random.default_rng(3)
        junk = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
        plan = [(A_KINDS, 0, 30), (B_KINDS, 30, 35), (None, 0, 4), (A2_KINDS, 35, 38), (A_KINDS, 38, 68), (B_KINDS, 0, 0), (B_KINDS, 68, 70)]
        self.parts = []          # (kinds, count, section bytes, values, request)
        for kinds, lo, hi in plan:
            if kinds is None:          # two attributes against a context of four: whatever the records hold
                kinds = [2, 1]
                values, req = junk(2, hi - lo, 32), dict(D=junk(4, 32), A=junk(1, 4, 32), B=junk(1, 4, 32), challenge=junk(4, 32), responses=junk(3, 4, 32))
            else:
                values, req = request_of(case, kinds, lo, hi)
            self.parts.append((list(kinds), hi - lo, wire.pack_blind_requests(kinds, values, req), values, req))
        self.stream = b"".join(p[2] for p in self.parts)
        self.total = sum(p[1] for p in self.parts)
        x = case.inputs(self.total)
        self.rnd = rnd_of(x)


@pytest.fixture(scope="module")
def mixed(cases):
    return Mixed(cases(*DAMAGE_LAYOUT))


def check_mixed_answer(mixed, got, status, alone):
    """`alone`: section -> (bytes, statuses) of the door on that section by itself with its slice of the randomness"""
    import aeonflux_amd as afx
    n = 4
    assert len(status) == mixed.total == 74
    assert len(got) == sum(32 + c * (n + 11) * 32 for _, c, *_ in mixed.parts)
    off = first = 0
    for k, (kinds, c, sec, values, req) in enumerate(mixed.parts):
        size = 32 + c * (n + 11) * 32
        mine = got[off:off + size]
        assert mine[:24] == b"AFXJ" + struct.pack("<5I", 1, c, n + 11, len(kinds), n + 6), k
        assert mine[24:32] == bytes(kinds) + bytes(8 - len(kinds)), k
        want, st = alone(k, sec, first, c)
        assert mine == want and status[first:first + c].tolist() == st.tolist(), k
        if len(kinds) != n:
            assert st.tolist() == [afx.ST_MAC_CREATION] * c and not any(mine[32:]), k
        else:
            assert not st.any(), k
        off += size
        first += c
    assert off == len(got)


def test_mixed_stream_order_headers_and_per_section_bytes(cases, mixed):
    from aeonflux_amd import wire
    case = cases(*DAMAGE_LAYOUT)
    got, status = wire.issue_blind_wire(case.issuer, mixed.stream, mixed.rnd)

    def alone(k, sec, first, c):
        return wire.issue_blind_wire(case.issuer, sec, {f: mixed.rnd[f][first:first + c] for f, _ in RND})
    check_mixed_answer(mixed, got, status, alone)
    # ... and each section alone is the column path (the layouts other than A's are nowhere else in this file)
    first = 0
    for kinds, c, sec, values, req in mixed.parts:
        if len(kinds) == 4 and c:
            want, st, _ = column_path(case.issuer, kinds, values, req, {f: mixed.rnd[f][first:first + c] for f, _ in RND})
            assert wire.issue_blind_wire(case.issuer, sec, {f: mixed.rnd[f][first:first + c] for f, _ in RND})[0] == want and not st.any(), kinds
        first += c


# ---- 4. several passes ----
def test_several_slices_give_the_default_settings_bytes(cases):
    from aeonflux_amd import wire
    n, kinds = 8, [0, 1, 2, 4, 3, 1, 4, 0]
    case, cnt = cases(n, kinds), 300
    x = case.inputs(cnt)
    good = case.flow(cnt, keep=True)
    one = wire.pack_blind_requests(kinds, x["values"], good["req"])
    rnd = rnd_of(x)
    twice = {f: np.concatenate([rnd[f], rnd[f][::-1]]) for f, _ in RND}
    seed = bytes(range(32))
    want, st = wire.issue_blind_wire(case.issuer, one, rnd)
    want2, st2 = wire.issue_blind_wire(case.issuer, one + one, twice)
    want3, st3 = wire.issue_blind_wire_rng(case.issuer, one + one, seed, 4)
    assert not st.any() and not st2.any() and not st3.any()
    try:
        case.issuer.set_chunk_items(256)          # 300 requests: two slices; 600 in two sections: three, on lanes 0, 1, 0
        got, st = wire.issue_blind_wire(case.issuer, one, rnd)
        got2, st2 = wire.issue_blind_wire(case.issuer, one + one, twice)
        got3, st3 = wire.issue_blind_wire_rng(case.issuer, one + one, seed, 4)
    finally:
        case.issuer.set_chunk_items(0)
    assert not st.any() and not st2.any() and not st3.any()
    assert got == want and got2 == want2 and got3 == want3
    assert got2[:len(want)] == want


# ---- 5. randomness drawn on the device ----
PREFIX = b"aeonflux-amd/device-rng/v1"


def shake_draws(seed, stream, total):
    import aeonflux_amd as afx
    labels = (afx.DRAW_BLIND_T_WIDE, afx.DRAW_BLIND_U_WIDE, afx.DRAW_BLIND_RPRIME_WIDE, afx.DRAW_BLIND_ISSUE_SEED)
    assert labels == (65, 66, 67, 68) and [afx.draw_bytes(l) for l in labels] == [64, 64, 64, 32]
    out = {}
    for (f, w), label in zip(RND, labels):
        rows = [hashlib.shake_256(PREFIX + seed + struct.pack("<QQB", stream, i, label)).digest(w) for i in range(total)]
        out[f] = np.frombuffer(b"".join(rows), np.uint8).reshape(total, w) if total else np.zeros((0, w), np.uint8)
    return out


def test_rng_form_is_the_explicit_door_on_shake256_draws(cases, mixed):
    from aeonflux_amd import batch, wire
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 70
    x = case.inputs(cnt)
    good = case.flow(cnt, keep=True)
    blob = wire.pack_blind_requests(kinds, x["values"], good["req"])
    seed = hashlib.sha256(b"blind wire rng").digest()
    for stream_no, (b, total) in ((0, (blob, cnt)), (1 << 40, (mixed.stream, mixed.total))):
        got, st = wire.issue_blind_wire_rng(case.issuer, b, seed, stream_no)
        want, st_want = wire.issue_blind_wire(case.issuer, b, shake_draws(seed, stream_no, total))
        assert got == want and st.tolist() == st_want.tolist(), stream_no
    assert not st_want[:30].any()
    # no seed: one from getrandom per call - two calls differ, and both are issuances the user accepts
    a, st_a = wire.issue_blind_wire_rng(case.issuer, blob)
    b2, st_b = wire.issue_blind_wire_rng(case.issuer, blob, None, 0)
    assert not st_a.any() and not st_b.any() and a[:32] == b2[:32] and a != b2
    ra, rb_ = records(a, 32, n + 11), records(b2, 32, n + 11)
    assert all(not np.array_equal(ra[i], rb_[i]) for i in range(cnt))
    for answer in (a, b2):
        V, st_unb = batch.unblind_issuances(case.user, kinds, x["values"], x["d"], good["req"], wire.unpack_blind_issuances(answer)[1])
        assert st_unb.tolist() == [0] * cnt and V.any(axis=1).all()


def test_rng_form_argument_errors_are_the_explicit_calls_and_write_nothing(cases, mixed):
    import aeonflux_amd as afx
    case = cases(*DAMAGE_LAYOUT)
    lib = afx.lib()
    stream, total = mixed.stream, mixed.total
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    rng = afx.DeviceRng(bytes(range(1, 33)), 5)
    afx.check(lib.afx_issue_blind_wire_rng(case.issuer.h, stream, len(stream), C.byref(rng), None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    size = out_len.value
    assert cnt.value == total
    r = afx.BlindIssueRandomness(*(np.ascontiguousarray(mixed.rnd[f]).ctypes.data for f, _ in RND))
    out, status = np.full(size, 0xEE, np.uint8), np.full(total, 0xEE, np.uint8)
    keyless = case.user.h
    table = [dict(cap=size - 1), dict(scap=total - 1), dict(blob=stream[:-1]), dict(h=keyless), dict(r=None)]
    for kw in table:
        codes = []
        for fn, rr in ((lib.afx_issue_blind_wire, r), (lib.afx_issue_blind_wire_rng, rng)):
            blob = kw.get("blob", stream)
            arg = None if "r" in kw else C.byref(rr)
            codes.append(fn(kw.get("h", case.issuer.h), blob, len(blob), arg, out.ctypes.data, kw.get("cap", size), C.byref(out_len), status.ctypes.data, kw.get("scap", total),
                            C.byref(cnt)))
        assert codes[0] == codes[1] == (afx.E_NO_KEY if "h" in kw else afx.E_BAD_ARGS), (list(kw), codes)
        assert (out == 0xEE).all() and (status == 0xEE).all(), list(kw)


# ---- 6. sizes, short buffers, a keyless context, a malformed last section ----
def test_size_query_short_buffers_a_keyless_context_and_a_malformed_last_section(cases, mixed):
    import aeonflux_amd as afx
    case = cases(*DAMAGE_LAYOUT)
    lib = afx.lib()
    stream, total = mixed.stream, mixed.total
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    afx.check(lib.afx_issue_blind_wire(case.issuer.h, stream, len(stream), None, None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    assert cnt.value == total == 74 and out_len.value == 7 * 32 + 74 * 15 * 32
    size = out_len.value
    afx.check(lib.afx_issue_blind_wire(case.user.h, stream, len(stream), None, None, 0, C.byref(out_len), None, 0, C.byref(cnt)))          # the size query needs no key
    assert (out_len.value, cnt.value) == (size, total)
    arrs = [np.ascontiguousarray(mixed.rnd[f]) for f, _ in RND]
    r = afx.BlindIssueRandomness(*(a.ctypes.data for a in arrs))
    out, status = np.full(size, 0xEE, np.uint8), np.full(total, 0xEE, np.uint8)
    args = lambda h, blob, cap, scap: (h, blob, len(blob), C.byref(r), out.ctypes.data, cap, C.byref(out_len), status.ctypes.data, scap, C.byref(cnt))
    assert lib.afx_issue_blind_wire(*args(case.issuer.h, stream, size - 1, total)) == afx.E_BAD_ARGS
    assert lib.afx_issue_blind_wire(*args(case.issuer.h, stream, size, total - 1)) == afx.E_BAD_ARGS
    assert lib.afx_issue_blind_wire(*args(case.user.h, stream, size, total)) == afx.E_NO_KEY
    last = mixed.parts[-1][2]
    for broken in (stream[:-1], stream[:-len(last)] + last[:20] + struct.pack("<I", 7) + last[24:], stream + b"AFXQ" + bytes(28)):
        assert lib.afx_issue_blind_wire(*args(case.issuer.h, broken, size + 64, total)) == afx.E_BAD_ARGS
        vst = np.full(total + 1, 0xEE, np.uint8)
        assert lib.afx_verify_blind_requests_wire(case.user.h, broken, len(broken), vst.ctypes.data, vst.size, C.byref(cnt)) == afx.E_BAD_ARGS
        assert (vst == 0xEE).all()
    for k in range(4):
        ptrs = [a.ctypes.data for a in arrs]
        ptrs[k] = None
        hole = afx.BlindIssueRandomness(*ptrs)
        assert lib.afx_issue_blind_wire(case.issuer.h, stream, len(stream), C.byref(hole), out.ctypes.data, size, C.byref(out_len), status.ctypes.data, total,
                                        C.byref(cnt)) == afx.E_BAD_ARGS, k
    assert (out == 0xEE).all() and (status == 0xEE).all()
    afx.check(lib.afx_issue_blind_wire(*args(case.issuer.h, stream, size, total)))
    assert (out_len.value, cnt.value) == (size, total) and status.tolist() == [0] * 35 + [afx.ST_MAC_CREATION] * 4 + [0] * 35


# ---- 7. the verification alone ----
def test_verify_wire_gives_the_column_calls_statuses_section_by_section(cases, mixed):
    import aeonflux_amd as afx
    from aeonflux_amd import batch, wire
    n, kinds = DAMAGE_LAYOUT
    case = cases(n, kinds)
    values, req, done = damaged(case)
    got = wire.verify_blind_requests_wire(case.user, wire.pack_blind_requests(kinds, values, req))
    want = batch.verify_blind_requests(case.user, kinds, req)
    assert got.tolist() == want.tolist()
    # (a damaged REVEALED value is the issuer's business, not the request proof's: it is in no transcript of the request)
    assert [i for i in range(70) if got[i]] == sorted(i for i in done if done[i] != "revealed point")
    for ctx in (case.user, case.issuer):
        got = wire.verify_blind_requests_wire(ctx, mixed.stream)
        want = np.concatenate([batch.verify_blind_requests(ctx, k, q) if c else np.zeros(0, np.uint8) for k, c, _, _, q in mixed.parts])
        assert got.tolist() == want.tolist()
        assert got.tolist() == [0] * 35 + [afx.ST_VERIFICATION_FAILURE] * 4 + [0] * 35


# ---- 8. a group ----
def test_group_gives_the_one_context_bytes(cases):
    import torch
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    n, kinds = DAMAGE_LAYOUT
    case = cases(n, kinds)
    c = case.c
    devices = list(range(torch.cuda.device_count())) or [0]
    if len(devices) == 1:
        devices = [0, 0]
    count = 5000          # above the small-call bound: every merged batch is split over the members
    good = case.flow(70, keep=True)
    idx = np.arange(count) % 70
    big_values = np.ascontiguousarray(case.values[:, idx])
    big_req = {f: np.ascontiguousarray(good["req"][f][..., idx, :]) for f in REQ}
    cut = lambda lo, hi: (np.ascontiguousarray(big_values[:, lo:hi]), {f: np.ascontiguousarray(big_req[f][..., lo:hi, :]) for f in REQ})
    b_values, b_req = request_of(case, B_KINDS, 0, 5)
    small = wire.pack_blind_requests(B_KINDS, b_values, b_req)
    stream = wire.pack_blind_requests(kinds, *cut(0, 3000)) + small + wire.pack_blind_requests(kinds, *cut(3000, count))
    rng = np.random.default_rng(8)
    rnd = {f: rng.integers(0, 256, size=(count + 5, w), dtype=np.uint8) for f, w in RND}
    seed = hashlib.sha256(b"blind wire group").digest()
    want, st1 = wire.issue_blind_wire(case.issuer, stream, rnd)
    want_rng, st1r = wire.issue_blind_wire_rng(case.issuer, stream, seed, 11)
    want_small, st3 = wire.issue_blind_wire(case.issuer, small, rnd)
    want_small_rng, st3r = wire.issue_blind_wire_rng(case.issuer, small, seed, 12)
    g = afx.Group(c["params"], c["key"], c["ip"], devices)
    try:
        got, st2 = wire.issue_blind_wire(g, stream, rnd)
        got_rng, st2r = wire.issue_blind_wire_rng(g, stream, seed, 11)
        got_small, st4 = wire.issue_blind_wire(g, small, rnd)
        got_small_rng, st4r = wire.issue_blind_wire_rng(g, small, seed, 12)
    finally:
        g.close()
    assert st1.tolist() == [0] * (count + 5) and st2.tolist() == st1.tolist() and got == want
    assert st1r.tolist() == [0] * (count + 5) and st2r.tolist() == st1r.tolist() and got_rng == want_rng and got_rng != got
    assert st3.tolist() == [0] * 5 and st4.tolist() == st3.tolist() and got_small == want_small
    assert st4r.tolist() == st3r.tolist() == [0] * 5 and got_small_rng == want_small_rng


# ---- 9. threads on one context ----
def test_eight_threads_on_one_context_get_what_each_call_gives_alone(cases):
    from aeonflux_amd import wire
    n, kinds = DAMAGE_LAYOUT
    case = cases(n, kinds)
    good = case.flow(70, keep=True)
    seed = hashlib.sha256(b"blind wire threads").digest()

    def blob_of(t, r):
        lo = 8 * t + 2 * r          # three requests from item lo on (neighbouring streams overlap; each has its own stream number)
        return wire.pack_blind_requests(kinds, np.ascontiguousarray(case.values[:, lo:lo + 3]), {f: np.ascontiguousarray(good["req"][f][..., lo:lo + 3, :]) for f in REQ})
    alone = {(t, r): wire.issue_blind_wire_rng(case.issuer, blob_of(t, r), seed, 100 * t + r) for t in range(8) for r in range(3)}
    assert all(not st.any() for _, st in alone.values())
    errs, results = [], {}

    def work(t):
        try:
            for r in range(3):
                results[(t, r)] = wire.issue_blind_wire_rng(case.issuer, blob_of(t, r), seed, 100 * t + r)
        except BaseException as e:   # noqa: an error in a thread must fail the test
            errs.append((t, repr(e)[:400]))
    ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs[:3]
    for key, (want, st) in alone.items():
        got, st2 = results[key]
        assert got == want and st2.tolist() == st.tolist(), key
    assert len({alone[k][0] for k in alone}) == 24          # every (stream, requests) pair its own bytes
