"""The user's doors of blind issuance on bytes on the device (aeonflux_amd/csrc/wire_blind_user.cpp): afx_blind_request_wire and
afx_unblind_issuances_wire with their _rng and group forms against the column path (afx_blind_request + the packer,
afx_unblind_issuances on the unpacked columns), the yardstick tests/blind_ref.py and the plain credential, and the whole blind protocol
on bytes.  The 300-item cases of tests/test_gpu_blind.Case, one per layout, are shared by every test here; counts 1, 70 (more than a
wave, no multiple of 64) and 300 (past the 256-item plan switch) take their first items, and the yardstick runs on items 0 and cnt - 1.

The slices: afx_ctx_set_chunk_items takes nothing below 256, so 300 items make two slices and 600 in two sections of one layout a
third, on the lane the first one used."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

from tests.test_gpu_blind import COUNTS, GPU_LAYOUTS, ISS, Case
from tests.test_gpu_blind_wire import A2_KINDS, A_KINDS, B_KINDS, DAMAGE_LAYOUT, damaged, records, rnd_of

pytestmark = pytest.mark.gpu

N8 = (8, [0, 1, 2, 4, 3, 1, 4, 0])
ELL = (1 << 252) + 27742317777372353535851937790883648493
PREFIX = b"aeonflux-amd/device-rng/v1"


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


def layout_of(kinds):
    return sum(1 for k in kinds if k in (1, 4)), sum(1 for k in kinds if k == 1)


def hdr_of(n):
    return (24 + n + 31) & ~31


def cells_of(kinds):
    h, hs = layout_of(kinds)
    return 3 + 2 * h + hs + len(kinds)


def group_of(case, kinds, lo, hi):
    """items [lo, hi) of the case's values under `kinds` (a layout over them) as a group of the request door"""
    h, _ = layout_of(kinds)
    c = np.ascontiguousarray
    return dict(kinds=list(kinds), values=c(case.values[:, lo:hi]), d=c(case.d[lo:hi]), r_wide=c(case.r_wide[:h, lo:hi]), rng_seed=c(case.req_seed[lo:hi]))


def column_request(ctx, g):
    """the column path of one group: (AFXQ section, statuses)"""
    from aeonflux_amd import batch, wire
    req, st = batch.blind_request(ctx, g["kinds"], g["values"], g["d"], g["r_wide"], g["rng_seed"])
    return wire.pack_blind_requests(g["kinds"], g["values"], req), st


def column_unblind(ctx, kinds, values, d, afxq, afxj):
    """the column path of one pair of sections: (t, U, V, statuses)"""
    from aeonflux_amd import batch, wire
    _, _, req = wire.unpack_blind_requests(afxq)
    _, iss = wire.unpack_blind_issuances(afxj)
    V, st = batch.unblind_issuances(ctx, kinds, values, d, req, iss)
    t, U = iss["t"].copy(), iss["U"].copy()
    t[st != 0] = 0          # the door zeroes all three for an item that failed
    U[st != 0] = 0
    return t, U, V, st


def sections(blob):
    from aeonflux_amd import wire
    out = []
    while blob:
        k = wire.blind_section_bytes(blob)
        out.append(blob[:k])
        blob = blob[k:]
    return out


# ---- 1. the request door equals the column path and the yardstick ----
@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("n,kinds", GPU_LAYOUTS)
def test_request_door_equals_the_column_path_and_the_yardstick(cases, n, kinds, cnt):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    case = cases(n, kinds)
    g = group_of(case, kinds, 0, cnt)
    h, hs = layout_of(kinds)
    try:
        for mode in (2, 0):
            case.user.set_secret_independent_addressing(mode)
            want, st_col = column_request(case.user, g)
            got, status = wire.blind_request_wire(case.user, [g])
            assert status.tolist() == [0] * cnt and st_col.tolist() == [0] * cnt, mode
            assert got == want, mode
            rec = records(got, hdr_of(n), cells_of(kinds))
            assert rec.shape[0] == cnt
            for i in sorted({0, cnt - 1}):
                req = case.reference(i)[0]
                revealed = b"".join(case.c["items"][i]["values"][p] for p in range(n) if kinds[p] not in (1, 4))
                assert rec[i].tobytes() == req["D"] + b"".join(req["A"]) + b"".join(req["B"]) + req["challenge"] + b"".join(req["responses"]) + revealed, (mode, i)
            n_out, nr, count, off = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
            k_out = (C.c_uint8 * 32)()
            afx.check(afx.lib().afx_blind_request_wire_parse(got, len(got), C.byref(n_out), k_out, C.byref(nr), C.byref(count), C.byref(off)))
            assert (n_out.value, nr.value, count.value, off.value, list(k_out)[:n]) == (n, 1 + h + hs, cnt, hdr_of(n), list(kinds))
    finally:
        case.user.set_secret_independent_addressing(2)


# ---- 2. failing items fail alone ----
def test_failing_request_items_fail_alone_with_zero_records(cases):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 70
    g = group_of(case, kinds, 0, cnt)
    clean, st0 = wire.blind_request_wire(case.user, [g])
    assert not st0.any()
    bad = dict(g, d=g["d"].copy(), values=g["values"].copy())
    bad["d"][5] = 0xFF               # not canonical
    bad["values"][1, 20] = 0         # a PUBLIC_POINT ...
    bad["values"][1, 20, 0] = 1      # ... whose s = 1 is negative: ristretto255 decodes no such string
    bad["d"][41] = 0                 # D would be the identity
    done = [5, 20, 41]
    got, status = wire.blind_request_wire(case.user, [bad])
    want, st_col = column_request(case.user, bad)
    assert status.tolist() == st_col.tolist()
    assert [i for i in range(cnt) if status[i]] == done and {int(status[i]) for i in done} == {afx.ST_MAC_CREATION}
    rec, ref = records(got, 32, cells_of(kinds)), records(clean, 32, cells_of(kinds))
    for i in range(cnt):
        if i in done:
            assert not rec[i].any(), i
        else:
            assert np.array_equal(rec[i], ref[i]), i
    assert got[:32] == clean[:32]


# ---- 3. the unblinding door equals the column path and the plain credential ----
@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("n,kinds", GPU_LAYOUTS)
def test_unblind_door_equals_the_column_path_and_the_plain_credential(cases, n, kinds, cnt):
    from aeonflux_amd import batch, wire
    case = cases(n, kinds)
    x = case.inputs(cnt)
    g = group_of(case, kinds, 0, cnt)
    afxq, st = wire.blind_request_wire(case.user, [g])
    assert not st.any()
    afxj, st = wire.issue_blind_wire(case.issuer, afxq, rnd_of(x))
    assert not st.any()
    plain, st = batch.issue(case.issuer, kinds, x["values"], x["t_wide"], x["U_wide"], x["iss_seed"])
    assert not st.any()
    try:
        for mode in (2, 0):
            case.user.set_secret_independent_addressing(mode)
            t, U, V, st_col = column_unblind(case.user, kinds, x["values"], x["d"], afxq, afxj)
            got, status = wire.unblind_issuances_wire(case.user, afxj, afxq, x["d"])
            assert status.tolist() == [0] * cnt and st_col.tolist() == [0] * cnt, mode
            for f, col in (("t", t), ("U", U), ("V", V)):
                assert got[f].shape == (cnt, 32) and np.array_equal(got[f], col), (mode, f)
                assert np.array_equal(got[f], plain[f]), (mode, f)
    finally:
        case.user.set_secret_independent_addressing(2)


# ---- 4. damaged issuances, and the zero records of refused requests ----
def test_damaged_issuances_fail_alone_with_zero_credentials(cases):
    from aeonflux_amd import wire
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 70
    x = case.inputs(cnt)
    afxq, st = wire.blind_request_wire(case.user, [group_of(case, kinds, 0, cnt)])
    assert not st.any()
    afxj, st = wire.issue_blind_wire(case.issuer, afxq, rnd_of(x))
    assert not st.any()
    clean, st = wire.unblind_issuances_wire(case.user, afxj, afxq, x["d"])
    assert not st.any()
    _, iss = wire.unpack_blind_issuances(afxj)
    iss = {f: iss[f].copy() for f in ISS}
    iss["S1"][4, 9] ^= 0x04
    iss["S2"][11, 30] ^= 0x01
    iss["challenge"][23, 0] ^= 0x80
    iss["responses"][2, 37, 17] ^= 0x20
    iss["t"][50] = 0xFF              # not canonical
    done = [4, 11, 23, 37, 50]
    bad = wire.pack_blind_issuances(kinds, iss)
    got, status = wire.unblind_issuances_wire(case.user, bad, afxq, x["d"])
    t, U, V, st_col = column_unblind(case.user, kinds, x["values"], x["d"], afxq, bad)
    assert status.tolist() == st_col.tolist() and np.array_equal(got["V"], V)
    assert [i for i in range(cnt) if status[i]] == done and {int(status[i]) for i in done} == {1}
    for f in ("t", "U", "V"):
        for i in range(cnt):
            if i in done:
                assert not got[f][i].any(), (f, i)
            else:
                assert np.array_equal(got[f][i], clean[f][i]), (f, i)
    # the zero records the issuer's door writes for the requests it refused: status 1 at exactly those indices
    values, req, refused = damaged(case)
    afxj2, st_iss = wire.issue_blind_wire(case.issuer, wire.pack_blind_requests(kinds, values, req), rnd_of(x))
    assert [i for i in range(cnt) if st_iss[i]] == sorted(refused)
    got2, status2 = wire.unblind_issuances_wire(case.user, afxj2, afxq, x["d"])
    assert [i for i in range(cnt) if status2[i]] == sorted(refused) and {int(status2[i]) for i in refused} == {1}
    for f in ("t", "U", "V"):
        for i in range(cnt):
            assert np.array_equal(got2[f][i], np.zeros(32, np.uint8) if i in refused else clean[f][i]), (f, i)


# ---- 5. streams: layouts interleaved, a wrong-n group, a count-0 group; slices ----
class Mixed:
    """groups in order A(30), B(5), wrong-n(4), A'(3), A(30), a count-0 group of B, B(2), over the values of the DAMAGE_LAYOUT case"""

    def __init__(self, case):
        rng = np.random.default_rng(5)
        junk = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
        plan = [(A_KINDS, 0, 30), (B_KINDS, 30, 35), (None, 0, 4), (A2_KINDS, 35, 38), (A_KINDS, 38, 68), (B_KINDS, 0, 0), (B_KINDS, 68, 70)]
        self.groups = []
        for kinds, lo, hi in plan:
            if kinds is None:          # two attributes against a context of four: whatever the arrays hold
                self.groups.append(dict(kinds=[2, 1], values=junk(2, 4, 32), d=junk(4, 32), r_wide=junk(1, 4, 64), rng_seed=junk(4, 32)))
            else:
                self.groups.append(group_of(case, kinds, lo, hi))
        self.counts = [g["values"].shape[1] for g in self.groups]
        self.total = sum(self.counts)
        self.d = np.concatenate([g["d"] for g in self.groups])
        self.rnd = rnd_of(case.inputs(self.total))


def test_streams_of_several_layouts_equal_per_section_column_calls(cases):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    case = cases(*DAMAGE_LAYOUT)
    m = Mixed(case)
    assert m.total == 74
    afxq, status = wire.blind_request_wire(case.user, m.groups)
    secs = sections(afxq)
    assert len(secs) == len(m.groups) and len(status) == m.total
    first = 0
    for k, (g, c, sec) in enumerate(zip(m.groups, m.counts, secs)):
        kinds = g["kinds"]
        h, hs = layout_of(kinds)
        assert sec[:24] == b"AFXQ" + struct.pack("<5I", 1, c, cells_of(kinds), len(kinds), 1 + h + hs) and sec[24:32] == bytes(kinds) + bytes(8 - len(kinds)), k
        assert len(sec) == 32 + c * cells_of(kinds) * 32, k
        st = status[first:first + c]
        if len(kinds) != 4:
            assert st.tolist() == [afx.ST_MAC_CREATION] * c and not any(sec[32:]), k
        elif c:
            want, st_col = column_request(case.user, g)
            assert sec == want and st.tolist() == st_col.tolist() == [0] * c, k
        first += c
    # the issuer answers the stream; the unblinding door merges the pairs of one layout and gives each section the column call's answer
    afxj, st_iss = wire.issue_blind_wire(case.issuer, afxq, m.rnd)
    assert st_iss.tolist() == [0] * 35 + [afx.ST_MAC_CREATION] * 4 + [0] * 35
    got, status = wire.unblind_issuances_wire(case.user, afxj, afxq, m.d)
    assert status.tolist() == [0] * 35 + [afx.ST_VERIFICATION_FAILURE] * 4 + [0] * 35
    first = 0
    for k, (g, c, q, j) in enumerate(zip(m.groups, m.counts, secs, sections(afxj))):
        mine = {f: got[f][first:first + c] for f in ("t", "U", "V")}
        if len(g["kinds"]) != 4:
            assert not any(mine[f].any() for f in mine), k
        elif c:
            t, U, V, st_col = column_unblind(case.user, g["kinds"], g["values"], g["d"], q, j)
            assert not st_col.any() and np.array_equal(mine["t"], t) and np.array_equal(mine["U"], U) and np.array_equal(mine["V"], V), k
        first += c


def test_several_slices_give_the_unsliced_bytes(cases):
    from aeonflux_amd import wire
    n, kinds = N8
    case, cnt = cases(n, kinds), 300
    x = case.inputs(cnt)
    g = group_of(case, kinds, 0, cnt)
    g2 = dict(g, d=np.ascontiguousarray(g["d"][::-1]))          # the second section: the same values under other one-time keys
    seed = bytes(range(32))
    rnd = rnd_of(x)
    twice = {f: np.concatenate([rnd[f], rnd[f][::-1]]) for f in rnd}
    d2 = np.concatenate([g["d"], g2["d"]])

    def run():
        out = {}
        out["q1"] = wire.blind_request_wire(case.user, [g])
        out["q2"] = wire.blind_request_wire(case.user, [g, g2])
        out["q3"] = wire.blind_request_wire_rng(case.user, [g, g2], seed, 6)
        return out
    want = run()
    assert all(not v[1].any() for v in want.values())
    j1, st = wire.issue_blind_wire(case.issuer, want["q1"][0], rnd)
    j2, st2 = wire.issue_blind_wire(case.issuer, want["q2"][0], twice)
    j3, st3 = wire.issue_blind_wire(case.issuer, want["q3"][0], twice)
    assert not st.any() and not st2.any() and not st3.any()

    def unblind():
        return [wire.unblind_issuances_wire(case.user, j1, want["q1"][0], g["d"]), wire.unblind_issuances_wire(case.user, j2, want["q2"][0], d2),
                wire.unblind_issuances_wire_rng(case.user, j3, want["q3"][0], seed, 6)]
    want_u = unblind()
    assert all(not st.any() for _, st in want_u)
    try:
        case.user.set_chunk_items(256)          # 300 items: two slices; 600 in two sections: three, on lanes 0, 1, 0
        got, got_u = run(), unblind()
    finally:
        case.user.set_chunk_items(0)
    for k in want:
        assert got[k][0] == want[k][0] and got[k][1].tolist() == want[k][1].tolist(), k
    assert np.array_equal(got["q3"][2], want["q3"][2])
    assert got["q2"][0][:len(want["q1"][0])] == want["q1"][0]
    for (a, sa), (b, sb) in zip(got_u, want_u):
        assert sa.tolist() == sb.tolist() and all(np.array_equal(a[f], b[f]) for f in ("t", "U", "V"))
    assert np.array_equal(want_u[1][0]["V"][:cnt], want_u[0][0]["V"])


# ---- 6. argument errors write nothing ----
def test_argument_errors_leave_every_output_untouched(cases):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    from aeonflux_amd.wire import _blind_request_groups
    case = cases(*DAMAGE_LAYOUT)
    lib = afx.lib()
    m = Mixed(case)
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    arr, keep = _blind_request_groups(m.groups, True)
    bare, _ = _blind_request_groups([dict(kinds=g["kinds"], values=np.zeros((len(g["kinds"]), 0, 32), np.uint8), count=c) for g, c in zip(m.groups, m.counts)], False)
    afx.check(lib.afx_blind_request_wire(case.user.h, bare, len(m.groups), None, 0, C.byref(out_len), None, 0, C.byref(cnt)))          # the size query needs no arrays
    size, total = out_len.value, cnt.value
    assert total == m.total and size == sum(32 + c * cells_of(g["kinds"]) * 32 for g, c in zip(m.groups, m.counts))
    out, status = np.full(size, 0xEE, np.uint8), np.full(total, 0xEE, np.uint8)
    call = lambda a, cap, scap: lib.afx_blind_request_wire(case.user.h, a, len(m.groups), out.ctypes.data, cap, C.byref(out_len), status.ctypes.data, scap, C.byref(cnt))
    assert call(arr, size - 1, total) == afx.E_BAD_ARGS
    assert call(arr, size, total - 1) == afx.E_BAD_ARGS
    five, keep5 = _blind_request_groups(m.groups, True)
    five[3].attrs.kinds[1] = 5
    assert call(five, size, total) == afx.E_BAD_ARGS
    assert (out == 0xEE).all() and (status == 0xEE).all()
    afx.check(call(arr, size, total))
    afxq = out[:out_len.value].tobytes()
    again, st_again = wire.blind_request_wire(case.user, m.groups)
    assert afxq == again and status.tolist() == st_again.tolist()
    afxj, _ = wire.issue_blind_wire(case.issuer, afxq, m.rnd)
    # the unblinding door
    cols = [np.full((total, 32), 0xEE, np.uint8) for _ in range(3)]
    st = np.full(total, 0xEE, np.uint8)
    co = afx.CredentialOut(*(a.ctypes.data for a in cols))
    d = np.ascontiguousarray(m.d)
    ucall = lambda j, q, scap=total: lib.afx_unblind_issuances_wire(case.user.h, j, len(j), q, len(q), d.ctypes.data, C.byref(co), st.ctypes.data, scap, C.byref(cnt))
    qs, js = sections(afxq), sections(afxj)
    other_count = wire.pack_blind_issuances(B_KINDS, {f: wire.unpack_blind_issuances(js[6])[1][f][..., :1, :] for f in ISS})
    other_kind = js[6][:24] + bytes([3, 3, 2, 0]) + js[6][28:]
    table = {"fewer issuance sections": (b"".join(js[:-1]), afxq), "fewer request sections": (afxj, b"".join(qs[:-1])),
             "a pair differing in count": (b"".join(js[:-1]) + other_count, afxq), "a pair differing in one kind": (b"".join(js[:-1]) + other_kind, afxq),
             "a truncated AFXJ": (afxj[:-1], afxq)}
    for what, (j, q) in table.items():
        assert ucall(j, q) == afx.E_BAD_ARGS, what
        assert all((a == 0xEE).all() for a in cols) and (st == 0xEE).all(), what
    assert ucall(afxj, afxq, total - 1) == afx.E_BAD_ARGS
    assert all((a == 0xEE).all() for a in cols) and (st == 0xEE).all()
    afx.check(ucall(afxj, afxq))
    assert cnt.value == total and st.tolist() == [0] * 35 + [afx.ST_VERIFICATION_FAILURE] * 4 + [0] * 35


# ---- 7. draws ----
def shake_draws(seed, stream, first, count, h):
    """(d [count,32], r_wide [h,count,64], rng_seed [count,32]) of the items at stream indices first .. first + count"""
    import aeonflux_amd as afx
    draw = lambda i, label, w: hashlib.shake_256(PREFIX + seed + struct.pack("<QQB", stream, i, label)).digest(w)
    u8 = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), w)
    idx = range(first, first + count)
    d = u8([(int.from_bytes(draw(i, afx.DRAW_BLINDREQ_D_WIDE, 64), "little") % ELL).to_bytes(32, "little") for i in idx], 32)
    r_wide = np.stack([u8([draw(i, afx.DRAW_BLINDREQ_R_WIDE(j), 64) for i in idx], 64) for j in range(h)]) if h else np.zeros((0, count, 64), np.uint8)
    return d, r_wide, u8([draw(i, afx.DRAW_BLINDREQ_SEED, 32) for i in idx], 32)


def test_rng_forms_are_the_explicit_doors_on_shake256_draws(cases):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    n, kinds = DAMAGE_LAYOUT
    case = cases(n, kinds)
    seed, stream = hashlib.sha256(b"blind user wire rng").digest(), (1 << 40) + 3
    # two layouts in three groups: the draws follow the item's index in the stream, whatever group it stands in
    plan = [(A_KINDS, 0, 40), (B_KINDS, 40, 47), (A_KINDS, 47, 70)]
    bare = [dict(kinds=k, values=np.ascontiguousarray(case.values[:, lo:hi])) for k, lo, hi in plan]
    drawn = []
    for g, (k, lo, hi) in zip(bare, plan):
        d, r_wide, rng_seed = shake_draws(seed, stream, lo, hi - lo, layout_of(k)[0])
        drawn.append(dict(g, d=d, r_wide=r_wide, rng_seed=rng_seed))
    got, st, d = wire.blind_request_wire_rng(case.user, bare, seed, stream)
    want, st_want = wire.blind_request_wire(case.user, drawn)
    assert st.tolist() == st_want.tolist() == [0] * 70 and got == want
    assert np.array_equal(d, np.concatenate([g["d"] for g in drawn]))
    again, _, none = wire.blind_request_wire_rng(case.user, bare, seed, stream, keep_d=False)
    assert again == got and none is None
    afxj, st_iss = wire.issue_blind_wire_rng(case.issuer, got, seed, 77)
    assert not st_iss.any()
    a, st_a = wire.unblind_issuances_wire_rng(case.user, afxj, got, seed, stream)
    b, st_b = wire.unblind_issuances_wire(case.user, afxj, got, d)
    assert st_a.tolist() == st_b.tolist() == [0] * 70 and all(np.array_equal(a[f], b[f]) for f in ("t", "U", "V")) and a["V"].any(axis=1).all()
    wrong, st_w = wire.unblind_issuances_wire_rng(case.user, afxj, got, seed, stream + 1)          # another stream: another d, no credential
    assert len(st_w) == 70 and not any(np.array_equal(wrong["V"][i], a["V"][i]) for i in range(70))
    # no seed: one from getrandom per call - two calls differ, and both flows complete
    q1, s1, d1 = wire.blind_request_wire_rng(case.user, bare)
    q2, s2, d2 = wire.blind_request_wire_rng(case.user, bare, None, 0)
    assert not s1.any() and not s2.any() and q1 != q2 and not np.array_equal(d1, d2)
    for q, dd in ((q1, d1), (q2, d2)):
        j, sj = wire.issue_blind_wire_rng(case.issuer, q)
        cred, su = wire.unblind_issuances_wire(case.user, j, q, dd)
        assert sj.tolist() == [0] * 70 and su.tolist() == [0] * 70 and cred["V"].any(axis=1).all()
    with pytest.raises(afx.AfxError) as e:
        wire.blind_request_wire_rng(case.user, bare, None, 0, keep_d=False)
    assert e.value.rc == afx.E_BAD_ARGS
    with pytest.raises(afx.AfxError) as e:
        wire.unblind_issuances_wire_rng(case.user, afxj, got, None, stream)
    assert e.value.rc == afx.E_BAD_ARGS


# ---- 8. the whole blind protocol on bytes ----
def test_the_whole_blind_protocol_on_bytes(cases):
    from aeonflux_amd import batch, wire
    n, kinds = N8
    case, cnt = cases(n, kinds), 70
    seed = hashlib.sha256(b"blind protocol on bytes").digest()
    values = np.ascontiguousarray(case.values[:, :cnt])
    afxq, st, _ = wire.blind_request_wire_rng(case.user, [dict(kinds=kinds, values=values)], seed, 1, keep_d=False)
    assert st.tolist() == [0] * cnt
    afxj, st = wire.issue_blind_wire_rng(case.issuer, afxq, seed, 2)
    assert st.tolist() == [0] * cnt
    cred, st = wire.unblind_issuances_wire_rng(case.user, afxj, afxq, seed, 1)
    assert st.tolist() == [0] * cnt
    full = [it["full_values"] for it in case.c["items"][:cnt]]
    part = lambda lo: np.stack([np.frombuffer(b"".join(v[p][lo:lo + 32] if kinds[p] == 4 else bytes(32) for v in full), np.uint8).reshape(cnt, 32) for p in range(n)])
    rng = np.random.default_rng(1416)
    rb = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    kp = batch.keypairs_derive(case.user, rb(cnt, 64))
    item = dict(kinds=kinds, values=values, t=cred["t"], U=cred["U"], V=cred["V"], keypairs=kp, z_wide=rb(cnt, 64), rng_seed=rb(cnt, 32), enc_seeds=rb(2, cnt, 32),
                M2=part(32), m3=part(64))
    try:
        # the strict statement: the reference's own reads a compact index as a position and refuses layouts like this one whoever issued them
        case.user.set_strict(1)
        case.issuer.set_strict(1)
        afxp, _, st = wire.show_wire(case.user, [item])
        assert st.tolist() == [0] * cnt
        verdicts = wire.verify_mixed_wire(case.issuer, afxp)
    finally:
        case.user.set_strict(0)
        case.issuer.set_strict(0)
    assert verdicts.tolist() == [0] * cnt


# ---- 9. a group ----
def test_group_forms_give_the_one_context_bytes(cases):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    from tests.test_gpu_group import _devices
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 300
    x = case.inputs(cnt)
    # two layouts, the first in two groups: the unblinding door merges those and splits the merged batch over the members
    groups = [group_of(case, A_KINDS, 0, 140), group_of(case, B_KINDS, 140, 160), group_of(case, A_KINDS, 160, 300)]
    small = [group_of(case, B_KINDS, 0, 5)]
    seed = hashlib.sha256(b"blind user wire group").digest()

    def run(ctx, issuer):
        out = {}
        for name, gs, c in (("large", groups, cnt), ("small", small, 5)):
            q, sq = wire.blind_request_wire(ctx, gs)
            qr, sqr, d = wire.blind_request_wire_rng(ctx, gs, seed, 21)
            rnd = rnd_of(case.inputs(c))
            j, sj = wire.issue_blind_wire(issuer, q, rnd)
            jr, sjr = wire.issue_blind_wire(issuer, qr, rnd)
            u, su = wire.unblind_issuances_wire(ctx, j, q, np.concatenate([g["d"] for g in gs]))
            ur, sur = wire.unblind_issuances_wire_rng(ctx, jr, qr, seed, 21)
            for s in (sq, sqr, sj, sjr, su, sur):
                assert s.tolist() == [0] * c, name
            out[name] = (q, qr, d.tobytes(), u["t"].tobytes(), u["U"].tobytes(), u["V"].tobytes(), ur["t"].tobytes(), ur["U"].tobytes(), ur["V"].tobytes())
        return out
    want = run(case.user, case.issuer)
    g = afx.Group(case.c["params"], case.c["key"], case.c["ip"], _devices())
    try:
        for k in range(len(g)):
            g.member(k).set_small_batch_items(64)          # 300 items: every group or merged batch is split; 5 go whole to one member
        got = run(g, case.issuer)
    finally:
        g.close()
    for name in want:
        for k, (a, b) in enumerate(zip(got[name], want[name])):
            assert a == b, (name, k)
    assert want["large"][0] != want["large"][1]
