"""Whole messages on the device (include/aeonflux_gpu.h "whole messages"; aeonflux_amd/csrc/messages.cuh, statements_messages.cpp):
every byte against tests/messages_ref.py, the yardstick composed from the oracle, and every call in both its host-pointer and its
*_dev form.  What the tests aim at is where the feature can go wrong: a message's chunks lie in several passes of the per-chunk plans
(afx_ctx_set_chunk_items), so a message's status and the zeroing of a failed message are decided behind the last pass."""
import hashlib

import numpy as np
import pytest

from tests import messages_ref as ref

pytestmark = pytest.mark.gpu
L_BYTES = bytes.fromhex("edd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010")   # l itself: the least non-canonical scalar


@pytest.fixture(scope="module")
def user():
    import oracle
    import aeonflux_amd as afx
    st = hashlib.shake_256(b"afx-tests/plaintext-context/v1").digest(1 << 15)
    params, used = oracle.system_parameters_generate(5, st)
    key, ip = oracle.issuer_new(params, st[used:used + 64 * 9])
    ctx = afx.Context(params, None, ip)
    yield ctx, oracle.Ctx(params, None, ip)
    ctx.close()


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def cut(label, lengths):
    src = hashlib.shake_256(label).digest(sum(lengths))
    out, at = [], 0
    for n in lengths:
        out.append(src[at:at + n])
        at += n
    return out


def keys_for(octx, label, n):
    """distinct keypairs, one per message: (oracle's 128 bytes each, dict of [n, 32] rows)"""
    okp = [octx.keypair_derive(hashlib.shake_256(label + b"/%d" % i).digest(64)) for i in range(n)]
    return okp, rows_of_keys(okp)


def rows_of_keys(okp):
    a = np.frombuffer(b"".join(okp), np.uint8).reshape(len(okp), 4, 32)
    return {f: np.ascontiguousarray(a[:, k]) for k, f in enumerate(("a", "a0", "a1", "pk"))}


def arr(rows, width=32):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width).copy() if rows else np.zeros((0, width), np.uint8)


# ---- both forms of every call ---------------------------------------------------------------------------------------------------
def dev(a):
    from tests.helpers import DevMem
    a = np.ascontiguousarray(a).view(np.uint8)
    return DevMem(a) if a.size else DevMem(nbytes=16, fill=0)


class Out:
    """a device output of `shape` bytes, 0xEE before the call (room for one row where the shape is empty)"""
    def __init__(self, *shape, fill=0xEE):
        from tests.helpers import DevMem
        self.shape, self.fill = shape, fill
        self.mem = DevMem(np.full(shape if int(np.prod(shape)) else (32,), fill, np.uint8))
        self.ptr = self.mem.ptr

    def numpy(self):
        got = self.mem.numpy()
        if int(np.prod(self.shape)):
            return got
        assert (got == self.fill).all()           # no row written
        return np.zeros(self.shape, np.uint8)


def from_messages(ctx, messages):
    """afx_plaintexts_from_messages, host and *_dev form (equal, every status 0) -> M1, M2, m3, counters, chunk_first"""
    from aeonflux_amd import batch
    M1, M2, m3, ctr, cf = batch.plaintexts_from_messages(ctx, messages)
    blob, offsets = batch.pack_messages(messages)
    n = int(cf[-1])
    o = [Out(n, 32), Out(n, 32), Out(n, 32), Out(n, 4), Out(n)]
    batch.plaintexts_from_messages_dev(ctx, dev(blob), offsets, *o)
    ctx.synchronize()
    d = [x.numpy() for x in o]
    assert np.array_equal(d[0], M1) and np.array_equal(d[1], M2) and np.array_equal(d[2], m3) and np.array_equal(d[3].view(np.uint32).reshape(n), ctr)
    assert not d[4].any()
    return M1, M2, m3, ctr, cf


def encrypt_messages(ctx, kp, messages):
    """afx_encrypt_messages, host and *_dev form (equal) -> E1, E2, counters, chunk_first, status"""
    from aeonflux_amd import batch
    E1, E2, ctr, cf, st = batch.encrypt_messages(ctx, kp, messages)
    blob, offsets = batch.pack_messages(messages)
    n, cnt = int(cf[-1]), len(cf) - 1
    o = [Out(n, 32), Out(n, 32), Out(n, 4), Out(cnt)]
    batch.encrypt_messages_dev(ctx, {f: dev(kp[f]) for f in ("a", "a0", "a1")}, dev(blob), offsets, *o)
    ctx.synchronize()
    d = [x.numpy() for x in o]
    assert np.array_equal(d[0], E1) and np.array_equal(d[1], E2) and np.array_equal(d[2].view(np.uint32).reshape(n), ctr) and np.array_equal(d[3], st)
    return E1, E2, ctr, cf, st


def decrypt_messages(ctx, kp, E1, E2, cf):
    """afx_decrypt_messages, host and *_dev form (equal), the output 0xA5 before the call -> list of bytes, status"""
    from aeonflux_amd import batch
    msgs, st = batch.decrypt_messages(ctx, kp, E1, E2, cf, fill=0xA5)
    n, cnt = int(cf[-1]), len(cf) - 1
    o = [Out(n, 30, fill=0xA5), Out(cnt, fill=0xA5)]
    batch.decrypt_messages_dev(ctx, {f: dev(kp[f]) for f in ("a", "a0", "a1")}, dev(E1), dev(E2), cf, *o)
    ctx.synchronize()
    d = [x.numpy() for x in o]
    assert batch.split_messages(d[0], cf) == msgs and np.array_equal(d[1], st)
    return msgs, st


def check_plaintext_rows(messages, got):
    M1, M2, m3, ctr, cf = got
    want = ref.plaintexts_from_messages(messages)
    assert cf.tolist() == ref.chunk_first(messages) and len(want) == len(M1) == len(M2) == len(m3) == len(ctr)
    for r, (w1, w2, w3, wc) in enumerate(want):
        assert (M1[r].tobytes(), M2[r].tobytes(), m3[r].tobytes(), int(ctr[r])) == (w1, w2, w3, wc), r


def check_encrypted(okp, messages, got, expect=None):
    """against the yardstick; `expect`: the statuses where the yardstick cannot give them (a non-canonical key is no value of the crate's)"""
    E1, E2, ctr, cf, st = got
    w1, w2, wc, wst = ref.encrypt_messages(okp, messages)
    assert cf.tolist() == ref.chunk_first(messages) and len(w1) == len(E1)
    want_st = wst if expect is None else expect
    assert st.tolist() == want_st
    for i in range(len(messages)):
        for r in range(cf[i], cf[i + 1]):
            if want_st[i]:
                assert not E1[r].any() and not E2[r].any() and ctr[r] == 0, (i, r)
            else:
                assert (E1[r].tobytes(), E2[r].tobytes(), int(ctr[r])) == (w1[r], w2[r], wc[r]), (i, r)


# ---- lengths ----------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 0, 1, 29, 30, 31, 59, 60, 0, 61, 90, 300, 3000, 0]


def length_messages():
    msgs = cut(b"afx-tests/messages/lengths/v1", LENGTHS)
    mid = cut(b"afx-tests/messages/zero-middle/v1", [30, 30])
    msgs[-1:-1] = [mid[0] + bytes(30) + mid[1], b"abc", b"abc\0"]      # (the batch still ends with an empty message)
    assert len(msgs[0]) == len(msgs[1]) == len(msgs[-1]) == 0
    return msgs


def test_lengths(user):
    ctx, octx = user
    msgs = length_messages()
    got = from_messages(ctx, msgs)
    check_plaintext_rows(msgs, got)
    M1, M2, m3, ctr, cf = got
    z = cf[len(msgs) - 4] + 1                       # the middle chunk of thirty zero bytes: the identity at counter 0
    assert msgs[-4][30:60] == bytes(30) and not M1[z].any() and ctr[z] == 0
    a, b = cf[len(msgs) - 3], cf[len(msgs) - 2]     # b"abc" and b"abc\0": the length is not carried
    assert all(np.array_equal(x[a], x[b]) for x in (M1, M2, m3)) and ctr[a] == ctr[b]
    okp, kp = keys_for(octx, b"afx-tests/messages/lengths/key", len(msgs))
    enc = encrypt_messages(ctx, kp, msgs)
    check_encrypted(okp, msgs, enc)
    back, st = decrypt_messages(ctx, kp, enc[0], enc[1], cf)
    assert not st.any() and back == [ref.padded(m) for m in msgs]
    assert (back, st.tolist()) == ref.decrypt_messages(okp, [r.tobytes() for r in enc[0]], [r.tobytes() for r in enc[1]], cf.tolist())


def test_only_empty_messages(user):
    ctx, octx = user
    msgs = [b""] * 5
    M1, M2, m3, ctr, cf = from_messages(ctx, msgs)              # (Out.numpy: the *_dev form wrote no row)
    assert cf.tolist() == [0] * 6 and len(M1) == len(M2) == len(m3) == len(ctr) == 0
    okp, kp = keys_for(octx, b"afx-tests/messages/empty/key", 5)
    E1, E2, c, cf2, st = encrypt_messages(ctx, kp, msgs)
    assert len(E1) == len(E2) == len(c) == 0 and st.tolist() == [0] * 5
    back, st = decrypt_messages(ctx, kp, E1, E2, cf2)
    assert back == [b""] * 5 and st.tolist() == [0] * 5


# ---- pass boundaries --------------------------------------------------------------------------------------------------------------
# about 600 chunks as messages of 7 chunks (200 bytes) under passes of 256 chunk rows.  "straddle": a first message of 3 chunks puts
# messages across chunk 256 (rows 255 .. 261) and chunk 512 (rows 507 .. 513).  "exact": a message of 4 chunks behind 36 of 7 ends
# exactly on row 256, and a message lies across 512 (rows 508 .. 514).
LAYOUTS = {"straddle": [90] + [200] * 85, "exact": [200] * 36 + [120] + [200] * 49}
_layout_cache = {}


def layout(octx, name):
    """the messages, keys and yardstick of a layout, computed once"""
    if name not in _layout_cache:
        msgs = cut(b"afx-tests/messages/layout/" + name.encode(), LAYOUTS[name])
        okp, kp = keys_for(octx, b"afx-tests/messages/layout-key/" + name.encode(), len(msgs))
        cf = ref.chunk_first(msgs)
        E1, E2, ctr, st = ref.encrypt_messages(okp, msgs)
        assert st == [0] * len(msgs) and 590 <= cf[-1] <= 610
        _layout_cache[name] = dict(msgs=msgs, okp=okp, kp=kp, cf=cf, E1=E1, E2=E2, ctr=ctr)
    return _layout_cache[name]


def message_of(cf, row):
    return max(i for i in range(len(cf) - 1) if cf[i] <= row < cf[i + 1])


def test_layouts_are_what_they_say(user):
    s, e = ref.chunk_first(cut(b"x", LAYOUTS["straddle"])), ref.chunk_first(cut(b"x", LAYOUTS["exact"]))
    for cf, b in ((s, 256), (s, 512), (e, 512)):
        i = message_of(cf, b)
        assert cf[i] < b < cf[i + 1]                 # rows on both sides of the boundary
    assert 256 in e and 256 not in s and 512 not in s and 512 not in e


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_pass_boundaries(user, name):
    ctx, octx = user
    L = layout(octx, name)
    msgs, kp, cf = L["msgs"], L["kp"], L["cf"]
    whole_p = from_messages(ctx, msgs)
    whole_e = encrypt_messages(ctx, kp, msgs)
    whole_d = decrypt_messages(ctx, kp, whole_e[0], whole_e[1], whole_e[3])
    ctx.set_chunk_items(256)
    try:
        p = from_messages(ctx, msgs)
        e = encrypt_messages(ctx, kp, msgs)
        d = decrypt_messages(ctx, kp, e[0], e[1], e[3])
    finally:
        ctx.set_chunk_items(0)
    # against the yardstick ...
    check_plaintext_rows(msgs, p)
    check_encrypted(L["okp"], msgs, e)
    assert d[0] == [ref.padded(m) for m in msgs] and not d[1].any()
    # ... and against the default-pass result
    assert all(np.array_equal(x, y) for x, y in zip(p, whole_p)) and all(np.array_equal(x, y) for x, y in zip(e, whole_e))
    assert d[0] == whole_d[0] and np.array_equal(d[1], whole_d[1]) and e[3].tolist() == cf


# ---- keys per message -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secret_mode", [0, 2])
def test_keys_per_message(user, secret_mode):
    ctx, octx = user
    msgs = cut(b"afx-tests/messages/keys/v1", [61, 0, 200, 30, 1, 95, 300, 31, 0, 29])
    okp, kp = keys_for(octx, b"afx-tests/messages/keys/key", len(msgs))
    assert len(set(okp)) == len(okp)
    ctx.set_secret_independent_addressing(secret_mode)
    try:
        enc = encrypt_messages(ctx, kp, msgs)
        check_encrypted(okp, msgs, enc)
        back, st = decrypt_messages(ctx, kp, enc[0], enc[1], enc[3])
        assert back == [ref.padded(m) for m in msgs] and not st.any()
        # a non-canonical a1 on message 2 (7 chunks): that message alone fails, its rows are zeros, its neighbours are the yardstick's
        bad = {f: kp[f].copy() for f in kp}
        bad["a1"][2] = np.frombuffer(L_BYTES, np.uint8)
        expect = [0] * len(msgs)
        expect[2] = ref.ST_VERIFICATION_FAILURE
        check_encrypted(okp, msgs, encrypt_messages(ctx, bad, msgs), expect=expect)
        # ... and a message of no chunks is refused for its key as well
        bad["a1"][1] = np.frombuffer(L_BYTES, np.uint8)
        expect[1] = ref.ST_VERIFICATION_FAILURE
        check_encrypted(okp, msgs, encrypt_messages(ctx, bad, msgs), expect=expect)
    finally:
        ctx.set_secret_independent_addressing(2)


# ---- containment on decrypt -------------------------------------------------------------------------------------------------------
def flip_rows(cf):
    first_of = message_of(cf, 100)
    last_of = message_of(cf, 400)
    return {"first": cf[first_of], "last": cf[last_of + 1] - 1, "before_boundary": 255, "after_boundary": 512}


@pytest.mark.parametrize("case", ["first", "last", "before_boundary", "after_boundary", "all"])
def test_containment_on_decrypt(user, case):
    import oracle
    ctx, octx = user
    L = layout(octx, "straddle")
    msgs, okp, kp, cf = L["msgs"], L["okp"], L["kp"], L["cf"]
    rows = flip_rows(cf)
    assert message_of(cf, 255) == message_of(cf, 256) and message_of(cf, 512) == message_of(cf, 511)      # both lie across their boundary
    hit = sorted(rows.values()) if case == "all" else [rows[case]]
    E1, E2 = arr(L["E1"]), arr(L["E2"])
    for r in hit:
        E2[r, 7] ^= 0x10
        assert oracle.decrypt(okp[message_of(cf, r)], E1[r].tobytes() + E2[r].tobytes())[0] != 0        # the yardstick refuses that chunk
    failed = sorted({message_of(cf, r) for r in hit})
    assert len(failed) == len(hit)
    want, want_st = ref.decrypt_messages(okp, [r.tobytes() for r in E1], [r.tobytes() for r in E2], cf)
    assert [i for i, s in enumerate(want_st) if s] == failed and all(want[i] == bytes(210) for i in failed)
    ctx.set_chunk_items(256)
    try:
        got, st = decrypt_messages(ctx, kp, E1, E2, np.array(cf, np.uint32))
    finally:
        ctx.set_chunk_items(0)
    # exactly those messages, all their bytes zeros (the chunks that by themselves decrypted included; the output held 0xA5)
    assert st.tolist() == want_st and [i for i, s in enumerate(st) if s == ref.ST_UNDECRYPTABLE] == failed
    for i, m in enumerate(msgs):
        assert got[i] == (bytes(30 * (cf[i + 1] - cf[i])) if i in failed else ref.padded(m)), i
    assert got == want
    # the default passes give the same
    got2, st2 = decrypt_messages(ctx, kp, E1, E2, np.array(cf, np.uint32))
    assert got2 == got and np.array_equal(st2, st)


# ---- from points ------------------------------------------------------------------------------------------------------------------
def fixture_messages(n=256):
    return np.frombuffer(hashlib.shake_256(b"afx-tests/plaintext-messages/v1").digest(30 * n), np.uint8).reshape(n, 30)


def test_from_points(user):
    import oracle
    from aeonflux_amd import batch
    ctx, _ = user
    msgs = fixture_messages()
    pts = [oracle.plaintext_from_bytes(m.tobytes())[0][:32] for m in msgs] + [bytes(32), oracle.basepoint()]
    # two encodings that do not decode: candidates below a message's first good counter
    bad = []
    for m in msgs:
        c = oracle.plaintext_from_bytes(m.tobytes())[1]
        if c >= 1 and len(bad) < 2:
            bad.append(ref.candidate(m.tobytes(), c - 1))
    assert len(bad) == 2 and not any(ref.decodes(b) for b in bad)
    pts = pts[:100] + [bad[0]] + pts[100:] + [bad[1]]
    want = [ref.plaintext_from_point(p) for p in pts]
    assert [w is None for w in want] == [i in (100, len(pts) - 1) for i in range(len(pts))]
    P = arr(pts)
    M2, m3, st = batch.plaintexts_from_points(ctx, P)
    o = [Out(len(pts), 32), Out(len(pts), 32), Out(len(pts))]
    batch.plaintexts_from_points_dev(ctx, dev(P), len(pts), *o)
    ctx.synchronize()
    assert all(np.array_equal(x.numpy(), y) for x, y in zip(o, (M2, m3, st)))
    for i, w in enumerate(want):
        if w is None:
            assert st[i] == ref.ST_VERIFICATION_FAILURE and not M2[i].any() and not m3[i].any(), i
        else:
            assert st[i] == 0 and (M2[i].tobytes(), m3[i].tobytes()) == w, i
    # the crate hashes the point's bytes here: not the triple of the message the point encodes
    fb = oracle.plaintext_from_bytes(msgs[0].tobytes())[0]
    assert M2[0].tobytes() != fb[32:64] and m3[0].tobytes() != fb[64:96]


# ---- at a counter -----------------------------------------------------------------------------------------------------------------
def at_counter(ctx, msgs, counters):
    from aeonflux_amd import batch
    counters = np.ascontiguousarray(counters, dtype=np.uint32)
    got = batch.plaintexts_from_bytes_at(ctx, msgs, counters)
    n = len(msgs)
    o = [Out(n, 32), Out(n, 32), Out(n, 32), Out(n)]
    batch.plaintexts_from_bytes_at_dev(ctx, dev(msgs), dev(counters.view(np.uint8)), n, *o)
    ctx.synchronize()
    assert all(np.array_equal(x.numpy(), y) for x, y in zip(o, got))
    return got


def test_at_a_counter(user):
    from aeonflux_amd import batch
    ctx, _ = user
    msgs = fixture_messages()
    M1, M2, m3, c = batch.plaintexts_from_bytes(ctx, msgs)
    # the counter that call returns reproduces it exactly
    g = at_counter(ctx, msgs, c)
    assert np.array_equal(g[0], M1) and np.array_equal(g[1], M2) and np.array_equal(g[2], m3) and not g[3].any()
    # c - 1 does not decode (the search would have stopped there): zero rows
    sel = np.flatnonzero(c >= 1)
    assert len(sel) >= 100
    g = at_counter(ctx, msgs[sel], c[sel] - 1)
    assert (g[3] == ref.ST_VERIFICATION_FAILURE).all() and not g[0].any() and not g[1].any() and not g[2].any()
    # a later counter that decodes gives exactly that candidate, with the same M2 and m3
    later = np.array([next(k for k in range(int(c[i]) + 1, 8192) if ref.decodes(ref.candidate(msgs[i].tobytes(), k))) for i in range(len(msgs))], np.uint32)
    g = at_counter(ctx, msgs, later)
    assert not g[3].any() and np.array_equal(g[1], M2) and np.array_equal(g[2], m3)
    for i in range(len(msgs)):
        assert g[0][i].tobytes() == ref.candidate(msgs[i].tobytes(), int(later[i])) != M1[i].tobytes(), i
    # counters past the last, a counter of the second round of 128 among them: 8192 fails; mixed with good ones item by item
    mix = c.copy()
    mix[::3] = 8192
    mix[1] = 8192 + int(c[1])
    mix[4] = 0xffffffff
    g = at_counter(ctx, msgs, mix)
    failed = mix >= 8192
    assert failed[0] and failed[1] and failed[4] and (g[3][failed] == ref.ST_VERIFICATION_FAILURE).all() and not g[3][~failed].any()
    assert not g[0][failed].any() and not g[1][failed].any() and not g[2][failed].any()
    assert np.array_equal(g[0][~failed], M1[~failed]) and np.array_equal(g[1][~failed], M2[~failed]) and np.array_equal(g[2][~failed], m3[~failed])
    # a candidate of the second round (j = 1) is built as the reference builds it
    i = 5
    k = next(k for k in range(128, 8192) if ref.decodes(ref.candidate(msgs[i].tobytes(), k)))
    g = at_counter(ctx, msgs[i:i + 1], [k])
    assert g[0][0].tobytes() == ref.candidate(msgs[i].tobytes(), k) and g[0][0][31] == 1 and not g[3].any()


# ---- round trip through the protocol ----------------------------------------------------------------------------------------------
def test_round_trip_through_the_existing_decrypt(user):
    from aeonflux_amd import batch
    ctx, octx = user
    msgs = cut(b"afx-tests/messages/round-trip/v1", [61] * 16)
    okp, kp = keys_for(octx, b"afx-tests/messages/round-trip/key", 16)
    E1, E2, ctr, cf, st = encrypt_messages(ctx, kp, msgs)
    assert not st.any() and len(E1) == 48
    E2 = E2.copy()
    E2[3 * 5 + 1, 0] ^= 2                                   # message 5 does not decrypt: its middle chunk
    # the existing call, chunk by chunk, the key replicated in numpy
    rep = np.repeat(np.arange(16), 3)
    _, _, _, rows, cst = batch.decrypt(ctx, {f: kp[f][rep] for f in ("a", "a0", "a1")}, E1, E2)
    want_st = np.where(cst.reshape(16, 3).any(axis=1), ref.ST_UNDECRYPTABLE, 0)
    back, st = decrypt_messages(ctx, kp, E1, E2, cf)
    assert st.tolist() == want_st.tolist() == [ref.ST_UNDECRYPTABLE if i == 5 else 0 for i in range(16)]
    for i in range(16):
        if i == 5:
            assert back[i] == bytes(90) and rows[15].tobytes() == msgs[5][:30]      # (the existing call releases the chunks that decrypted)
        else:
            assert back[i] == rows[3 * i:3 * i + 3].tobytes() == ref.padded(msgs[i]), i
