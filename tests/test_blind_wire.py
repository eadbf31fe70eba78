"""Blind requests ("AFXQ" v1) and blind issuances ("AFXJ" v1, include/aeonflux_gpu.h "Blind issuance on bytes"), CPU only: the Python
and C packers write the same bytes, the host-side parsers round-trip them, the header arithmetic, every malformation the parsers must
refuse, and a stream of sections of both formats."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.test_blind_ref import LAYOUTS

WIDE = (1, 0, 4, 2, 3, 1, 4, 0) * 4          # 32 attributes, 16 of them hidden
CASES = [(tuple(kinds), 3) for _, kinds in LAYOUTS] + [((), 4), ((0, 2), 0), (WIDE, 2)]


def layout(kinds):
    return sum(1 for k in kinds if k in (1, 4)), sum(1 for k in kinds if k == 1)


def random_request(kinds, count, seed):
    rng = np.random.default_rng(seed)
    rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    h, hs = layout(kinds)
    return rb(len(kinds), count, 32), dict(D=rb(count, 32), A=rb(h, count, 32), B=rb(h, count, 32), challenge=rb(count, 32), responses=rb(1 + h + hs, count, 32))


def random_issuance(nr, count, seed):
    rng = np.random.default_rng(seed)
    rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    return dict(t=rb(count, 32), U=rb(count, 32), S1=rb(count, 32), S2=rb(count, 32), challenge=rb(count, 32), responses=rb(nr, count, 32))


def attrs_of(kinds, values):
    import aeonflux_amd as afx
    a = afx.AttributesSoA()
    a.n_attributes = len(kinds)
    for i, k in enumerate(kinds):
        a.kinds[i] = k
    a.values = values.ctypes.data if values is not None and values.size else None
    return a


def ptr(a):
    return a.ctypes.data if a.size else None


def c_pack_requests(kinds, values, req):
    import aeonflux_amd as afx
    values = np.ascontiguousarray(values)
    a = attrs_of(kinds, values)
    q = afx.BlindRequestSoA(*(ptr(req[f]) for f in ("D", "A", "B", "challenge", "responses")))
    count = req["D"].shape[0]
    n = C.c_size_t(0)
    afx.check(afx.lib().afx_blind_request_wire_pack(C.byref(a), C.byref(q), count, None, 0, C.byref(n)))
    buf = np.zeros(max(1, n.value), np.uint8)
    afx.check(afx.lib().afx_blind_request_wire_pack(C.byref(a), C.byref(q), count, buf.ctypes.data, n.value, C.byref(n)))
    return buf[:n.value].tobytes()


def c_pack_issuances(kinds, iss):
    import aeonflux_amd as afx
    a = attrs_of(kinds, None)
    s = afx.BlindIssuanceSoA(*(ptr(iss[f]) for f in ("t", "U", "S1", "S2", "challenge", "responses")))
    count, nr = iss["t"].shape[0], iss["responses"].shape[0]
    n = C.c_size_t(0)
    afx.check(afx.lib().afx_blind_issuance_wire_pack(C.byref(a), C.byref(s), nr, count, None, 0, C.byref(n)))
    buf = np.zeros(max(1, n.value), np.uint8)
    afx.check(afx.lib().afx_blind_issuance_wire_pack(C.byref(a), C.byref(s), nr, count, buf.ctypes.data, n.value, C.byref(n)))
    return buf[:n.value].tobytes()


def c_parse(fmt, blob):
    import aeonflux_amd as afx
    n, nr, cnt, off = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
    kinds = (C.c_uint8 * afx.MAX_ATTRIBUTES)()
    rc = getattr(afx.lib(), "afx_blind_%s_wire_parse" % fmt)(blob, len(blob), C.byref(n), kinds, C.byref(nr), C.byref(cnt), C.byref(off))
    return rc, n.value, list(kinds[:n.value]), nr.value, cnt.value, off.value


def c_section(fmt, blob):
    import aeonflux_amd as afx
    sl = C.c_size_t(0)
    return getattr(afx.lib(), "afx_blind_%s_wire_section_bytes" % fmt)(blob, len(blob), C.byref(sl)), sl.value


@pytest.mark.parametrize("kinds,count", CASES)
def test_request_packers_agree_and_round_trip(kinds, count):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    n = len(kinds)
    h, hs = layout(kinds)
    values, req = random_request(kinds, count, 11 + count)
    blob = wire.pack_blind_requests(kinds, values, req)
    assert blob == c_pack_requests(kinds, values, req)
    hdr, cells = afx.lib().afx_blind_request_wire_header_bytes(n), 3 + 2 * h + hs + n
    assert len(blob) == hdr + count * cells * 32
    assert blob[:24] == b"AFXQ" + struct.pack("<5I", 1, count, cells, n, 1 + h + hs)
    assert blob[24:24 + n] == bytes(kinds) and not any(blob[24 + n:hdr])
    assert c_parse("request", blob) == (afx.OK, n, list(kinds), 1 + h + hs, count, hdr)
    k2, v2, q2 = wire.unpack_blind_requests(blob)
    assert k2 == list(kinds) and all(np.array_equal(q2[f], req[f]) for f in req)
    for i, k in enumerate(kinds):          # a hidden position has no value cell: its row comes back as zeros
        assert np.array_equal(v2[i], values[i]) if k not in (1, 4) else not v2[i].any()
    # the value rows of hidden positions are not read: other bytes there give the same section
    other = values.copy()
    for i, k in enumerate(kinds):
        if k in (1, 4):
            other[i] ^= 0x5A
    assert c_pack_requests(kinds, other, req) == blob and wire.pack_blind_requests(kinds, other, req) == blob


@pytest.mark.parametrize("kinds,count", CASES)
def test_issuance_packers_agree_and_round_trip(kinds, count):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    n, nr = len(kinds), len(kinds) + 6
    iss = random_issuance(nr, count, 23 + count)
    blob = wire.pack_blind_issuances(kinds, iss)
    assert blob == c_pack_issuances(kinds, iss)
    hdr = afx.lib().afx_blind_issuance_wire_header_bytes(n)
    assert len(blob) == hdr + count * (5 + nr) * 32
    assert blob[:24] == b"AFXJ" + struct.pack("<5I", 1, count, 5 + nr, n, nr) and blob[24:24 + n] == bytes(kinds)
    assert c_parse("issuance", blob) == (afx.OK, n, list(kinds), nr, count, hdr)
    k2, s2 = wire.unpack_blind_issuances(blob)
    assert k2 == list(kinds) and all(np.array_equal(s2[f], iss[f]) for f in iss)


def test_an_issuance_section_of_another_context_still_parses():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    blob = wire.pack_blind_issuances((0, 2), random_issuance(10, 3, 5))          # a context of n = 4 answered a request of n = 2
    assert c_parse("issuance", blob) == (afx.OK, 2, [0, 2], 10, 3, 32)


def test_header_bytes():
    import aeonflux_amd as afx
    for fmt in ("request", "issuance"):
        hb = getattr(afx.lib(), "afx_blind_%s_wire_header_bytes" % fmt)
        assert [hb(n) for n in (0, 8, 9, 32, 33)] == [32, 32, 64, 64, 0], fmt


def word(b, at, v):
    return b[:at] + struct.pack("<I", v) + b[at + 4:]


def test_malformed_request_sections_are_refused():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    kinds = (4, 2, 3, 1)          # h = 2, hs = 1: 4 responses, 12 cells
    good = wire.pack_blind_requests(kinds, *random_request(kinds, 3, 1))
    assert c_parse("request", good)[0] == afx.OK and c_section("request", good) == (afx.OK, len(good))
    bad = {
        "wrong magic": b"AFXJ" + good[4:],
        "version 2": word(good, 4, 2),
        "n = 33": word(good, 16, 33),
        "kind 5": good[:25] + b"\x05" + good[26:],
        "n_responses 5": word(good, 20, 5),
        "a hidden kind made public": good[:24] + b"\x02" + good[25:],          # the response count no longer fits the kinds
        "wrong cells_per_record": word(good, 12, 13),
        "short header": good[:23],
        "padding not zero": good[:31] + b"\x01" + good[32:],
        "truncated header": wire.pack_blind_requests(WIDE, *random_request(WIDE, 0, 2))[:32],          # n = 32 needs 64 bytes
        "truncated": good[:-1],
        "one extra byte": good + b"\0",
        "count 2^30": word(good, 8, 1 << 30),
    }
    for why, b in bad.items():
        assert c_parse("request", b)[0] == afx.E_BAD_ARGS, why
        if why != "one extra byte":          # (the walker reads a section off the front of a longer stream)
            assert c_section("request", b)[0] == afx.E_BAD_ARGS, why
    # n = 0 is well formed whatever its count: D, challenge and one response per record
    empty = wire.pack_blind_requests((), *random_request((), 7, 3))
    assert len(empty) == 32 + 7 * 96 and c_parse("request", empty)[:5] == (afx.OK, 0, [], 1, 7)
    assert empty[12:16] == struct.pack("<I", 3)
    assert c_parse("request", empty + bytes(32))[0] == afx.E_BAD_ARGS


def test_malformed_issuance_sections_are_refused():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    kinds = (4, 2, 3, 1)
    good = wire.pack_blind_issuances(kinds, random_issuance(10, 3, 4))
    assert c_parse("issuance", good)[0] == afx.OK and c_section("issuance", good) == (afx.OK, len(good))
    bad = {
        "wrong magic": b"AFXQ" + good[4:],
        "version 2": word(good, 4, 2),
        "n = 33": word(good, 16, 33),
        "kind 5": good[:25] + b"\x05" + good[26:],
        "n_responses 39": word(word(good, 20, 39), 12, 44),          # above AFX_MAX_ATTRIBUTES + 6, with the cell count that goes with it
        "wrong cells_per_record": word(good, 12, 16),
        "short header": good[:23],
        "padding not zero": good[:28] + b"\x80" + good[29:],
        "truncated header": wire.pack_blind_issuances(WIDE, random_issuance(38, 0, 2))[:32],
        "truncated": good[:-1],
        "one extra byte": good + b"\0",
        "count 2^30": word(good, 8, 1 << 30),
    }
    for why, b in bad.items():
        assert c_parse("issuance", b)[0] == afx.E_BAD_ARGS, why
        if why != "one extra byte":
            assert c_section("issuance", b)[0] == afx.E_BAD_ARGS, why
    most = wire.pack_blind_issuances(WIDE, random_issuance(38, 1, 6))          # n_responses = AFX_MAX_ATTRIBUTES + 6 is the last accepted
    assert c_parse("issuance", most)[:4] == (afx.OK, 32, list(WIDE), 38)


def test_section_bytes_walks_a_stream_of_both_formats():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    parts = [("request", wire.pack_blind_requests((4, 2, 3, 1), *random_request((4, 2, 3, 1), 3, 2))),
             ("issuance", wire.pack_blind_issuances((4, 2, 3, 1), random_issuance(10, 3, 3))),
             ("request", wire.pack_blind_requests((), *random_request((), 2, 4))),
             ("issuance", wire.pack_blind_issuances((), random_issuance(9, 0, 5))),
             ("request", wire.pack_blind_requests(WIDE, *random_request(WIDE, 2, 6)))]
    stream = b"".join(p for _, p in parts)
    off = 0
    for fmt, p in parts:
        rest = stream[off:]
        assert c_section(fmt, rest) == (afx.OK, len(p)), (fmt, off)
        assert wire.blind_section_bytes(rest) == len(p)
        assert c_section("issuance" if fmt == "request" else "request", rest)[0] == afx.E_BAD_ARGS          # each walker knows its own magic only
        off += len(p)
    assert off == len(stream)
    first = parts[0][1]
    assert c_section("request", first[:-1])[0] == afx.E_BAD_ARGS
