"""CredentialRequest batches ("AFXR" v1, include/aeonflux_gpu.h), CPU only: the Python and C packers write the same bytes, the
host-side parser round-trips them, the header arithmetic, every malformation the parser must refuse, and a stream of sections."""
import ctypes as C
import struct

import numpy as np
import pytest


def requests(kinds, count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(len(kinds), count, 32), dtype=np.uint8)


def c_pack(kinds, values):
    import aeonflux_amd as afx
    req = afx.AttributesSoA()
    req.n_attributes = len(kinds)
    for i, k in enumerate(kinds):
        req.kinds[i] = k
    values = np.ascontiguousarray(values)
    req.values = values.ctypes.data
    count = values.shape[1]
    n = C.c_size_t(0)
    afx.check(afx.lib().afx_request_wire_pack(C.byref(req), count, None, 0, C.byref(n)))
    buf = np.zeros(n.value, np.uint8)
    afx.check(afx.lib().afx_request_wire_pack(C.byref(req), count, buf.ctypes.data, buf.size, C.byref(n)))
    return buf.tobytes()


def c_parse(blob):
    import aeonflux_amd as afx
    n, cnt, off = C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
    kinds = (C.c_uint8 * afx.MAX_ATTRIBUTES)()
    rc = afx.lib().afx_request_wire_parse(blob, len(blob), C.byref(n), kinds, C.byref(cnt), C.byref(off))
    return rc, n.value, list(kinds[:n.value]), cnt.value, off.value


@pytest.mark.parametrize("kinds,count", [((1, 0, 2, 3), 5), ((1,) * 8 + (2,) * 4 + (4,) * 4, 3), ((2,), 1), ((0, 1, 4), 0), ((), 4)])
def test_python_and_c_packers_agree_and_round_trip(kinds, count):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    vals = requests(kinds, count, 7 + count)
    blob = wire.pack_requests(kinds, vals)
    assert blob == c_pack(kinds, vals)
    hdr = afx.lib().afx_request_wire_header_bytes(len(kinds))
    assert len(blob) == hdr + count * len(kinds) * 32
    assert blob[:20] == b"AFXR" + struct.pack("<4I", 1, count, len(kinds), len(kinds))
    rc, n, k2, cnt, off = c_parse(blob)
    assert (rc, n, k2, cnt, off) == (afx.OK, len(kinds), list(kinds), count, hdr)
    k3, v3 = wire.unpack_requests(blob)
    assert k3 == list(kinds) and np.array_equal(v3, vals)


def test_header_bytes():
    import aeonflux_amd as afx
    hb = afx.lib().afx_request_wire_header_bytes
    assert [hb(n) for n in (0, 12, 13, 32, 33)] == [32, 32, 64, 64, 0]


def test_malformed_sections_are_refused():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    kinds = (1, 0, 2, 3)
    good = wire.pack_requests(kinds, requests(kinds, 3, 1))
    assert c_parse(good)[0] == afx.OK

    def word(b, at, v):
        return b[:at] + struct.pack("<I", v) + b[at + 4:]
    bad = {
        "truncated": good[:-1],
        "one extra byte": good + b"\0",
        "wrong magic": b"AFXI" + good[4:],
        "version 2": word(good, 4, 2),
        "wrong cells_per_record": word(good, 12, 5),
        "n = 33": word(word(good, 16, 33), 12, 33),
        "count 2^30": word(good, 8, 1 << 30),
        "kind 5": good[:22] + b"\x05" + good[23:],
        "short header": good[:19],
    }
    for why, b in bad.items():
        assert c_parse(b)[0] == afx.E_BAD_ARGS, why
        sl = C.c_size_t(0)
        if why in ("truncated", "wrong magic", "version 2", "wrong cells_per_record", "n = 33", "count 2^30", "short header"):
            assert afx.lib().afx_request_wire_section_bytes(b, len(b), C.byref(sl)) == afx.E_BAD_ARGS, why
    # n = 0 is a well-formed header whatever its count: no records, and nothing divides by cells_per_record
    empty = wire.pack_requests((), np.zeros((0, 7, 32), np.uint8))
    assert len(empty) == 32 and c_parse(empty)[:4] == (afx.OK, 0, [], 7)
    assert c_parse(empty + bytes(32))[0] == afx.E_BAD_ARGS


def test_section_bytes_walks_a_stream():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    parts = [wire.pack_requests((1, 0, 2, 3), requests((1, 0, 2, 3), 3, 2)), wire.pack_requests((), np.zeros((0, 2, 32), np.uint8)),
             wire.pack_requests((4,) * 13, requests((4,) * 13, 2, 3))]
    stream = b"".join(parts)
    off, seen = 0, []
    while off < len(stream):
        sl = C.c_size_t(0)
        afx.check(afx.lib().afx_request_wire_section_bytes(stream[off:], len(stream) - off, C.byref(sl)))
        seen.append(sl.value)
        off += sl.value
    assert seen == [len(p) for p in parts]
    sl = C.c_size_t(0)
    assert afx.lib().afx_request_wire_section_bytes(stream[:len(parts[0]) - 1], len(parts[0]) - 1, C.byref(sl)) == afx.E_BAD_ARGS

