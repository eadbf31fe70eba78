"""The header cases of the six wire formats (AFXP, AFXB, AFXR, AFXI, AFXQ, AFXJ), enumerated: what tests/gen_wire_headers.py records at
one commit and tests/test_wire_headers.py replays at every later one.  Deterministic - no randomness, no clock - so that the recorder
and the test walk the same cases in the same order and the fixture (tests/golden/wire_headers.json) holds outcomes only, not blobs.

Valid sections come from the Python packers' headers (aeonflux_amd/wire.py) at 0, 1, 4 and AFX_MAX_ATTRIBUTES attributes with 0, 1 and
3 records of zeros; every one is then damaged the way the byte fuzzers damage them, but exhaustively: every u32 header word set to
0, 1, its value - 1 and + 1, AFX_MAX_ATTRIBUTES, that + 1, 0x7fffffff and 0xffffffff; every kinds byte to 4 and to 255; every padding
byte to 1; every length from 0 to the header's + 33; one trailing byte; count + 1 with no record more; every other format's magic.
A case's outcome is what *_wire_parse and *_wire_section_bytes answer: return code, every out-parameter (pre-filled, so that "left
untouched" shows) and, after a failure, afx_last_error()."""
import ctypes as C
import hashlib
import struct

import aeonflux_amd as afx
from aeonflux_amd import batch, wire

MAX = afx.MAX_ATTRIBUTES
WORD_VALUES = lambda v: (0, 1, (v - 1) & 0xffffffff, (v + 1) & 0xffffffff, MAX, MAX + 1, 0x7fffffff, 0xffffffff)
COUNTS = (0, 1, 3)
# credential kinds (AFX_ATTR_*) of the layouts; 1 is a hidden scalar, 4 a hidden point
LAYOUTS = ([], [0], [0, 1, 2, 4], [(0, 1, 2, 4)[i % 4] for i in range(MAX)])
SENTINEL = 0xAA


def n_main_of(shape, strict=False):
    """afx_batchable_n_main_of (aeonflux_amd/csrc/statements.hpp)"""
    n = shape.n_attributes
    k = sum(1 for i in range(n) if shape.kinds[i] != 3)
    if strict:
        return 2 + k + sum(1 for e in range(shape.n_enc_proofs) if shape.enc_indices[e] != 0)
    return 2 + sum(1 for j in range(k) if shape.kinds[j] != 3)


def _hidden(kinds):
    return sum(1 for k in kinds if k in (1, 4)), sum(1 for k in kinds if k == 1)


class Format:
    def __init__(self, name, fixed, lists, parse, section, header):
        self.name, self.fixed, self.lists, self.parse_fn, self.section_fn, self.header = name, fixed, lists, parse, section, header

    def valid(self, kinds, count):
        """(blob, header bytes, n, bytes of index lists) of a valid section of `count` zero records"""
        h, cells, lists = self.header(kinds, count)
        return h + bytes(count * cells * 32), len(h), len(kinds), lists


def _afxp(kinds, count):
    sh = batch.shape_of_kinds(kinds)
    h, cells = wire.header(sh, count)
    return h, cells, 2 * (sh.n_hidden_scalars + sh.n_enc_proofs)


def _afxb(kinds, count):
    sh = batch.shape_of_kinds(kinds)
    h, cells = wire.batchable_header(sh, n_main_of(sh), count)
    return h, cells, 2 * (sh.n_hidden_scalars + sh.n_enc_proofs)


def _afxr(kinds, count):
    n = len(kinds)
    h = b"AFXR" + struct.pack("<4I", 1, count, n, n) + bytes(kinds)   # (wire.pack_requests' header)
    return h + bytes(-len(h) % 32), n, 0


def _afxi(kinds, count):
    n, nr = len(kinds), len(kinds) + 5
    h = b"AFXI" + struct.pack("<5I", 1, count, 4 + nr + n, n, nr) + bytes(kinds)   # (wire.pack_issuances' header)
    return h + bytes(-len(h) % 32), 4 + nr + n, 0


def _afxq(kinds, count):
    h, hs = _hidden(kinds)
    cells = 3 + 2 * h + hs + len(kinds)
    return wire._blind_header(b"AFXQ", kinds, count, cells, 1 + h + hs), cells, 0


def _afxj(kinds, count):
    nr = len(kinds) + 6
    return wire._blind_header(b"AFXJ", kinds, count, 5 + nr, nr), 5 + nr, 0


FORMATS = (
    Format("AFXP", 32, True, "afx_wire_parse", "afx_wire_section_bytes", _afxp),
    Format("AFXB", 36, True, "afx_batchable_wire_parse", "afx_batchable_wire_section_bytes", _afxb),
    Format("AFXR", 20, False, "afx_request_wire_parse", "afx_request_wire_section_bytes", _afxr),
    Format("AFXI", 24, False, "afx_issuance_wire_parse", "afx_issuance_wire_section_bytes", _afxi),
    Format("AFXQ", 24, False, "afx_blind_request_wire_parse", "afx_blind_request_wire_section_bytes", _afxq),
    Format("AFXJ", 24, False, "afx_blind_issuance_wire_parse", "afx_blind_issuance_wire_section_bytes", _afxj),
)


def cases():
    """yields (format, description, blob)"""
    for f in FORMATS:
        for kinds in LAYOUTS:
            for count in COUNTS:
                blob, hdr, n, lists = f.valid(kinds, count)
                tag = "%s n=%d count=%d: " % (f.name, n, count)
                yield f, tag + "valid", blob
                for off in range(4, f.fixed, 4):
                    v = struct.unpack_from("<I", blob, off)[0]
                    for w in WORD_VALUES(v):
                        yield f, tag + "word at %d = %#x" % (off, w), blob[:off] + struct.pack("<I", w) + blob[off + 4:]
                for i in range(n):
                    for k in (4, 255):
                        yield f, tag + "kind %d = %d" % (i, k), blob[:f.fixed + i] + bytes([k]) + blob[f.fixed + i + 1:]
                for p in range(f.fixed + n + lists, hdr):
                    yield f, tag + "padding byte %d = 1" % p, blob[:p] + b"\x01" + blob[p + 1:]
                for length in range(0, min(len(blob), hdr + 33) + 1):
                    yield f, tag + "truncated to %d" % length, blob[:length]
                yield f, tag + "one trailing byte", blob + b"\x00"
                yield f, tag + "count + 1, no record more", blob[:8] + struct.pack("<I", count + 1) + blob[12:]
                for g in FORMATS:
                    if g is not f:
                        yield f, tag + "magic " + g.name, g.name.encode() + blob[4:]


def _filled(ctype):
    v = ctype()
    C.memset(C.byref(v), SENTINEL, C.sizeof(v))
    return v


def outcome(lib, f, blob):
    """(parse outcome, section_bytes outcome): each [rc, error text or None, out-parameters...]"""
    shape, n_main, n, nr = _filled(afx.Shape), _filled(C.c_uint32), _filled(C.c_uint32), _filled(C.c_uint32)
    kinds, count, off, sl = _filled(C.c_uint8 * MAX), _filled(C.c_size_t), _filled(C.c_size_t), _filled(C.c_size_t)
    if f.name == "AFXP":
        outs = (shape, count, off)
    elif f.name == "AFXB":
        outs = (shape, n_main, count, off)
    elif f.name == "AFXR":
        outs = (n, kinds, count, off)
    else:
        outs = (n, kinds, nr, count, off)
    rc = getattr(lib, f.parse_fn)(blob, C.c_size_t(len(blob)), *[C.byref(o) for o in outs])
    parse = [rc, lib.afx_last_error().decode() if rc else None] + [bytes(o).hex() if isinstance(o, (afx.Shape, C.Array)) else o.value for o in outs]
    rc = getattr(lib, f.section_fn)(blob, C.c_size_t(len(blob)), C.byref(sl))
    return parse, [rc, lib.afx_last_error().decode() if rc else None, sl.value]


def sweep_shapes(n):
    """the shapes of the layout sweep at n attributes: every kind alone, the kinds mixed, and counts no header carries"""
    out = []
    for kinds in ([0] * n, [1] * n, [2] * n, [4] * n, [(0, 1, 2, 4)[i % 4] for i in range(n)]):
        sh = batch.shape_of_kinds(kinds[:MAX])
        sh.n_attributes = n   # (MAX + 1: what the functions refuse)
        out.append(sh)
    for field, value in (("n_responses", 3 + MAX + 1), ("n_hidden_scalars", MAX + 1), ("n_enc_proofs", MAX + 1)):
        sh = batch.shape_of_kinds([0] * min(n, MAX))
        setattr(sh, field, value)
        out.append(sh)
    if 0 < n <= MAX:
        sh = batch.shape_of_kinds([0] * n)
        sh.kinds[n - 1] = 4   # above AFX_ENC_SECRET_POINT
        out.append(sh)
    return out


def sweep(lib):
    """*_wire_header_bytes and *_wire_cells_per_record for every n in 0 .. AFX_MAX_ATTRIBUTES + 1"""
    for name in ("afx_wire_header_bytes", "afx_batchable_wire_header_bytes", "afx_request_wire_header_bytes", "afx_issuance_wire_header_bytes",
                 "afx_blind_request_wire_header_bytes", "afx_blind_issuance_wire_header_bytes"):
        getattr(lib, name).restype = C.c_size_t
    lib.afx_wire_cells_per_record.restype = C.c_uint32
    lib.afx_batchable_wire_cells_per_record.restype = C.c_uint32
    rows = []
    for n in range(MAX + 2):
        row = [getattr(lib, "afx_%s_wire_header_bytes" % k)(C.c_uint32(n)) for k in ("request", "issuance", "blind_request", "blind_issuance")]
        for sh in sweep_shapes(n):
            row += [lib.afx_wire_header_bytes(C.byref(sh)), lib.afx_wire_cells_per_record(C.byref(sh)), lib.afx_batchable_wire_header_bytes(C.byref(sh))]
            ok = n <= MAX and sh.n_hidden_scalars <= MAX and sh.n_enc_proofs <= MAX
            mains = (n_main_of(sh), n_main_of(sh, True), 0, 1) if ok else (2, 0)
            row += [lib.afx_batchable_wire_cells_per_record(C.byref(sh), C.c_uint32(m)) for m in mains]
        rows.append(row)
    return rows


def digest():
    """of every case's format, description and blob: the fixture names the cases it was recorded for"""
    h = hashlib.sha256()
    for f, what, blob in cases():
        h.update(("%s|%s|%d|" % (f.name, what, len(blob))).encode() + hashlib.sha256(blob).digest())
    return h.hexdigest()
