"""One honest record of a packed section (include/aeonflux_gpu.h: AFXP, AFXB, AFXR, AFXI, AFXQ, AFXJ) damaged once per (cell, damage):
the input of tests/test_cell_sweep_ref.py (what the yardsticks say of every damaged record) and tests/test_gpu_cell_sweep.py (what the
engine's doors say).  Header length and cells per record come from the library's own format functions, so the sweep covers whatever
cells the format holds.  The damages do not look at what a cell holds; with v the cell as a little-endian integer:

  +l      v + l            the same scalar, not canonical: only a canonicity check on that row refuses it
  bit255  v xor 2^255      the same field element to a decoder that drops bit 255
  neg     p - v            the same point to a decoder without the sign test on s (v = 0 gives p, an alias of the identity)
  other   the same cell of another honest record: a cell bound to nothing, or two cells mapped to one row
  zero    32 zero bytes
  bit     one flipped bit below bit 255, its position chosen from (cell, record)

No fixtures and no hooks: a plain module."""
import ctypes as C
import struct

import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
P = 2 ** 255 - 19
DAMAGES = ("+l", "bit255", "neg", "other", "zero", "bit")
CONTROL_EVERY = 16          # an untouched control follows every 16 damaged records (and the last, shorter run)


def _layout_parse(name, with_nr):
    """the reader of a format whose layout is n_attributes, the kinds and (with_nr) n_responses: blob -> (header bytes, cells, count)"""
    def read(lib, blob):
        import aeonflux_amd as afx
        n, nr, count, off = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
        kinds = (C.c_uint8 * 32)()
        args = [blob, len(blob), C.byref(n), kinds] + ([C.byref(nr)] if with_nr else []) + [C.byref(count), C.byref(off)]
        afx.check(getattr(lib, "afx_%s_wire_parse" % name)(*args))
        hdr = getattr(lib, "afx_%s_wire_header_bytes" % name)(n.value)
        assert hdr == off.value and count.value
        # these formats have no cells_per_record function: the parser has checked the header's word against the layout and the
        # record area against count * cells * 32
        cells, rest = divmod(len(blob) - hdr, 32 * count.value)
        assert rest == 0 and cells == struct.unpack("<I", blob[12:16])[0]
        return hdr, cells, count.value
    return read


def _afxp(lib, blob):
    import aeonflux_amd as afx
    shape, count, off = afx.Shape(), C.c_size_t(0), C.c_size_t(0)
    afx.check(lib.afx_wire_parse(blob, len(blob), C.byref(shape), C.byref(count), C.byref(off)))
    hdr = lib.afx_wire_header_bytes(C.byref(shape))
    assert hdr == off.value
    return hdr, lib.afx_wire_cells_per_record(C.byref(shape)), count.value


def _afxb(lib, blob):
    import aeonflux_amd as afx
    shape, n_main, count, off = afx.Shape(), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
    afx.check(lib.afx_batchable_wire_parse(blob, len(blob), C.byref(shape), C.byref(n_main), C.byref(count), C.byref(off)))
    hdr = lib.afx_batchable_wire_header_bytes(C.byref(shape))
    assert hdr == off.value
    return hdr, lib.afx_batchable_wire_cells_per_record(C.byref(shape), n_main.value), count.value


FORMATS = {b"AFXP": _afxp, b"AFXB": _afxb, b"AFXR": _layout_parse("request", False), b"AFXI": _layout_parse("issuance", True),
           b"AFXQ": _layout_parse("blind_request", True), b"AFXJ": _layout_parse("blind_issuance", True)}


def layout(blob):
    """(header bytes, cells per record, count) of the one section `blob` holds, as the library's format functions give them"""
    import aeonflux_amd as afx
    hdr, cells, count = FORMATS[bytes(blob[:4])](afx.lib(), bytes(blob))
    assert hdr and cells and len(blob) == hdr + count * cells * 32
    return hdr, cells, count


def bit_position(cell, record):
    return (131 * cell + 29 * record + 7) % 255


def damaged_cell(damage, v, other, cell, record):
    """the new 32 bytes of a cell whose honest bytes are v; other: the same cell of another honest record"""
    x = int.from_bytes(v, "little")
    assert x < 2 ** 255, "an honest cell has bit 255 clear"
    if damage == "+l":
        y = x + L
    elif damage == "bit255":
        y = x ^ (1 << 255)
    elif damage == "neg":
        y = P - x
    elif damage == "other":
        y = int.from_bytes(other, "little")
    elif damage == "zero":
        y = 0
    elif damage == "bit":
        y = x ^ (1 << bit_position(cell, record))
    else:
        raise ValueError(damage)
    assert 0 <= y < 2 ** 256
    new = y.to_bytes(32, "little")
    assert new != bytes(v), ("the damage changes nothing", cell, damage)
    return new


class Sweep:
    """records [count, cells, 32]: the swept records; entries[k]: (cell, damage) of record k, None for a control; blob: the swept
    section (None for records that have no wire format); record: the honest record's index in the section it came from"""

    def __init__(self, records, entries, record, blob=None, hdr=0):
        self.records, self.entries, self.record, self.blob, self.hdr = records, entries, record, blob, hdr
        self.count, self.cells = records.shape[0], records.shape[1]
        self.honest = records[-1]          # (the last record is a control)
        self.controls = [k for k, e in enumerate(entries) if e is None]
        self.damaged = [k for k, e in enumerate(entries) if e is not None]

    def of(self, damage):
        """{cell: record index} of one damage"""
        return {e[0]: k for k, e in enumerate(self.entries) if e is not None and e[1] == damage}


def sweep_records(rec, record, other=None):
    """rec [count, cells, 32] honest records -> the Sweep of record `record`: damaged once per (cell, damage), cell-major, a control
    after every CONTROL_EVERY damaged records and at the end.  other: the record `other` takes its cells from (default: the next)."""
    count, cells = rec.shape[0], rec.shape[1]
    assert count >= 2 and 0 <= record < count and rec.shape[2] == 32 and rec.dtype == np.uint8
    other = (record + 1) % count if other is None else other
    assert other != record and 0 <= other < count
    honest = rec[record].copy()
    out, entries, done = [], [], 0
    for cell in range(cells):
        for damage in DAMAGES:
            r = honest.copy()
            r[cell] = np.frombuffer(damaged_cell(damage, honest[cell].tobytes(), rec[other, cell].tobytes(), cell, record), np.uint8)
            out.append(r)
            entries.append((cell, damage))
            done += 1
            if done % CONTROL_EVERY == 0:
                out.append(honest.copy())
                entries.append(None)
    if entries[-1] is not None:
        out.append(honest.copy())
        entries.append(None)
    # none skipped, none twice
    assert done == cells * len(DAMAGES) and set(e for e in entries if e) == {(c, d) for c in range(cells) for d in DAMAGES}
    return Sweep(np.stack(out), entries, record)


def sweep(blob, record, other=None):
    """the section `blob` with its records replaced by the sweep of its record `record` (sweep_records)"""
    hdr, cells, count = layout(blob)
    s = sweep_records(np.frombuffer(blob, np.uint8, offset=hdr).reshape(count, cells, 32), record, other)
    assert s.count - len(s.controls) == cells * len(DAMAGES)
    header = bytearray(blob[:hdr])
    header[8:12] = struct.pack("<I", s.count)          # every format: magic | version | count | cells_per_record | ...
    s.blob, s.hdr = bytes(header) + s.records.tobytes(), hdr
    assert layout(s.blob) == (hdr, cells, s.count)
    return s


def describe(door, fields, entry):
    """what a mismatch report says of one record: the door, the cell index, the field that cell belongs to and the damage"""
    if entry is None:
        return "%s: an untouched control" % door
    cell, damage = entry
    return "%s: cell %d (%s), damage %s" % (door, cell, fields[cell], damage)


# ---- which field a cell belongs to, per format (the record layouts of include/aeonflux_gpu.h, in words) ----
ENC_FIELDS = ["challenge"] + ["responses[%d]" % k for k in range(6)] + ["pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p"]
# 's': a scalar the statement reads; 'p': a point; the order of ENC_FIELDS
ENC_TYPES = "s" * 7 + "p" * 7


def presentation_fields(shape):
    """[(name, 's' | 'p')] per cell of an AFXP record of `shape`"""
    n, nr = shape.n_attributes, shape.n_responses
    f = [("challenge", "s")] + [("responses[%d]" % k, "s") for k in range(nr)] + [("C_x_0", "p"), ("C_x_1", "p"), ("C_V", "p")]
    f += [("C_y[%d]" % i, "p") for i in range(n)]
    f += [("attr_values[%d]" % i, "s" if shape.kinds[i] == 0 else "p") for i in range(n) if shape.kinds[i] in (0, 2)]
    for e in range(shape.n_enc_proofs):
        f += [("enc[%d].%s" % (e, name), t) for name, t in zip(ENC_FIELDS, ENC_TYPES)]
    return f


def batchable_fields(shape, n_main):
    n, nr = shape.n_attributes, shape.n_responses
    f = [("commitments.main[%d]" % j, "p") for j in range(n_main)] + [("responses[%d]" % k, "s") for k in range(nr)]
    f += [("C_x_0", "p"), ("C_x_1", "p"), ("C_V", "p")] + [("C_y[%d]" % i, "p") for i in range(n)]
    f += [("attr_values[%d]" % i, "s" if shape.kinds[i] == 0 else "p") for i in range(n) if shape.kinds[i] in (0, 2)]
    for e in range(shape.n_enc_proofs):
        f += [("commitments.enc[%d][%d]" % (e, j), "p") for j in range(5)]
        f += [("enc[%d].%s" % (e, name), t) for name, t in list(zip(ENC_FIELDS, ENC_TYPES))[1:]]
    return f


def _value_type(kind):
    return "s" if kind in (0, 1) else "p"


def request_fields(kinds):
    return [("values[%d]" % i, _value_type(k)) for i, k in enumerate(kinds)]


def issuance_fields(kinds, nr):
    f = [("t", "s"), ("U", "p"), ("V", "p"), ("challenge", "s")] + [("responses[%d]" % k, "s") for k in range(nr)]
    return f + request_fields(kinds)


def blind_request_fields(kinds):
    h = sum(1 for k in kinds if k in (1, 4))
    hs = sum(1 for k in kinds if k == 1)
    f = [("D", "p")] + [("A[%d]" % j, "p") for j in range(h)] + [("B[%d]" % j, "p") for j in range(h)] + [("challenge", "s")]
    f += [("responses[%d]" % k, "s") for k in range(1 + h + hs)]
    return f + [("values[%d]" % i, _value_type(k)) for i, k in enumerate(kinds) if k not in (1, 4)]


def blind_issuance_fields(nr):
    return [("t", "s"), ("U", "p"), ("S1", "p"), ("S2", "p"), ("challenge", "s")] + [("responses[%d]" % k, "s") for k in range(nr)]
