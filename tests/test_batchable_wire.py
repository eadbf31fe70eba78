"""CPU-only: the AFXB wire format (include/aeonflux_gpu.h) through the real library's host-only entry points - header, packer, parser
and section length round trips against the Python mirror (aeonflux_amd/wire.py); malformed headers are AFX_E_BAD_ARGS; and the number
of main-proof commitments the format accepts for the shapes of the golden flows is the number the ORACLE's verifier reports."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import batchable_ref as B
from tests.helpers import pres_from_json
from tests.soa import presentation_arrays, shape_of

H = bytes.fromhex


def _n_main(afx, shape, strict=False):
    """what the library accepts for the shape: the reference's count (the smaller or equal one) or the strict one"""
    ok = [m for m in range(0, 80) if afx.lib().afx_batchable_wire_cells_per_record(C.byref(shape), m)]
    assert 1 <= len(ok) <= 2, ok
    return ok[-1] if strict else ok[0]


def _flow_items(flows):
    import oracle
    import aeonflux_amd as afx
    for f in flows:
        if "presentation" not in f:
            continue
        p = pres_from_json(f)
        yield f, oracle.Ctx(H(f["params"]), H(f["key"]), H(f["issuer_params"])), p, afx.Shape.from_buffer_copy(bytes(shape_of(p)))


def test_n_main_commitments_of_the_golden_flows_is_the_oracles_count(flows):
    import aeonflux_amd as afx
    n = with_commitments = 0
    for f, issuer, p, shape in _flow_items(flows):
        n += 1
        cm = B.to_batchable(issuer, p)
        if cm is None:
            continue
        m = len(cm["main"])
        cells = afx.lib().afx_batchable_wire_cells_per_record(C.byref(shape), m)
        pub = sum(1 for i in range(shape.n_attributes) if shape.kinds[i] in (0, 2))
        assert cells == m + shape.n_responses + 3 + shape.n_attributes + pub + 18 * shape.n_enc_proofs, f["name"]
        assert _n_main(afx, shape) == m, f["name"]                       # the reference's statement: the smaller accepted count
        assert all(len(c) == 5 for c in cm["enc"])
        with_commitments += 1
    assert n >= 15 and with_commitments >= 10, (n, with_commitments)


def _batch(flows):
    """one accepted golden presentation with proofs of encryption, tiled to 3 items, as columns + commitments"""
    import aeonflux_amd as afx
    for f, issuer, p, shape in _flow_items(flows):
        if f["verify"] == 0 and p.n_enc_proofs:
            cm = B.to_batchable(issuer, p)
            a = presentation_arrays([p, p, p])
            return afx, shape, a, B.arrays_of([cm, cm, cm])
    pytest.fail("no accepted flow with a proof of encryption")


def _c_pack(afx, shape, a, cm, n_main):
    from aeonflux_amd import batch
    soa, k1 = batch.presentation_soa(a)
    csoa, k2 = batch.commitments_soa(cm)
    n = C.c_size_t(0)
    count = a["responses"].shape[1]
    afx.check(afx.lib().afx_batchable_wire_pack(C.byref(shape), C.byref(soa), C.byref(csoa), n_main, count, None, 0, C.byref(n)))   # the size query
    buf = np.zeros(n.value, np.uint8)
    assert afx.lib().afx_batchable_wire_pack(C.byref(shape), C.byref(soa), C.byref(csoa), n_main, count, buf.ctypes.data, n.value - 1, C.byref(n)) == afx.E_BAD_ARGS
    afx.check(afx.lib().afx_batchable_wire_pack(C.byref(shape), C.byref(soa), C.byref(csoa), n_main, count, buf.ctypes.data, n.value, C.byref(n)))
    return buf.tobytes()


def _parse(afx, blob):
    sh, m, cnt, off = afx.Shape(), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
    rc = afx.lib().afx_batchable_wire_parse(blob, len(blob), C.byref(sh), C.byref(m), C.byref(cnt), C.byref(off))
    return rc, sh, m.value, cnt.value, off.value


def test_pack_parse_and_section_length_round_trips(flows):
    from aeonflux_amd import wire
    afx, shape, a, cm = _batch(flows)
    n_main = cm["main"].shape[0]
    blob = _c_pack(afx, shape, a, cm, n_main)
    assert blob == wire.pack_batchable(shape, a, cm)                       # the C packer and the Python mirror write the same bytes
    assert blob[:4] == b"AFXB" and len(blob) % 32 == 0
    rc, sh, m, cnt, off = _parse(afx, blob)
    assert rc == 0 and bytes(sh) == bytes(shape) and m == n_main and cnt == 3
    assert off == afx.lib().afx_batchable_wire_header_bytes(C.byref(shape)) and off % 32 == 0
    assert len(blob) == off + 3 * 32 * afx.lib().afx_batchable_wire_cells_per_record(C.byref(shape), n_main)
    sh2, p2, cm2 = wire.unpack_batchable(blob)
    assert bytes(sh2) == bytes(shape) and np.array_equal(cm2["main"], cm["main"]) and all(np.array_equal(x, y) for x, y in zip(cm2["enc"], cm["enc"]))
    for f in ("responses", "C_x_0", "C_x_1", "C_V", "C_y"):
        assert np.array_equal(p2[f], a[f]), f
    for d2, d in zip(p2["enc"], a["enc"]):
        for f in wire.ENC_ORDER[1:]:
            assert np.array_equal(d2[f], d[f]), f
    assert wire.pack_batchable(sh2, p2, cm2) == blob
    # sections back to back: each names its own length
    stream = blob + blob
    sl = C.c_size_t(0)
    assert afx.lib().afx_batchable_wire_section_bytes(stream, len(stream), C.byref(sl)) == 0 and sl.value == len(blob)
    assert afx.lib().afx_batchable_wire_section_bytes(stream, len(blob) - 1, C.byref(sl)) == afx.E_BAD_ARGS
    # an empty section is a header
    empty = wire.pack_batchable(shape, {k: (v[..., :0, :] if k != "enc" else [{f: x[..., :0, :] for f, x in d.items()} for d in v]) for k, v in a.items()},
                                {"main": cm["main"][:, :0], "enc": [c[:, :0] for c in cm["enc"]]})
    assert _parse(afx, empty)[0] == 0 and len(empty) == off


def test_malformed_headers_are_bad_args(flows):
    from aeonflux_amd import wire
    afx, shape, a, cm = _batch(flows)
    blob = wire.pack_batchable(shape, a, cm)
    n_main = cm["main"].shape[0]
    assert _parse(afx, blob)[0] == 0

    def put32(at, v):
        return blob[:at] + struct.pack("<I", v) + blob[at + 4:]
    cells = struct.unpack("<I", blob[12:16])[0]
    bad = {
        "magic": b"AFXP" + blob[4:], "version": put32(4, 2), "count too large": put32(8, 4), "count too small": put32(8, 2),
        "cells": put32(12, cells + 1), "n_attributes out of range": put32(16, 33), "n_enc_proofs out of range": put32(28, 33),
        "n_main + 1": put32(32, n_main + 1), "n_main - 1": put32(32, n_main - 1), "n_main 0": put32(32, 0), "n_main huge": put32(32, 0xffffffff),
        "truncated header": blob[:35], "truncated in the kinds": blob[:38], "truncated records": blob[:-1], "trailing bytes": blob + b"\0",
        "trailing cell": blob + bytes(32), "kind out of range": blob[:36] + b"\x09" + blob[37:], "empty": b"",
    }
    for name, b in bad.items():
        assert _parse(afx, b)[0] == afx.E_BAD_ARGS, name
    # n_main and the cell count changed TOGETHER still do not make a header the shape allows
    assert _parse(afx, put32(12, cells + 1)[:32] + struct.pack("<I", n_main + 1) + blob[36:])[0] == afx.E_BAD_ARGS
    sl = C.c_size_t(0)
    for name in ("magic", "version", "truncated header", "truncated records", "empty"):
        assert afx.lib().afx_batchable_wire_section_bytes(bad[name], len(bad[name]), C.byref(sl)) == afx.E_BAD_ARGS, name
    # null arguments
    sh, m, cnt, off = afx.Shape(), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0)
    assert afx.lib().afx_batchable_wire_parse(None, 0, C.byref(sh), C.byref(m), C.byref(cnt), C.byref(off)) == afx.E_BAD_ARGS
    assert afx.lib().afx_batchable_wire_parse(blob, len(blob), None, C.byref(m), C.byref(cnt), C.byref(off)) == afx.E_BAD_ARGS
    assert afx.lib().afx_batchable_wire_header_bytes(None) == 0 and afx.lib().afx_batchable_wire_cells_per_record(None, n_main) == 0
    big = afx.Shape.from_buffer_copy(bytes(shape))
    big.n_attributes = 33
    assert afx.lib().afx_batchable_wire_header_bytes(C.byref(big)) == 0
