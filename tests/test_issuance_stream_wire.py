"""CredentialIssuance streams ("AFXI" v1 sections back to back, as afx_issue_wire writes them), CPU only: afx_issuance_wire_section_bytes
measures a section from its header alone and refuses every malformed header, and walking a packed stream with it gives back the
sections it was built from."""
import ctypes as C
import struct

import numpy as np
import pytest


def issuances(kinds, count, nr, seed):
    from aeonflux_amd import wire
    rng = np.random.default_rng(seed)
    iss = {k: rng.integers(0, 256, size=(count, 32), dtype=np.uint8) for k in ("t", "U", "V", "challenge")}
    iss["responses"] = rng.integers(0, 256, size=(nr, count, 32), dtype=np.uint8)
    values = rng.integers(0, 256, size=(len(kinds), count, 32), dtype=np.uint8)
    return wire.pack_issuances(list(kinds), values, iss)


def section_bytes(blob, length=None):
    import aeonflux_amd as afx
    n = C.c_size_t(12345)
    rc = afx.lib().afx_issuance_wire_section_bytes(blob, len(blob) if length is None else length, C.byref(n))
    return rc, n.value


def split(blob):
    from aeonflux_amd import wire
    out, off = [], 0
    while off < len(blob):
        sl = wire.issuance_section_bytes(blob[off:])
        out.append(blob[off:off + sl])
        off += sl
    return out


LAYOUTS = [((1, 0, 2, 3), 5, 9), ((1,) * 8 + (2,) * 4 + (4,) * 4, 3, 21), ((2,), 1, 6), ((0, 1, 4), 0, 8), ((), 4, 5), ((4,) * 32, 2, 37)]


@pytest.mark.parametrize("kinds,count,nr", LAYOUTS)
def test_a_single_section_is_measured_from_its_header(kinds, count, nr):
    import aeonflux_amd as afx
    blob = issuances(kinds, count, nr, 3 + count)
    hdr = afx.lib().afx_issuance_wire_header_bytes(len(kinds))
    assert len(blob) == hdr + count * (4 + nr + len(kinds)) * 32
    assert section_bytes(blob) == (afx.OK, len(blob))
    # anything behind the section is not the section's business
    assert section_bytes(blob + b"\0" * 40) == (afx.OK, len(blob))
    # a section that runs past the end of what was given
    if count:
        assert section_bytes(blob, len(blob) - 1)[0] == afx.E_BAD_ARGS
        assert section_bytes(blob[:-32])[0] == afx.E_BAD_ARGS


@pytest.mark.parametrize("kinds,count,nr", LAYOUTS[:3])
def test_truncation_at_every_header_byte_is_refused(kinds, count, nr):
    import aeonflux_amd as afx
    blob = issuances(kinds, count, nr, 11)
    hdr = afx.lib().afx_issuance_wire_header_bytes(len(kinds))
    for cut in range(hdr):
        assert section_bytes(blob[:cut])[0] == afx.E_BAD_ARGS, cut


def test_magic_version_and_layout_fields_are_checked():
    import aeonflux_amd as afx
    blob = bytearray(issuances((1, 0, 2, 3), 2, 9, 5))
    ok = bytes(blob)
    put = lambda at, v: ok[:at] + struct.pack("<I", v) + ok[at + 4:]
    for bad in (b"AFXP" + ok[4:], b"AFXR" + ok[4:], b"afxi" + ok[4:], put(4, 0), put(4, 2), put(4, 0x01000000)):
        assert section_bytes(bad)[0] == afx.E_BAD_ARGS
    # cells_per_record must be 4 + n_responses + n_attributes
    for cells in (0, 1, 16, 18, 0xffffffff):
        assert section_bytes(put(12, cells))[0] == afx.E_BAD_ARGS, cells
    # n_attributes and n_responses out of range (and cells made to agree, so that only the range check can refuse)
    big = put(16, 33)
    big = big[:12] + struct.pack("<I", 4 + 9 + 33) + big[16:]
    assert section_bytes(big + bytes(4096))[0] == afx.E_BAD_ARGS
    big = put(20, 38)
    big = big[:12] + struct.pack("<I", 4 + 38 + 4) + big[16:]
    assert section_bytes(big + bytes(8192))[0] == afx.E_BAD_ARGS
    # a count that promises more records than there are
    assert section_bytes(put(8, 3))[0] == afx.E_BAD_ARGS
    assert section_bytes(put(8, 0xffffffff))[0] == afx.E_BAD_ARGS
    # a smaller count is a shorter section: the rest is the next section's business
    assert section_bytes(put(8, 1)) == (afx.OK, 32 + 17 * 32)
    assert section_bytes(None, 0)[0] == afx.E_BAD_ARGS


def test_splitting_a_packed_stream_gives_back_its_sections():
    sections = [issuances(k, c, nr, 100 + i) for i, (k, c, nr) in enumerate(LAYOUTS)]
    sections += [sections[0], issuances((1, 0, 2, 3), 1, 9, 7), sections[4]]
    stream = b"".join(sections)
    assert split(stream) == sections


def test_another_format_in_the_middle_of_a_stream_stops_the_walk_there():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    a, b = issuances((1, 0, 2, 3), 3, 9, 1), issuances((2, 2), 2, 7, 2)
    afxr = wire.pack_requests([1, 0, 2, 3], np.zeros((4, 2, 32), np.uint8))
    afxp = b"AFXP" + struct.pack("<7I", 1, 0, 6, 1, 3, 0, 0) + bytes([2]) + bytes(31)
    for other in (afxr, afxp):
        stream = a + other + b
        assert section_bytes(stream) == (afx.OK, len(a))
        assert section_bytes(stream[len(a):])[0] == afx.E_BAD_ARGS
        with pytest.raises(afx.AfxError):
            split(stream)
