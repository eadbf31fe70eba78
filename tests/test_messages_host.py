"""CPU-only: the host side of the whole-message calls (aeonflux_amd/csrc/statements_messages.cpp), on the built library as
tests/test_wire.py loads it for the packers: the chunk count, the chunk table against Python, refusal of malformed tables with
nothing written, and NULL arguments of every new call refused before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import aeonflux_amd as afx
from aeonflux_amd import batch
from tests import messages_ref as ref


def test_message_chunks_at_the_edges():
    want = {0: 0, 1: 1, 29: 1, 30: 1, 31: 2, 60: 2, 2**64 - 1: (2**64 - 1) // 30 + 1}
    assert {n: batch.message_chunks(n) for n in want} == want
    assert (2**64 - 1) % 30 != 0          # (the last one rounds up: len + 29 would have wrapped)


def test_chunk_table_against_python():
    r = np.random.default_rng(20261019)
    for lengths in ([], [0], [0, 0, 0], [1], [30], [31, 0, 0, 59, 60, 61, 0], list(r.integers(0, 200, 500)), [3000] * 7):
        msgs = [bytes(int(n)) for n in lengths]
        blob, offsets = batch.pack_messages(msgs)
        assert offsets.tolist() == [sum(len(m) for m in msgs[:i]) for i in range(len(msgs) + 1)] and blob.size == offsets[-1]
        assert batch.chunk_table(offsets).tolist() == ref.chunk_first(msgs)
    # offsets need not start at 0: message i is blob[offsets[i] .. offsets[i + 1])
    assert batch.chunk_table(np.array([7, 7, 8, 68, 69], np.uint64)).tolist() == [0, 0, 1, 3, 4]


def test_malformed_tables_are_refused_and_nothing_is_written():
    lib = afx.lib()
    cf = np.full(4, 0xA5A5A5A5, np.uint32)
    dec = np.array([0, 40, 39, 80], np.uint64)
    assert lib.afx_messages_chunk_table(dec.ctypes.data, 3, cf.ctypes.data) == afx.E_BAD_ARGS and (cf == 0xA5A5A5A5).all()
    assert b"decrease" in lib.afx_last_error()
    # more than 2^32 - 1 chunks: two messages of 2^36 bytes (offsets only - no blob is read)
    big = np.array([0, 30 * (2**31), 30 * (2**32)], np.uint64)
    assert lib.afx_messages_chunk_table(big.ctypes.data, 2, cf.ctypes.data) == afx.E_BAD_ARGS and (cf == 0xA5A5A5A5).all()
    fits = np.array([0, 30 * (2**31), 30 * (2**32 - 1)], np.uint64)
    assert lib.afx_messages_chunk_table(fits.ctypes.data, 2, cf.ctypes.data) == 0
    assert cf[:3].tolist() == [0, 2**31, 2**32 - 1]
    with pytest.raises(Exception):
        batch.chunk_table(dec)


def test_null_arguments_of_every_new_call_are_bad_args():
    """(a NULL context first of all: nothing here reaches a device)"""
    lib = afx.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    kp = afx.KeypairsSoA(p, p, p, None)
    off = np.array([0, 10], np.uint64)
    cf = np.array([0, 1], np.uint32)
    o, c = off.ctypes.data, cf.ctypes.data
    E = afx.E_BAD_ARGS
    assert lib.afx_messages_chunk_table(None, 1, c) == E and lib.afx_messages_chunk_table(o, 1, None) == E
    for sfx, tail in (("", ()), ("_dev", (p,))):
        f = getattr(lib, "afx_plaintexts_from_messages" + sfx)
        assert f(None, p, o, 1, p, p, p, p, *tail) == E
    for sfx in ("", "_dev"):
        assert getattr(lib, "afx_plaintexts_from_points" + sfx)(None, p, 1, p, p, p) == E
        assert getattr(lib, "afx_plaintexts_from_bytes_at" + sfx)(None, p, p, 1, p, p, p, p) == E
        assert getattr(lib, "afx_encrypt_messages" + sfx)(None, C.byref(kp), p, o, 1, p, p, p, p) == E
        assert getattr(lib, "afx_decrypt_messages" + sfx)(None, C.byref(kp), p, p, c, 1, p, p) == E
        # a missing keypair struct or key row with everything else in place is refused at the same door
        assert getattr(lib, "afx_encrypt_messages" + sfx)(None, None, p, o, 1, p, p, p, p) == E
        assert getattr(lib, "afx_decrypt_messages" + sfx)(None, None, p, p, c, 1, p, p) == E
