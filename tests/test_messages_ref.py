"""CPU-only self-checks of tests/messages_ref.py, the yardstick of the whole-message calls: chunking as Plaintext::from_slice does it,
the round trip through the oracle's encrypt and decrypt, the candidate at a counter against the oracle's own search, and the fact the
from-point form pins - the crate hashes the point's 32 bytes there, not the 30 bytes the point encodes."""
import hashlib

import pytest

from tests import messages_ref as ref

LENGTHS = [0, 0, 1, 29, 30, 31, 59, 60, 0, 61, 90, 300, 3000, 0]


@pytest.fixture(scope="module")
def octx():
    import oracle
    st = hashlib.shake_256(b"afx-tests/plaintext-context/v1").digest(1 << 15)
    params, used = oracle.system_parameters_generate(5, st)
    _, ip = oracle.issuer_new(params, st[used:used + 64 * 9])
    return oracle.Ctx(params, None, ip)


def messages():
    src = hashlib.shake_256(b"afx-tests/messages-ref/v1").digest(sum(LENGTHS))
    out, at = [], 0
    for n in LENGTHS:
        out.append(src[at:at + n])
        at += n
    return out


def test_chunking_is_chunks_of_30_zero_padded():
    assert ref.chunks(b"") == [] and ref.chunks(b"abc") == [b"abc" + bytes(27)] == ref.chunks(b"abc\0")
    assert [len(ref.chunks(bytes(n))) for n in (0, 1, 29, 30, 31, 60, 61)] == [0, 1, 1, 1, 2, 2, 3]
    m = bytes(range(61))
    assert ref.chunks(m) == [m[:30], m[30:60], m[60:] + bytes(29)] and ref.padded(m) == m + bytes(29)
    assert ref.chunk_first([b"", b"x", bytes(30), bytes(31), b""]) == [0, 0, 1, 2, 4, 4]


def test_round_trip_returns_every_padded_message(octx):
    msgs = messages()
    keys = [octx.keypair_derive(hashlib.shake_256(b"afx-tests/messages-ref/key/%d" % i).digest(64)) for i in range(len(msgs))]
    E1, E2, counters, status = ref.encrypt_messages(keys, msgs)
    cf = ref.chunk_first(msgs)
    assert len(E1) == len(E2) == len(counters) == cf[-1] == sum((n + 29) // 30 for n in LENGTHS) and status == [ref.ST_OK] * len(msgs)
    back, st = ref.decrypt_messages(keys, E1, E2, cf)
    assert st == [ref.ST_OK] * len(msgs) and back == [ref.padded(m) for m in msgs]
    # under a neighbour's key nothing of a non-empty message comes back; an empty one has nothing to fail
    wrong, st = ref.decrypt_messages(keys[1:] + keys[:1], E1, E2, cf)
    assert st == [ref.ST_UNDECRYPTABLE if n else ref.ST_OK for n in LENGTHS] and all(w == bytes(len(w)) for w in wrong)


def test_the_candidate_at_the_oracles_counter_is_the_oracles_M1():
    import oracle
    src = hashlib.shake_256(b"afx-tests/messages-ref/at/v1").digest(30 * 64)
    seen_later = 0
    for i in range(64):
        m = src[30 * i:30 * i + 30]
        pt, ctr = oracle.plaintext_from_bytes(m)
        assert ref.plaintext_at(m, ctr) == (pt[:32], pt[32:64], pt[64:96])
        assert all(ref.plaintext_at(m, c) is None for c in range(ctr))          # the search stops at the first that decodes
        later = next(c for c in range(ctr + 1, 8192) if ref.decodes(ref.candidate(m, c)))
        M1, M2, m3 = ref.plaintext_at(m, later)
        assert M1 != pt[:32] and (M2, m3) == (pt[32:64], pt[64:96]) and oracle.decode_from_group(M1)[0] == m
        seen_later += 1
    assert seen_later == 64 and ref.plaintext_at(src[:30], 8192) is None
    assert ref.candidate(bytes(30), 0) == bytes(32) and ref.candidate(b"\x01" * 30, 129) == b"\x02" + b"\x01" * 30 + b"\x01"


def test_the_from_point_triple_is_not_the_from_bytes_triple():
    import oracle
    m = hashlib.shake_256(b"afx-tests/messages-ref/point/v1").digest(30)
    pt, _ = oracle.plaintext_from_bytes(m)
    M2, m3 = ref.plaintext_from_point(pt[:32])
    assert (M2, m3) != (pt[32:64], pt[64:96]) and M2 != pt[32:64] and m3 != pt[64:96]
    wide = hashlib.sha512(pt[:32]).digest()
    assert (M2, m3) == (oracle.point_from_uniform(wide), oracle.scalar_reduce_wide(wide))
    assert ref.plaintext_from_point(bytes(32)) is not None            # the identity is a valid input
    bad = next(ref.candidate(m, c) for c in range(8192) if not ref.decodes(ref.candidate(m, c)))
    assert ref.plaintext_from_point(bad) is None
