"""The yardstick of the whole-message calls (include/aeonflux_gpu.h "whole messages"), composed from the existing oracle: chunk and pad
in Python as Plaintext::from_slice does (src/symmetric.rs:118-133: `chunks(30)`, the last chunk zero-padded), then
oracle.plaintext_from_bytes, oracle.encrypt and oracle.decrypt per chunk; the from-point form (src/symmetric.rs:152-161) is
oracle.sha512 -> oracle.point_from_uniform / oracle.scalar_reduce_wide; the candidate at a counter (src/encoding.rs:56-70) is built
here and tested with oracle.point_decode_encode.  Keypairs are the oracle's 128 bytes a || a0 || a1 || pk, one per MESSAGE."""
import oracle

ST_OK, ST_VERIFICATION_FAILURE, ST_UNDECRYPTABLE = 0, 1, 4
ZERO32 = bytes(32)


def chunks(message):
    """the 30-byte chunks of a message, the last one zero-padded; an empty message has none"""
    return [message[i:i + 30].ljust(30, b"\0") for i in range(0, len(message), 30)]


def padded(message):
    return b"".join(chunks(message))


def chunk_first(messages):
    cf = [0]
    for m in messages:
        cf.append(cf[-1] + (len(m) + 29) // 30)
    return cf


def plaintexts_from_messages(messages):
    """per chunk, in row order: (M1, M2, m3, counter)"""
    rows = []
    for m in messages:
        for c in chunks(m):
            pt, ctr = oracle.plaintext_from_bytes(c)
            rows.append((pt[:32], pt[32:64], pt[64:96], ctr))
    return rows


def plaintext_from_point(point):
    """(M2, m3) of a point attribute held only as a point, or None for an encoding that does not decode"""
    if oracle.point_decode_encode(point) is None:
        return None
    wide = oracle.sha512(point)
    return oracle.point_from_uniform(wide), oracle.scalar_reduce_wide(wide)


def candidate(msg30, counter):
    """encode_to_group's candidate at a counter: i fastest (bytes[0] = 2 i), j in the last byte"""
    assert len(msg30) == 30 and 0 <= counter < 8192
    return bytes([2 * (counter % 128)]) + msg30 + bytes([counter // 128])


def decodes(enc):
    return oracle.point_decode_encode(enc) is not None


def plaintext_at(msg30, counter):
    """(M1, M2, m3) with M1 the candidate at `counter`, or None where that candidate does not decode or counter >= 8192"""
    if counter >= 8192 or not decodes(candidate(msg30, counter)):
        return None
    wide = oracle.sha512(msg30)
    return candidate(msg30, counter), oracle.point_from_uniform(wide), oracle.scalar_reduce_wide(wide)


def encrypt_messages(keypairs, messages):
    """-> (E1 rows, E2 rows, counters, status per message); the rows of a failed message are zeros"""
    E1, E2, counters, status = [], [], [], []
    for kp, m in zip(keypairs, messages):
        rows, bad = [], False
        for c in chunks(m):
            pt, ctr = oracle.plaintext_from_bytes(c)
            ct = oracle.encrypt(kp, pt)
            bad |= ct is None
            rows.append((ct[:32], ct[32:], ctr) if ct is not None else (ZERO32, ZERO32, 0))
        if bad:
            rows = [(ZERO32, ZERO32, 0)] * len(rows)
        for e1, e2, ctr in rows:
            E1.append(e1); E2.append(e2); counters.append(ctr)
        status.append(ST_VERIFICATION_FAILURE if bad else ST_OK)
    return E1, E2, counters, status


def decrypt_messages(keypairs, E1, E2, cf):
    """-> (messages as bytes of 30 * chunks(i), status per message); a message one of whose chunks does not decrypt is all zeros"""
    out, status = [], []
    for i, kp in enumerate(keypairs):
        parts, bad = [], False
        for r in range(cf[i], cf[i + 1]):
            rc, pt = oracle.decrypt(kp, E1[r] + E2[r])
            bad |= rc != 0
            parts.append(pt[1:31])
        out.append(bytes(30 * len(parts)) if bad else b"".join(parts))
        status.append(ST_UNDECRYPTABLE if bad else ST_OK)
    return out, status
