"""The hole-offset sweep of the transcript tests (tests/test_gpu_hash_kernels.py on the device, tests/test_hostsim_hash_sweep.py on
the host simulation): the scripts, the per-item fields, and a restatement of where STROBE's position stands at every byte.

A per-item 32-byte value is a HOLE in the compiled byte schedule (aeonflux_amd/csrc/strobe_sim.hpp): each 8-byte word of a 166-byte
rate block that holds some of its bytes names the field, the 64-bit word q of the field that holds the word's lowest selected byte
(-1 .. 3) and a byte rotation r (0 .. 7) (plan.h afx_hash_word).  positions() below follows merlin's operations byte by byte the way
STROBE-128 does (2 bytes open an operation, the rate is 166 bytes, an operation with the C flag permutes first) and says where every
hole byte lands, without looking at the engine: the tests assert from it that the sweep reaches every case they are there for."""
import hashlib

R = 166                      # STROBE-128's rate in bytes
K_RANGE = range(171)         # pad lengths: the first hole then starts at every residue of the rate
PATTERN = bytes((37 * i + 11) & 0xff for i in range(256))


def sweep_ops(k):
    """pad of k bytes, two different holes 8 bytes apart (an empty label: the closest two can lie), an empty append, the first again"""
    return [("append", b"pad", PATTERN[:k]), ("append_field", b"", 0), ("append_field", b"", 1), ("append", b"", b""),
            ("append_field", b"again", 0), ("challenge", b"c", 64)]


SWEEP_LABEL = b"hole sweep"


def fields_for(tag, count, n_fields=2):
    """n_fields arrays [count][32] of bytes from shake_256 (as bytes objects, item-major)"""
    raw = hashlib.shake_256(b"hash-sweep-fields:" + tag).digest(32 * count * n_fields)
    return [raw[32 * count * f:32 * count * (f + 1)] for f in range(n_fields)]


def positions(label, ops):
    """[(record, position in the rate, byte of the field, which append_field)] for every hole byte of the script"""
    st = dict(pos=0, rec=0)
    holes = []

    def run_f():
        st["pos"] = 0
        st["rec"] += 1

    def absorb(n, hole=None):
        for j in range(n):
            if hole is not None:
                holes.append((st["rec"], st["pos"], j, hole))
            st["pos"] += 1
            if st["pos"] == R:
                run_f()

    def begin_op(forces_f):
        absorb(2)            # the previous operation's start and the flags
        if forces_f and st["pos"] != 0:
            run_f()

    def meta_ad(n, more):
        if not more:
            begin_op(False)
        absorb(n)

    def append(llen, n, hole=None):
        meta_ad(llen, False)
        meta_ad(4, True)     # the length, little-endian
        begin_op(False)
        absorb(n, hole)

    meta_ad(len(b"Merlin v1.0"), False)
    append(len(b"dom-sep"), len(label))
    n_hole = 0
    for op in ops:
        if op[0] == "append":
            append(len(op[1]), len(op[2]))
        elif op[0] == "append_field":
            append(len(op[1]), 32, n_hole)
            n_hole += 1
        elif op[0] == "challenge":
            meta_ad(len(op[1]), False)
            meta_ad(4, True)
            begin_op(True)
            st["pos"] = op[2]    # the squeezed bytes are zeroed and the position moves behind them
        else:
            raise ValueError(op[0])
    return holes


def words_of(holes):
    """{(record, word, hole): (q, r)} as StrobeSim::to_device derives them: field byte = stream byte in the word + 8 q + r"""
    out = {}
    for rec, pos, fbyte, hole in holes:
        delta = fbyte - pos % 8
        qr = (delta // 8, delta % 8)      # floor division: -1 for a hole that starts inside the word
        assert out.setdefault((rec, pos // 8, hole), qr) == qr
    return out


def coverage(label=SWEEP_LABEL, ks=K_RANGE):
    """what the sweep reaches: start positions, (q, r) pairs, where the rate boundary cuts a hole (bytes before it), words 20 (6 bytes) with a hole"""
    starts, qrs, cut, word20 = set(), set(), set(), 0
    for k in ks:
        holes = positions(label, sweep_ops(k))
        starts |= {pos for rec, pos, fbyte, hole in holes if fbyte == 0}
        w = words_of(holes)
        qrs |= set(w.values())
        word20 += sum(1 for (rec, word, hole) in w if word == 20)
        first = {hole: rec for rec, pos, fbyte, hole in holes if fbyte == 0}
        for h in first:            # a hole cut by the rate boundary: how many of its bytes lie before it
            before = sum(1 for rec, pos, fbyte, hole in holes if hole == h and rec == first[h])
            if before < 32:
                cut.add(before)
    return dict(starts=starts, qrs=qrs, cut=cut, word20=word20)


# every (q, r) a word can carry: q = -1 means the hole starts inside the word, r bytes short of its end - so never with r = 0, which
# would be a word holding no byte of the field at all
ALL_QR = {(q, r) for q in range(-1, 4) for r in range(8)} - {(-1, 0)}
