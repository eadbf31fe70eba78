"""The case list of the arithmetic headers (aeonflux_amd/csrc/fe.cuh, fe10.cuh, ge.cuh, sc.cuh), shared by the two builds that run it:
tests/test_device_arith_on_host.py (g++, every product under the bounds checker) and tests/test_gpu_device_arith.py (hipcc for
gfx950, one case per lane).  Generators, the packing into words, the expected results from Python integers / pyref / the oracle,
and the two builders.  A plain module: no pytest hooks, no fixtures."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
M32 = 0xffffffff


def stream(seed, n):
    return hashlib.shake_256(seed).digest(n)


def b32(v):
    return int(v).to_bytes(32, "little")


def words(b):
    """bytes -> little-endian 32-bit words"""
    return [int.from_bytes(b[i:i + 4], "little") for i in range(0, len(b), 4)]


def unwords(w):
    return b"".join(int(x).to_bytes(4, "little") for x in w)


def s32(x):
    return x - (1 << 32) if x >= 1 << 31 else x


# ---- fe.cuh: 9 limbs of 29 bits (limb 8: 23) ----

UNIT = [1 << 29] * 8 + [1 << 23]


def limbs_value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def product_cases():
    """operands with every limb at the extreme of its range, all sign patterns that maximise a column: 8 magnitude pairs x 16 sign
    patterns, then 300 random limit cases (|f| * |g| = 3.8 units, or 1 x 1)"""
    rnd = random.Random(9)

    def limbs(mag, mode):
        v = []
        for i in range(9):
            top = int(UNIT[i] * mag) - 1
            x = top if mode != "random" or rnd.random() < 0.5 else rnd.randrange(0, top + 1)
            sign = {"pos": 1, "neg": -1, "alt": (-1) ** i, "random": rnd.choice((1, -1))}[mode]
            v.append(sign * x)
        return v
    cases = []
    for ma, mb in ((1, 1), (2, 1), (2, 1.9), (3.8, 1), (1, 3.8), (1.9, 1.99), (3, 1.25), (1.5, 2)):
        for sa in ("pos", "neg", "alt", "random"):
            for sb in ("pos", "neg", "alt", "random"):
                cases.append((limbs(ma, sa), limbs(mb, sb)))
    for _ in range(300):
        ma = rnd.choice((1, 2, 3.8))
        cases.append((limbs(ma, "random"), limbs(3.8 / ma if ma > 1 else 1, "random")))
    return cases


def squaring_operand(f):
    """the squaring takes |f| <= 1.9: scale f down for it when the case is a wider operand"""
    return f if max(abs(x) / u for x, u in zip(f, UNIT)) <= 1.9 else [x // 2 for x in f]


def encoding_limb_cases():
    """limb patterns around 0, p and 2^255, positive and negative, lazily added, up to the int32 range (fe_tobytes, fe_carry)"""
    p_limbs = [(1 << 29) - 19] + [(1 << 29) - 1] * 7 + [(1 << 23) - 1]
    return [[0] * 9, [1] + [0] * 8, [-1] + [0] * 8, [-19] + [0] * 8, [-20] + [0] * 8, p_limbs, [x + (i == 0) for i, x in enumerate(p_limbs)],
            [x - (i == 0) for i, x in enumerate(p_limbs)], [-x for x in p_limbs], [2 * x for x in p_limbs], [-2 * x for x in p_limbs],
            [(1 << 29) - 1] * 8 + [(1 << 23) - 1], [18] + [0] * 8, [19] + [0] * 8, [0] * 8 + [1 << 23], [0] * 8 + [-(1 << 23)],
            [3 * x for x in p_limbs], [(1 << 31) - 1] * 9, [-(1 << 31)] * 9, [(-1) ** i * ((1 << 31) - 1) for i in range(9)]]


def field_byte_edges():
    return [bytes(32), (1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little"), (P).to_bytes(32, "little"), b"\xff" * 32,
            (2 ** 255 - 1).to_bytes(32, "little"), (2 ** 254).to_bytes(32, "little"), (19).to_bytes(32, "little")]


def field_byte_cases():
    """400 random pairs of encodings, then every pair of the edge encodings"""
    s = stream(b"fe-host", 64 * 400)
    edge = field_byte_edges()
    return [(s[64 * i:64 * i + 32], s[64 * i + 32:64 * i + 64]) for i in range(400)] + [(a, b) for a in edge for b in edge]


# ---- fe10.cuh: 10 limbs of 26 / 25 bits ----

FE10_BITS = [26, 25] * 5
FE10_OFFSET = [sum(FE10_BITS[:i]) for i in range(10)]
FE10_TOP = [(1 << b) - 1 for b in FE10_BITS]
# The largest carry the wrap can leave on limb 1 of a raw result, from the header's "column sums stay below 2^62" (what
# afx_check_products10 enforces on the magnitudes, the incoming carry apart).  Column k's chain is H_k = sum_k + c_(k-1) with
# c_(k-1) = H_(k-1) >> 25 or 26, so c_8 < (2^62 + c_7) / 2^26 < 2^36 + 2^11 and H_9 < 2^62 + 2^36 + 2^11; c_9 = H_9 >> 25
# < 2^37 + 2^11 + 1.  The wrap adds 19 * c_9 to limb 0 (u0 < 2^26): H0 < 2^26 + 19 * 2^37 + 19 * (2^11 + 1), and what goes to
# limb 1 is H0 >> 26 <= 19 * 2^11 + 1.
FE10_WRAP_CARRY = 19 * (1 << 11) + 1
FE10_RANGE = [t + (FE10_WRAP_CARRY if i == 1 else 0) for i, t in enumerate(FE10_TOP)]   # largest raw limb, each position


def limbs10_value(l):
    return sum(int(x) << FE10_OFFSET[i] for i, x in enumerate(l))


def fe10_operands():
    """the raw range's corners: zero, all one, all top, alternating top / 0 in both phases, one limb at 1 or at its top with the
    rest zero; limb 1 with the largest wrap carry on top wherever it is at its top"""
    top = list(FE10_TOP)
    with_carry = lambda v: [x + (FE10_WRAP_CARRY if i == 1 else 0) for i, x in enumerate(v)]
    ops = [[0] * 10, [1] * 10, top, with_carry(top), [t if i % 2 == 0 else 0 for i, t in enumerate(top)],
           [t if i % 2 else 0 for i, t in enumerate(top)], with_carry([t if i % 2 else 0 for i, t in enumerate(top)])]
    for i in range(10):
        ops.append([1 if j == i else 0 for j in range(10)])
        ops.append([top[i] if j == i else 0 for j in range(10)])
    ops.append(with_carry([top[1] if j == 1 else 0 for j in range(10)]))
    return ops


def fe10_limb_cases():
    """(f, g, which): every pair of fe10_operands(), 200 seeded random mixes that stick to the extremes (0, 1, top; limb 1: no carry or
    the largest) with probability 1/2 - all for the product, the squaring, the carry and the encoding (which = 5) - then operands for
    fe10_carry / fe10_tobytes alone (which = 4): p and its neighbours, negated and doubled values, int32 extremes"""
    rnd = random.Random(10)
    ops = fe10_operands()
    cases = [(f, g, 5) for f in ops for g in ops]

    def mix():
        v = []
        for i in range(10):
            x = rnd.choice((0, 1, FE10_TOP[i])) if rnd.random() < 0.5 else rnd.randrange(0, FE10_TOP[i] + 1)
            if i == 1:
                x += rnd.choice((0, FE10_WRAP_CARRY)) if rnd.random() < 0.5 else rnd.randrange(0, FE10_WRAP_CARRY + 1)
            v.append(x)
        return v
    for _ in range(200):
        cases.append((mix(), mix(), 5))
    p10 = [FE10_TOP[0] - 18] + FE10_TOP[1:]
    wide = [p10, [x + (i == 0) for i, x in enumerate(p10)], [x - (i == 0) for i, x in enumerate(p10)], [-x for x in p10], [2 * x for x in p10],
            [-2 * x for x in p10], [3 * x for x in p10], [-x for x in FE10_RANGE], [-1] + [0] * 9, [-19] + [0] * 9, [-20] + [0] * 9,
            [0] * 9 + [1 << 25], [0] * 9 + [-(1 << 25)], [(1 << 31) - 1] * 10, [-(1 << 31)] * 10, [(-1) ** i * ((1 << 31) - 1) for i in range(10)]]
    return cases + [(f, [0] * 10, 4) for f in wide]


def fe10_byte_patterns():
    """encodings for fe10_frombytes -> fe10_tobytes: 0, 1, p - 1, p, p + 1, 2^255 - 20 .. 2^255 - 1, and 2^255 + x (bit 255 is dropped)"""
    v = [0, 1, P - 1, P, P + 1] + list(range(2 ** 255 - 20, 2 ** 255))
    v += [2 ** 255 + x for x in (0, 1, 19, P - 1, P, 2 ** 254, 2 ** 255 - 1)]
    return [b32(x) for x in v]


def fe_bytes_cases():
    """(a, b) for case_fe_bytes: the field cases, then every fe10 byte pattern (paired with itself)"""
    return field_byte_cases() + [(a, a) for a in fe10_byte_patterns()]


# ---- ge.cuh ----

def sqrt_ratio_cases():
    """(u, v) as integers: u = 0; v = 0 with u != 0; u / v square; non-square; u / v = -1, i, -i; all pairs of {1, p - 1, 2, 19, 2^254,
    p - 2}; 100 seeded random pairs"""
    from tests.pyref import ristretto as R
    rnd = random.Random(11)
    rand = lambda: rnd.randrange(1, P)
    cases = [(0, 1), (0, 0), (0, rand()), (0, P - 1), (1, 0), (P - 1, 0), (rand(), 0), (2, 0)]
    for _ in range(8):
        v, x = rand(), rand()
        cases.append((v * x * x % P, v))                    # a square ratio
        cases.append((2 * v * x * x % P, v))                # 2 is no square mod p (p = 5 mod 8): a non-square ratio
    for _ in range(3):
        v = rand()
        cases += [((-v) % P, v), (R.SQRT_M1 * v % P, v), ((-R.SQRT_M1 * v) % P, v)]
    cases += [(P - 1, 1), (R.SQRT_M1, 1), (P - R.SQRT_M1, 1)]
    small = [1, P - 1, 2, 19, 2 ** 254, P - 2]
    cases += [(u, v) for u in small for v in small]
    cases += [(rand(), rand()) for _ in range(100)]
    return cases


def elligator_cases():
    """r0 as encodings: 0, 1, p - 1, sqrt(-1), -sqrt(-1), 2^254, the unreduced patterns 2^255 - 19 (= 0) and 2^255 - 1 (= 18) whose limbs
    fe_frombytes hands on as they are, 50 seeded random"""
    from tests.pyref import ristretto as R
    s = stream(b"elligator-edge", 32 * 50)
    fixed = [0, 1, P - 1, 2 ** 255 - 20, R.SQRT_M1, P - R.SQRT_M1, 2 ** 254, 2 ** 255 - 19, 2 ** 255 - 1]
    return [b32(x) for x in fixed] + [s[32 * i:32 * i + 32] for i in range(50)]


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def decode_encode_cases():
    """encodings, valid and invalid: RFC 9496's generator multiples and bad encodings (App. A.1, A.2), libsodium's validity vectors"""
    kat, prim = _golden("kat.json"), _golden("primitives.json")
    enc = list(kat["rfc9496_generator_multiples"]) + [x for grp in kat["rfc9496_bad_encodings"].values() for x in grp]
    enc += list(prim["base_multiples"]) + [v["in"] for v in prim["validity"]]
    return [bytes.fromhex(x) for x in enc]


def exceptional_points():
    """the base point, a random point, and the first two of RFC 9496's generator multiples whose decoded y is negative (odd)"""
    import oracle
    from tests.pyref import ristretto as R
    kat = _golden("kat.json")
    neg = [bytes.fromhex(x) for x in kat["rfc9496_generator_multiples"][1:] if R.decode(bytes.fromhex(x))[1] & 1]
    assert len(neg) >= 2
    return [bytes.fromhex(kat["rfc9496_B"]), oracle.point_from_uniform(stream(b"ge-exceptional", 64))] + neg[:2]


def point_ops_cases():
    """(P, Q): P over the exceptional points, Q over the same and the identity"""
    pts = exceptional_points()
    return [(p, q) for p in pts for q in pts + [bytes(32)]]


# ---- sc.cuh ----

def canonicity_values():
    """around l: l +- 2^(32 k) for every limb, l +- 1, the powers of two next to it, 2^256 - 1; and for each limb position a value equal
    to l above that limb and all zeros / all ones in and below it (the borrow chain decides at that limb)"""
    v = [L + s * (1 << (32 * k)) for k in range(8) for s in (1, -1)]
    v += [L + 1, L - 1, L, 0, 1, 2 ** 252, 2 ** 252 - 1, 2 ** 253 - 1, 2 ** 256 - 1]
    for j in range(8):
        above = (L >> (32 * (j + 1))) << (32 * (j + 1))
        v += [above, above | ((1 << (32 * (j + 1))) - 1)]
    assert all(0 <= x < 2 ** 256 for x in v)
    return v


def reduce512_values():
    """k * l + r at the ends of the reduction's trailing subtractions, h * 2^252 (+ 2^252 - 1) at the ends of each split at bit 252,
    2^512 - 1"""
    kmax = (2 ** 512 - 1) // L
    v = [k * L + r for k in (0, 1, 2, 3, 4, 2 ** 252, 2 ** 259, kmax - 1, kmax) for r in (0, 1, L - 1)]
    v = [x for x in v if x < 2 ** 512]                       # k * l + r has to fit: kmax * l + (l - 1) does not
    assert len(v) == 26 and kmax * L in v and kmax * L + 1 in v
    for h in (1, 2 ** 132 - 1, 2 ** 133, 2 ** 259, 2 ** 260 - 1):
        v += [h << 252, (h << 252) + 2 ** 252 - 1]
    # the running value at its top: lo1 and lo3 both next to 2^252, lo2 small, t3 = 0, so that acc >= 3 l and all three
    # subtractions that acc < 4 l can need are taken.  hi2 = the largest with hi2 * delta < 2^252 (then lo3 = hi2 * delta >
    # 2^252 - delta, hi3 = 0); hi1 = the smallest with hi1 * delta >= hi2 * 2^252 (then lo2 < delta)
    delta = L - 2 ** 252
    hi2 = (2 ** 252 - 1) // delta
    hi1 = -((-hi2 << 252) // delta)
    top = (hi1 << 252) + 2 ** 252 - 1
    assert hi1 < 2 ** 260 and 3 * L <= reduce512_acc(top) < 4 * L
    # and at its bottom: lo1 = 0, lo3 < delta, lo2 next to 2^252 and t3 = 16 delta, so that acc < l and no subtraction is taken.
    # hi2 = the smallest with hi2 * delta >= 16 * 2^252; hi1 = the largest with hi1 * delta < (hi2 + 1) * 2^252
    hi2 = -((-16 << 252) // delta)
    hi1 = (((hi2 + 1) << 252) - 1) // delta
    bottom = hi1 << 252
    assert hi1 < 2 ** 260 and 0 <= reduce512_acc(bottom) < L
    return v + [top, bottom, 2 ** 512 - 1]


def reduce512_acc(x):
    """sc_reduce512's running value before its trailing subtractions, step for step: lo1 + lo3 + 2 l - lo2 - t3"""
    delta, m = L - 2 ** 252, 2 ** 252 - 1
    t1 = (x >> 252) * delta
    t2 = (t1 >> 252) * delta
    t3 = (t2 >> 252) * delta
    assert x >> 252 < 2 ** 260 and t1 >> 252 < 2 ** 133 and t2 >> 252 < 2 ** 6 and t3 < 2 ** 131     # the header's size comments
    return (x & m) + (t2 & m) + 2 * L - (t1 & m) - t3


def muladd_triples():
    """(x, b, c), canonical: the largest operands, zero operands, a = 1; then (x, 0, 0) for the operands of sc_neg / sc_half / sc_dbl"""
    rnd = random.Random(12)
    r = lambda: rnd.randrange(L)
    t = [(L - 1, L - 1, L - 1), (0, 0, 0), (0, r(), r()), (r(), 0, r()), (0, L - 1, L - 1), (L - 1, 0, L - 1), (r(), r(), 0), (1, r(), r()),
         (1, L - 1, L - 1), (1, L - 1, 1), (r(), 1, 0), (1, 0, 0), (L - 1, 1, 1), (L - 1, L - 1, 0)]
    t += [(x, 0, 0) for x in (0, 1, 2, L - 1, L - 2, (L + 1) // 2, (L - 1) // 2)]
    return t


def scalar_cases():
    """(wide, a, x, b, c) as integers: the three lists above side by side, each repeated to the longest's length, then 64 random ones"""
    wide, can, tri = reduce512_values(), canonicity_values(), muladd_triples()
    n = max(len(wide), len(can), len(tri))
    cases = [(wide[i % len(wide)], can[i % len(can)]) + tri[i % len(tri)] for i in range(n)]
    rnd = random.Random(13)
    cases += [(rnd.randrange(2 ** 512), rnd.randrange(2 ** 256), rnd.randrange(L), rnd.randrange(L), rnd.randrange(L)) for _ in range(64)]
    return cases


# ---- the kinds: packing into words, expected results ----
# name -> (words in, words out); the order of arith_host_words / arith_dev_words
KINDS = {"fe_limbs": (28, 93), "fe10_limbs": (21, 54), "fe_bytes": (16, 40), "sqrt_ratio": (16, 9), "elligator": (8, 8),
         "decode_encode": (8, 9), "point_ops": (16, 121), "scalar": (48, 41)}


def _u32(l):
    return [x & M32 for x in l]


def rows_fe_limbs():
    rows = [_u32(f) + _u32(squaring_operand(f)) + _u32(g) + [7] for f, g in product_cases()]
    return rows + [_u32(v) + [0] * 18 + [4] for v in encoding_limb_cases()]


def rows_fe10_limbs():
    return [_u32(f) + _u32(g) + [w] for f, g, w in fe10_limb_cases()]


def rows_fe_bytes():
    return [words(a) + words(b) for a, b in fe_bytes_cases()]


def rows_sqrt_ratio():
    return [words(b32(u)) + words(b32(v)) for u, v in sqrt_ratio_cases()]


def rows_elligator():
    return [words(r) for r in elligator_cases()]


def rows_decode_encode():
    return [words(e) for e in decode_encode_cases()]


def rows_point_ops():
    return [words(p) + words(q) for p, q in point_ops_cases()]


def rows_scalar():
    return [words(w.to_bytes(64, "little")) + words(b32(a)) + words(b32(x)) + words(b32(b)) + words(b32(c)) for w, a, x, b, c in scalar_cases()]


def rows(kind):
    r = globals()["rows_" + kind]()
    assert all(len(x) == KINDS[kind][0] for x in r)
    return r


def _int(w):
    return int.from_bytes(unwords(w), "little")


def _in_ranges(l, raw, slack1, unit, what):
    """raw: limbs in [0, 1); centred: in [-1/2, 1/2]; limb 1 may hold slack1 more on either side"""
    for i, x in enumerate(l):
        s = slack1 if i == 1 else 0
        if raw:
            assert -s <= x < unit[i] + s, (what, i, x)
        else:
            assert -(unit[i] >> 1) - s <= x <= (unit[i] >> 1) + s, (what, i, x)


def check_fe_limbs(out):
    """products, squarings, fe_carry and fe_tobytes of the 9-limb form against Python integers; the limb ranges of every result: raw in
    [0, 1), centred in [-1/2, 1/2], limb 1 with the wrap's last carry (|.| < 2^17 after a product; at most 1 after fe_carry, whose
    wrap brings 19 * (a carry below 2^9) to a centred limb 0) on top"""
    cases = [(f, squaring_operand(f), g, 7) for f, g in product_cases()] + [(v, [0] * 9, [0] * 9, 4) for v in encoding_limb_cases()]
    assert len(out) == len(cases) and len(cases) >= 428 + 20
    for (f, fs, g, which), o in zip(cases, out):
        lim = [[s32(x) for x in o[9 * k:9 * k + 9]] for k in range(5)]
        byt = [_int(o[45 + 8 * k:53 + 8 * k]) for k in range(6)]
        if which & 1:
            want = limbs_value(f) * limbs_value(g) % P
            assert byt[0] == want and byt[1] == want, (f, g)
            assert limbs_value(lim[0]) % P == want and limbs_value(lim[1]) % P == want, (f, g)
            _in_ranges(lim[0], False, 1 << 17, UNIT, "fe_mul")
            _in_ranges(lim[1], True, 1 << 17, UNIT, "fe_mul_raw")
        if which & 2:
            want = limbs_value(fs) ** 2 % P
            assert byt[2] == want and byt[3] == want, fs
            assert limbs_value(lim[2]) % P == want and limbs_value(lim[3]) % P == want, fs
            _in_ranges(lim[2], False, 1 << 17, UNIT, "fe_sq")
            _in_ranges(lim[3], True, 1 << 17, UNIT, "fe_sq_raw")
            assert byt[5] == limbs_value(fs) % P, fs
        if which & 4:
            assert byt[4] == limbs_value(f) % P and byt[4] < P, f
            assert limbs_value(lim[4]) % P == byt[4], f
            _in_ranges(lim[4], False, 1, UNIT, "fe_carry")
        if not which & 1:
            assert not any(o[:36]) and not any(o[45:77]) and not any(o[85:]), f


def check_fe10_limbs(out):
    """fe10_mul_raw, fe10_sq_raw, fe10_carry, fe10_tobytes against Python integers, and the closure the header states: a raw result of
    in-range operands is in range again - limbs in [0, 2^26) / [0, 2^25), limb 1 at most FE10_WRAP_CARRY more - so it is valid as
    either operand of a product and as the input of a squaring.  (The checker works on magnitudes, which grow with every limb: the
    operand with every limb at the top of that range passes it in the list's first pairs, so every operand within the range does.)"""
    unit = [1 << b for b in FE10_BITS]
    cases = fe10_limb_cases()
    assert len(out) == len(cases) and sum(1 for c in cases if c[2] & 1) >= 28 * 28 + 200
    for (f, g, which), o in zip(cases, out):
        lim = [[s32(x) for x in o[10 * k:10 * k + 10]] for k in range(3)]
        byt = [_int(o[30 + 8 * k:38 + 8 * k]) for k in range(3)]
        vf, vg = limbs10_value(f), limbs10_value(g)
        if which & 1:
            assert all(0 <= x <= r for x, r in zip(f, FE10_RANGE)) and all(0 <= x <= r for x, r in zip(g, FE10_RANGE))
            assert byt[0] == vf * vg % P and limbs10_value(lim[0]) % P == byt[0], (f, g)
            assert byt[1] == vf * vf % P and limbs10_value(lim[1]) % P == byt[1], f
            for r in lim[:2]:
                assert all(0 <= x <= hi for x, hi in zip(r, FE10_RANGE)), (f, g, r)
        else:
            assert not any(o[:20]) and not any(o[30:46])
        if which & 4:
            assert byt[2] == vf % P and byt[2] < P, f
            assert limbs10_value(lim[2]) % P == byt[2], f
            _in_ranges(lim[2], False, 1, unit, "fe10_carry")


def check_fe_bytes(out):
    cases = fe_bytes_cases()
    assert len(out) == len(cases)
    for (a, b), o in zip(cases, out):
        x, y = int.from_bytes(a, "little") % 2 ** 255, int.from_bytes(b, "little") % 2 ** 255
        got = [_int(o[8 * k:8 * k + 8]) for k in range(5)]
        assert got[0] == x * y % P and got[1] == x * x % P, (a.hex(), b.hex())
        assert got[2] == pow(x, P - 2, P) and got[3] == pow(x, (P - 5) // 8, P), a.hex()
        assert got[4] == x % P, a.hex()


def check_sqrt_ratio(out):
    """the flag and the non-negative root of RFC 9496's SQRT_RATIO_M1; the case list reaches all four outcomes"""
    from tests.pyref import ristretto as R
    cases = sqrt_ratio_cases()
    assert len(out) == len(cases)
    seen = set()
    for (u, v), o in zip(cases, out):
        ok, r = R.sqrt_ratio_m1(u, v)
        assert (o[0], _int(o[1:9])) == (1 if ok else 0, r), (u, v)
        seen.add((ok, r != 0))
        if ok:
            assert v * r * r % P == u % P
        elif u % P and v % P:
            assert v * r * r % P == R.SQRT_M1 * u % P
        assert r & 1 == 0
    # square with a root, non-square with the root of i * u / v, u = 0 (square, 0), v = 0 (not square, 0)
    assert seen == {(True, True), (False, True), (True, False), (False, False)}, seen


def check_elligator(out):
    from tests.pyref import ristretto as R
    cases = elligator_cases()
    assert len(out) == len(cases)
    for r0, o in zip(cases, out):
        want = R.encode(R._elligator((int.from_bytes(r0, "little") & (2 ** 255 - 1)) % P))
        assert unwords(o) == want, r0.hex()


def check_decode_encode(out):
    from tests.pyref import ristretto as R
    cases = decode_encode_cases()
    assert len(out) == len(cases)
    valid = 0
    for e, o in zip(cases, out):
        pt = R.decode(e)
        assert o[0] == (0 if pt is None else 1), e.hex()
        assert unwords(o[1:]) == (bytes(32) if pt is None else R.encode(pt)), e.hex()
        if pt is not None:
            assert unwords(o[1:]) == e
            valid += 1
    assert 16 <= valid < len(cases)


def check_point_ops(out):
    """the point formulas at their exceptional inputs against the oracle's point_add / point_sub"""
    import oracle
    cases = point_ops_cases()
    assert len(out) == len(cases) == 20
    ident = bytes(32)
    for (p, q), o in zip(cases, out):
        assert o[0] == 1
        got = [unwords(o[1 + 8 * k:9 + 8 * k]) for k in range(15)]
        dbl, neg = oracle.point_add(p, p), oracle.point_sub(ident, p)
        want = [oracle.point_add(p, q), oracle.point_sub(p, q), dbl, dbl, ident, p, p, ident, ident, p, p, oracle.point_add(p, q),
                oracle.point_sub(p, q), ident, neg]
        assert got == want, (p.hex(), q.hex(), [k for k in range(15) if got[k] != want[k]])
        assert oracle.point_add(p, ident) == p and oracle.point_sub(p, p) == ident and dbl != ident


def check_scalar(out):
    cases = scalar_cases()
    assert len(out) == len(cases)
    reached = set()
    for (w, a, x, b, c), o in zip(cases, out):
        got = [_int(o[8 * k:8 * k + 8]) for k in range(5)]
        assert got[0] == w % L, hex(w)
        acc = reduce512_acc(w)
        assert 0 <= acc < 4 * L and acc % L == w % L, hex(w)          # sc.cuh: "acc < 4l", and never negative
        reached.add(acc // L)
        assert got[1] == (x * b + c) % L, (x, b, c)
        assert got[2] == (-x) % L and got[4] == 2 * x % L, x
        assert got[3] < L and got[3] * 2 % L == x, x
        assert o[40] == (1 if a < L else 0), hex(a)
    assert reached == {0, 1, 2, 3}, reached          # every number of trailing subtractions the running value can need


def check(kind, out):
    assert all(len(o) == KINDS[kind][1] for o in out)
    globals()["check_" + kind](out)


def run(fn, rows_in, n_out):
    """one call of a library's entry point (in words, out words, n) over the rows; returns (what it returned, the rows out)"""
    n, n_in = len(rows_in), len(rows_in[0])
    flat = (C.c_uint32 * (n * n_in))(*[x for r in rows_in for x in r])
    out = (C.c_uint32 * (n * n_out))()
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    fn.restype = C.c_int
    rc = fn(flat, out, n)
    o = list(out)
    return rc, [o[i * n_out:(i + 1) * n_out] for i in range(n)]


# ---- the two builds ----

def build_host_lib(outdir):
    """tests/hostsim/arith_host.cpp by g++: the headers' host build, every product under the bounds checker"""
    out = os.path.join(str(outdir), "libarith_host.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out,
           os.path.join(ROOT, "tests", "hostsim", "arith_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(out)
    lib.arith_bounds_violations.restype = C.c_uint64
    lib.arith_last_violation.restype = C.c_char_p
    return lib


def device_compile_command(out):
    """tests/gpu_arith/arith_device.hip with the compiler and the device flags of the product Makefile's build/kernels.o rule, read
    from the Makefile so that the two cannot drift, as a shared library"""
    csrc = os.path.join(ROOT, "aeonflux_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        mk = f.read()
    var = {k: os.environ.get(k, v.strip()) for k, v in re.findall(r"^(HIPCC|ARCH)\s*\?=\s*(.+)$", mk, re.M)}
    assert set(var) == {"HIPCC", "ARCH"}, var
    rule = re.search(r"^build/kernels\.o:.*\n(?:\t.*\n)*?\t(\$\(HIPCC\).*)$", mk, re.M)
    assert rule, "no compile line under build/kernels.o"
    tok = rule.group(1).replace("$(HIPCC)", var["HIPCC"]).replace("$(ARCH)", var["ARCH"]).split()
    assert tok[-4:] == ["-c", "kernels.hip", "-o", "$@"], tok
    flags = tok[1:-4]
    assert "-O3" in flags and any(x.startswith("--offload-arch=") for x in flags), flags
    return [tok[0]] + flags + ["-shared", "-fPIC"] + ["-o", str(out), os.path.join(ROOT, "tests", "gpu_arith", "arith_device.hip")]


def build_device_lib(outdir, load=True):
    """compile the device harness; a failed compile is an error.  Returns (library or None, seconds the compile took)"""
    import time
    out = os.path.join(str(outdir), "libarith_device.so")
    t0 = time.time()
    r = subprocess.run(device_compile_command(out), capture_output=True, text=True, timeout=900)
    took = time.time() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    return (C.CDLL(out) if load else None), took
