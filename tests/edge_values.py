"""Named edge values for the multiscalar paths: scalars, extreme-digit scalars for every window width the kernels recode to, issuer
keys of chosen width-5 NAF weight, and points.  Pure Python (the points take the oracle as an argument), shared by the host recoding
tests (tests/test_device_arith_on_host.py) and the GPU parity module (tests/test_gpu_edge_scalars.py).

The widths: 2 bits (secret scalars on variable bases, plan.h AFX_SECVAR_BITS), 4 bits (per-item scalars on variable bases,
kernels.hip msm_add_var), 6 bits (secret scalars on generators, AFX_SEC_BITS), 13 bits (public scalars on generators,
AFX_POS_BITS).  Every value here is canonical (in [0, L)) unless its name says otherwise."""
L = 2 ** 252 + 27742317777372353535851937790883648493
WIDTHS = (2, 4, 6, 13)

SCALARS = {
    "0": 0, "1": 1, "2": 2, "3": 3, "8": 8, "15": 15, "16": 16, "2^128": 2 ** 128,
    "2^251-1": 2 ** 251 - 1, "2^251": 2 ** 251, "2^252-1": 2 ** 252 - 1, "2^252": 2 ** 252, "2^252+1": 2 ** 252 + 1,
    "L-16": L - 16, "L-9": L - 9, "L-3": L - 3, "L-2": L - 2, "L-1": L - 1,
    "(L-1)/2": (L - 1) // 2, "(L+1)/2": (L + 1) // 2, "(L+3)/2": (L + 3) // 2,
}
# non-canonical scalars: the engine must flag them (ok = 0) and leave the other lanes alone
NON_CANONICAL = {"L": L, "L+1": L + 1, "2^253": 2 ** 253, "2^255-1": 2 ** 255 - 1}


def _from_digits(digits, B, top):
    """sum d_j 2^(B j) for the low windows, plus a small positive top digit in the next window"""
    return sum(d << (B * j) for j, d in enumerate(digits)) + (top << (B * len(digits)))


def extreme_digit_scalars(B):
    """scalars whose low windows (width B) hold the extreme signed digits: all -2^(B-1), all 2^(B-1)-1, alternating, and
    the extremes with zeros between.  The low windows stop below bit 248, the top digit is 1 or 3: every value lies in [0, L)."""
    lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
    k = (248 // B) - 1
    out = {}
    for top in (1, 3):
        pats = {
            "min": [lo] * k, "max": [hi] * k,
            "alt": [lo if j % 2 == 0 else hi for j in range(k)],
            "alt'": [hi if j % 2 == 0 else lo for j in range(k)],
            "min0max0": [(lo, 0, hi, 0)[j % 4] for j in range(k)],
        }
        for name, digits in pats.items():
            s = _from_digits(digits, B, top)
            assert 0 <= s < L, (B, name)
            out["w%d %s top%d" % (B, name, top)] = s
    return out


def naf5(k):
    """width-5 NAF of a non-negative integer, lowest digit first: digits in {0, +-1, +-3, ..., +-15}, at most one nonzero digit
    in any 5 consecutive positions (the restatement of the engine's host NAF, used to reason about coverage)"""
    out = []
    while k:
        if k & 1:
            d = k & 31
            if d >= 16:
                d -= 32
            k -= d
        else:
            d = 0
        out.append(d)
        k >>= 1
    return out


def naf_weight(k):
    return sum(1 for d in naf5(k) if d)


def _max_weight_naf_scalar():
    """digits -15 / +15 alternating, one every 5 bits from bit 0 up to bit 245, and +1 at bit 250: 51 nonzero digits, the most a
    scalar below L can carry (positions 0 .. 252, at least 5 apart)"""
    digits = [(-15 if (j % 2 == 0) else 15) for j in range(50)] + [1]
    return sum(d << (5 * j) for j, d in enumerate(digits))


NAF_MAX = _max_weight_naf_scalar()
assert 0 < NAF_MAX < L and naf_weight(NAF_MAX) == 51
NAF_MAX_NEG = L - NAF_MAX   # its negation mod l: what a negated key term recodes


def all_scalars():
    """every named canonical scalar: the plain edge values and the extreme-digit ones of each width"""
    out = dict(SCALARS)
    for B in WIDTHS:
        out.update(extreme_digit_scalars(B))
    out["naf-max"] = NAF_MAX
    out["naf-max-neg"] = NAF_MAX_NEG
    return out


def b32(v):
    return int(v).to_bytes(32, "little")


def key_draws(scalars):
    """the draws oracle.issuer_new reads for a key whose scalars are exactly `scalars` (w, w', x0, x1, y_0 ...): each draw is
    s || 0^32, which reduces mod l to s itself (oracle/aeonflux.c afxo_issuer_new)"""
    for s in scalars:
        assert 0 <= s < L
    return b"".join(b32(s) + bytes(32) for s in scalars)


def edge_key(n, which=0):
    """key scalars (w, w', x0, x1, y_0 .. y_{n-1}) for n attributes.  Key 0 holds the NAF weights 0 (x0 = 0), 1 (x1 = 1) and the
    maximum (y_1, and its negation y_2: attributes 1 and 2 are points in the GPU tests' layout, so these key terms sit on variable
    bases in issue's V as well as in verify's Z), key 1 the other extremes (w = 0, a maximum-weight x0, x1 = L - 1, halves of l)."""
    if which == 0:
        base = [2 ** 252, L - 1, 0, 1] + [(L - 1) // 2, NAF_MAX, NAF_MAX_NEG, 3, L - 16, 2 ** 128, 2 ** 251 - 1]
    else:
        base = [0, 1, NAF_MAX, L - 1] + [(L + 1) // 2, 0, NAF_MAX_NEG, 2 ** 252 - 1, 16, L - 2]
    ys = base[4:]
    return base[:4] + [ys[i % len(ys)] for i in range(n)]


def edge_points(oracle, primitives):
    """named points: the identity, B, -B, the RFC 9496 generator multiples (primitives["base_multiples"]) and a hashed point"""
    B = oracle.basepoint()
    out = {"identity": bytes(32), "B": B, "-B": oracle.point_sub(bytes(32), B), "hashed": oracle.point_from_uniform(b"\x5a" * 64)}
    for k, enc in enumerate(primitives["base_multiples"]):
        out["%dB" % k] = bytes.fromhex(enc)
    return out
