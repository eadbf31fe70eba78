"""CPU-only: the engine's DEVICE arithmetic headers (aeonflux_amd/csrc/fe.cuh, sc.cuh, ge.cuh) compiled for the host
(tests/hostsim/arith_host.cpp) and compared with the oracle and with Python integers.  This is the arithmetic the
kernels run, statement for statement, so a slip in a carry chain or a bound shows up here without a GPU.  The same
build measures the field-operation counts that DESIGN.md section 3 publishes."""
import ctypes as C
import hashlib
import os

import pytest

from tests import arith_cases
from tests.arith_cases import L, P, ROOT, stream


@pytest.fixture(scope="module")
def arith(tmp_path_factory):
    return arith_cases.build_host_lib(tmp_path_factory.mktemp("arith"))


def test_field_ops_against_python_integers(arith):
    cases = arith_cases.field_byte_cases()
    assert len(cases) == 400 + 64
    out = ((C.c_uint8 * 32) * 4)()
    for a, b in cases:
        arith.arith_fe(out, a, b)
        x, y = int.from_bytes(a, "little") % 2 ** 255, int.from_bytes(b, "little") % 2 ** 255
        got = [int.from_bytes(bytes(o), "little") for o in out]
        assert got[0] == x * y % P and got[1] == x * x % P
        assert got[2] == pow(x, P - 2, P) and got[3] == pow(x, (P - 5) // 8, P)


def test_lazily_added_operands_at_the_documented_bounds(arith):
    s = stream(b"fe-lazy", 192 * 300)
    big = (2 ** 255 - 20).to_bytes(32, "little")
    cases = [[s[192 * i + 32 * k:192 * i + 32 * k + 32] for k in range(6)] for i in range(300)] + [[big] * 4 + [big, bytes(32)], [big] * 4 + [bytes(32), big]]
    out = ((C.c_uint8 * 32) * 2)()
    for c in cases:
        a = ((C.c_uint8 * 32) * 4)(*[(C.c_uint8 * 32)(*x) for x in c[:4]])
        b = ((C.c_uint8 * 32) * 2)(*[(C.c_uint8 * 32)(*x) for x in c[4:]])
        arith.arith_fe_lazy(out, a, b)
        v = [int.from_bytes(x, "little") % 2 ** 255 for x in c]
        assert int.from_bytes(bytes(out[0]), "little") == (v[0] + v[1] + v[2] + v[3]) * (v[4] - v[5]) % P
        assert int.from_bytes(bytes(out[1]), "little") == (v[0] - v[1]) ** 2 % P


_limbs_value = arith_cases.limbs_value


def test_products_at_the_limits_of_the_bounds_discipline(arith):
    """fe.cuh: a product needs |f| * |g| <= 3.8 units (1 unit = 2^29; limb 8: 2^23), a squaring |f| <= 1.9.  Operands with every limb at
    the extreme of its range, all sign patterns that maximise a column, must come out right and must not trip the checker."""
    unit = arith_cases.UNIT
    out = ((C.c_uint8 * 32) * 5)()
    raw, cen = (C.c_int32 * 9)(), (C.c_int32 * 9)()
    before = arith.arith_bounds_violations()
    cases = arith_cases.product_cases()           # shared with the device build: tests/test_gpu_device_arith.py
    assert len(cases) == 428
    for f, g in cases:
        fs = arith_cases.squaring_operand(f)      # the squaring takes |f| <= 1.9
        arith.arith_fe_limbs(out, (C.c_int32 * 9)(*fs), (C.c_int32 * 9)(*g), 2 | 4)
        vs = _limbs_value(fs)
        assert int.from_bytes(bytes(out[2]), "little") == vs * vs % P and bytes(out[3]) == bytes(out[2])
        assert int.from_bytes(bytes(out[4]), "little") == vs % P
        arith.arith_fe_limbs(out, (C.c_int32 * 9)(*f), (C.c_int32 * 9)(*g), 1)
        want = _limbs_value(f) * _limbs_value(g) % P
        assert int.from_bytes(bytes(out[0]), "little") == want and int.from_bytes(bytes(out[1]), "little") == want
        # ranges of the results: raw in [0, 1), centred in [-1/2, 1/2]; limb 1 takes the wrap's last carry (|.| < 2^15) on top
        arith.arith_fe_mul_limbs(raw, cen, (C.c_int32 * 9)(*f), (C.c_int32 * 9)(*g))
        for i in range(9):
            slack = (1 << 17) if i == 1 else 0
            assert -slack <= raw[i] < unit[i] + slack, (i, raw[i])
            assert -(unit[i] >> 1) - slack <= cen[i] <= (unit[i] >> 1) + slack, (i, cen[i])
    assert arith.arith_bounds_violations() == before, arith.arith_last_violation()


def test_canonical_encoding_of_edge_values(arith):
    """fe_tobytes on limb patterns around 0, p and 2^255, positive and negative, lazily added, up to the int32 range"""
    out = ((C.c_uint8 * 32) * 5)()
    vals = arith_cases.encoding_limb_cases()
    assert len(vals) == 20
    zero = (C.c_int32 * 9)(*([0] * 9))
    for v in vals:
        arith.arith_fe_limbs(out, (C.c_int32 * 9)(*v), zero, 4)
        got = int.from_bytes(bytes(out[4]), "little")
        assert got == _limbs_value(v) % P and got < P, v


def test_group_ops_against_the_oracle(arith, primitives):
    import oracle
    s = stream(b"ge-host", 64 * 3 * 40)
    o = [(C.c_uint8 * 32)() for _ in range(4)]
    for i in range(40):
        p = oracle.point_from_uniform(s[192 * i:192 * i + 64])
        q = oracle.point_from_uniform(s[192 * i + 64:192 * i + 128])
        k = oracle.scalar_reduce_wide(s[192 * i + 128:192 * i + 192])
        assert arith.arith_point_ops(o[0], o[1], o[2], o[3], k, p, q) == 1
        assert bytes(o[0]) == oracle.point_scalarmult(k, p)
        assert bytes(o[1]) == oracle.point_add(p, q) and bytes(o[2]) == oracle.point_sub(p, q)
        assert bytes(o[3]) == oracle.point_add(p, p)
        arith.arith_from_uniform(o[0], s[192 * i:192 * i + 64])
        assert bytes(o[0]) == p
    # committed fixtures (libsodium / RFC 9496): generator multiples round-trip, invalid encodings are refused,
    # hash-to-group and scalar multiplication vectors
    for enc in primitives["base_multiples"]:
        assert arith.arith_decode_encode(o[0], bytes.fromhex(enc)) == 1 and bytes(o[0]).hex() == enc
    for v in primitives["validity"]:
        assert arith.arith_decode_encode(o[0], bytes.fromhex(v["in"])) == (1 if v["valid"] else 0), v["in"]
    for v in primitives["from_uniform"]:
        arith.arith_from_uniform(o[0], bytes.fromhex(v["in"]))
        assert bytes(o[0]).hex() == v["out"]
    for v in primitives["scalarmult"]:
        p = bytes.fromhex(v["p"])
        assert arith.arith_point_ops(o[0], o[1], o[2], o[3], bytes.fromhex(v["s"]), p, p) == 1 and bytes(o[0]).hex() == v["out"]


def test_scalar_ops_against_python_integers(arith):
    s = stream(b"sc-host", 160 * 300)
    red, ma, ng = ((C.c_uint8 * 32)() for _ in range(3))
    can = C.c_int(0)
    edge = [(L - 1).to_bytes(32, "little"), L.to_bytes(32, "little"), bytes(32), b"\xff" * 32]
    for i in range(300):
        wide = s[160 * i:160 * i + 64]
        a, b, c = (s[160 * i + 64 + 32 * k:160 * i + 96 + 32 * k] for k in range(3))
        if i < 4:
            a = edge[i]
            wide = b"\xff" * 64 if i == 0 else wide
        ai = int.from_bytes(a, "little")
        # sc_muladd / sc_neg take canonical inputs (the kernels check canonicity first); reduce them here
        a_r, b_r, c_r = ((int.from_bytes(x, "little") % L).to_bytes(32, "little") for x in (a, b, c))
        arith.arith_sc(red, ma, ng, C.byref(can), wide, a_r, b_r, c_r)
        assert int.from_bytes(bytes(red), "little") == int.from_bytes(wide, "little") % L
        av, bv, cv = (int.from_bytes(x, "little") for x in (a_r, b_r, c_r))
        assert int.from_bytes(bytes(ma), "little") == (av * bv + cv) % L
        assert int.from_bytes(bytes(ng), "little") == (-av) % L
        arith.arith_sc(red, ma, ng, C.byref(can), wide, a, b_r, c_r)
        assert can.value == (1 if ai < L else 0)
        half, dbl = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        arith.arith_sc_half_dbl(half, dbl, a_r)
        assert int.from_bytes(bytes(half), "little") * 2 % L == av and int.from_bytes(bytes(half), "little") < L
        assert int.from_bytes(bytes(dbl), "little") == 2 * av % L


def test_msm_chain_with_consumer_aware_conversions(arith):
    """k_msm's chain, step for step (raw / centred conversions chosen by what consumes them), against the oracle's
    multiscalar multiplication; every fe_mul / fe_sq of the host build asserts its operand bounds on the way"""
    import oracle
    s = stream(b"chain-host", 64 * 12 * 12)
    out = (C.c_uint8 * 32)()
    pos = 0
    for case in range(12):
        nv, nf = 1 + case % 6, case % 3
        pts = [oracle.point_from_uniform(s[pos + 64 * i:pos + 64 * i + 64]) for i in range(nv + nf)]
        pos += 64 * (nv + nf)
        scs = [oracle.scalar_reduce_wide(hashlib.sha512(b"k%d-%d" % (case, i)).digest()) for i in range(nv + nf)]
        if case == 3:
            scs[0] = bytes(32)                                          # all-zero digits: identity entries only
        if case == 4:
            scs[0] = (L - 1).to_bytes(32, "little")
        if case == 5:
            pts[0] = bytes(32)                                          # the identity as a base
        assert arith.arith_msm_chain(out, nv, b"".join(scs[:nv]), b"".join(pts[:nv]), nf, b"".join(scs[nv:]), b"".join(pts[nv:])) == 1
        assert bytes(out) == oracle.multiscalar(scs, pts), case
    assert arith.arith_bounds_violations() == 0, arith.arith_last_violation()


def test_double_and_compress_against_the_oracle(arith):
    """ge.cuh c2x_from / c2x_finish (k_compress2x): the encodings of 2P for a batch of points with one inversion equal the
    oracle's encode(P + P) - identities in the batch included - with every multiplication's operand bounds checked"""
    import ctypes as C
    import hashlib
    import oracle
    rnd = hashlib.shake_256(b"c2x-host").digest(64 * 40)
    pts = [oracle.point_from_uniform(rnd[64 * i:64 * i + 64]) for i in range(39)]
    pts.insert(7, bytes(32))                     # the identity in the middle of the batch
    pts.insert(20, bytes(32))
    shift = oracle.point_from_uniform(hashlib.sha512(b"c2x-shift").digest())
    out = C.create_string_buffer(32 * len(pts))
    arith.arith_double_and_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p]
    assert arith.arith_double_and_compress(out, len(pts), b"".join(pts), shift) == 1
    for j, p in enumerate(pts):
        assert out.raw[32 * j:32 * j + 32] == oracle.point_add(p, p), j
    assert out.raw[32 * 7:32 * 8] == bytes(32)


def test_negate_and_encode_against_the_oracle(arith, primitives):
    """ge.cuh negenc_den / negenc_finish (k_negenc): the encodings of -P for a batch of DECODED points with one inversion and no
    square root equal the oracle's encode(identity - P) - random points, small multiples of the base point, the libsodium-valid
    encodings of the golden file (both parities of every decision inside Encode occur), the identity in the batch - with every
    multiplication's operand bounds checked"""
    import ctypes as C
    import hashlib
    import oracle
    rnd = hashlib.shake_256(b"negenc-host").digest(64 * 30)
    pts = [oracle.point_from_uniform(rnd[64 * i:64 * i + 64]) for i in range(30)]
    pts += [bytes.fromhex(x) for x in primitives["base_multiples"][1:]]
    pts += [bytes.fromhex(v["in"]) for v in primitives["validity"] if v["valid"]][:16]
    pts.insert(5, bytes(32))                      # the identity in the middle of the batch
    arith.arith_negate_and_encode.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
    seen = set()
    for lo in range(0, len(pts), 60):
        chunk = pts[lo:lo + 60]
        out = C.create_string_buffer(32 * len(chunk))
        assert arith.arith_negate_and_encode(out, len(chunk), b"".join(chunk)) == 1
        for j, p in enumerate(chunk):
            want = oracle.point_sub(bytes(32), p)
            assert out.raw[32 * j:32 * j + 32] == want, (lo + j, p.hex())
            seen.add(want == p)
    assert seen == {True, False} or len(pts) > 40   # 2-torsion-like fixed points are rare; most negations differ


@pytest.mark.parametrize("kind", list(arith_cases.KINDS))
def test_shared_limit_cases_on_the_host_build(arith, kind):
    """the case list of tests/arith_cases.py - what tests/test_gpu_device_arith.py runs one lane each on the device build - through the
    same case bodies (tests/gpu_arith/arith_cases.cuh) on this build: every result against Python integers, pyref or the oracle, the
    limb ranges and the fe10 closure (arith_cases.check_*), and not one operand beyond the bounds discipline"""
    got = (C.c_uint32 * 16)()
    arith.arith_host_words(got)
    assert list(got) == [x for k in arith_cases.KINDS.values() for x in k]
    before = arith.arith_bounds_violations()
    _, out = arith_cases.run(getattr(arith, "arith_host_" + kind), arith_cases.rows(kind), arith_cases.KINDS[kind][1])
    arith_cases.check(kind, out)
    assert arith.arith_bounds_violations() == before, arith.arith_last_violation()


def test_device_harness_cross_compiles(tmp_path):
    """tests/gpu_arith/arith_device.hip builds for gfx950 with the flags of the product's kernels.o (no GPU needed): the harness of
    tests/test_gpu_device_arith.py cannot rot between GPU visits"""
    cmd = arith_cases.device_compile_command(tmp_path / "libarith_device.so")
    assert "-O3" in cmd and "--offload-arch=gfx950" in cmd and "-shared" in cmd
    arith_cases.build_device_lib(tmp_path, load=False)
    assert os.path.getsize(tmp_path / "libarith_device.so") > 0


def test_the_bounds_checker_fires(arith):
    arith.arith_bounds_checker_selftest.restype = C.c_uint64
    assert arith.arith_bounds_checker_selftest() >= 2
    # fe10.cuh's checker: an operand of 2^28 per limb trips it in the product and in the squaring, and the count is put back
    arith.arith_bounds_checker_selftest10.restype = C.c_uint64
    before = arith.arith_bounds_violations()
    assert arith.arith_bounds_checker_selftest10() >= 2
    assert arith.arith_bounds_violations() == before


def test_no_bound_was_violated_anywhere(arith):
    """runs last in this module: all the field operations of the tests above stayed within their operand bounds"""
    arith.arith_bounds_violations.restype = C.c_uint64
    arith.arith_last_violation.restype = C.c_char_p
    assert arith.arith_bounds_violations() == 0, arith.arith_last_violation()


def test_signed_digit_recoding(arith):
    """k_msm's carry-free recoding: the digits of s + bias minus the per-digit offset sum back to s"""
    s = stream(b"digits", 32 * 100)
    out = (C.c_uint32 * 8)()
    for i in range(100):
        k = int.from_bytes(s[32 * i:32 * i + 32], "little") % L
        kb = k.to_bytes(32, "little")
        arith.arith_sc_bias(out, kb, 0x88888888)
        v = sum(int(out[j]) << (32 * j) for j in range(8))
        assert sum((((v >> (4 * j)) & 15) - 8) << (4 * j) for j in range(64)) == k
        arith.arith_sc_bias(out, kb, 0x80808080)
        v = sum(int(out[j]) << (32 * j) for j in range(8))
        assert sum((((v >> (8 * j)) & 255) - 128) << (8 * j) for j in range(32)) == k


def _recoding_constants(arith):
    c = (C.c_int32 * 11)()
    arith.arith_recoding_constants(c)
    c = list(c)
    # width -> (windows, largest digit magnitude the stored table serves); 4 bits: sc_bias fills 8 words of 4-bit windows and
    # msm_add_var reads multiples 1 .. AFX_TABLE_STORED
    return {c[0]: (c[1], c[2]), c[3]: (c[4], c[5] - 1), c[6]: (c[7], c[8] - 1), 4: (8 * 32 // 4, c[10])}, c[9]


def _recode(arith, B, s, words):
    """the digit words msm_recode writes for scalar s at width B"""
    if B == 4:
        out = (C.c_uint32 * 8)()
        arith.arith_sc_bias(out, s.to_bytes(32, "little"), 0x88888888)
        return list(out) + [0]
    out = (C.c_uint32 * words)()
    assert arith.arith_sc_bias_wide(out, s.to_bytes(32, "little"), B) == 1
    return list(out)


def _kernel_digits(B, windows, words, w):
    """the digits as the kernels read them: one word, or two when the window straddles a word boundary (kernels.hip
    msm_add_positional / msm_add_positional_secret / narrow_fetch; msm_add_var's 4-bit windows never straddle)"""
    out = []
    for j in range(windows):
        o = B * j
        k, sh = o >> 5, o & 31
        assert k < words, (B, j)
        x = w[k]
        if sh + B > 32:
            assert k + 1 < words, ("two-word read past the digit words", B, j)
            x |= w[k + 1] << 32
        out.append(((x >> sh) & ((1 << B) - 1)) - (1 << (B - 1)))
    return out


def _recoding_inputs(arith):
    from tests.edge_values import all_scalars
    edge = list(all_scalars().values())
    half, dbl = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
    derived = []
    for s in edge:
        arith.arith_sc_half_dbl(half, dbl, s.to_bytes(32, "little"))   # the scalars of halved jobs and of dbl terms
        derived += [int.from_bytes(bytes(half), "little"), int.from_bytes(bytes(dbl), "little")]
    r = stream(b"recoding-wide", 64 * 300)
    rand = [int.from_bytes(r[64 * i:64 * i + 64], "little") % L for i in range(300)]
    return edge, edge + derived + rand


def test_every_recoding_width_sums_back_within_its_table(arith):
    """msm_recode at every width the kernels use - 2 (AFX_SECVAR_BITS), 4, 6 (AFX_SEC_BITS), 13 (AFX_POS_BITS) - on the named edge
    scalars, their halves and doubles (sc_half / sc_dbl, as msm_recode applies them) and 300 random ones: the digits, read as the
    kernels read them, sum back to s; each lies in [-2^(B-1), 2^(B-1) - 1], so its entry index is at most the table's last
    entry; no bit is set at or above B * WINDOWS; every two-word read stays inside AFX_DIGIT_WORDS"""
    consts, words = _recoding_constants(arith)
    assert sorted(consts) == [2, 4, 6, 13] and words == 9
    _, scalars = _recoding_inputs(arith)
    assert len(scalars) > 450
    for B, (windows, stored) in consts.items():
        lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
        assert stored == 1 << (B - 1), (B, stored)          # digit -2^(B-1) reads the last stored multiple
        assert B * windows <= 32 * words
        bias = sum(1 << (B * j + B - 1) for j in range(windows))
        for s in scalars:
            assert 0 <= s < L
            w = _recode(arith, B, s, words)
            v = sum(x << (32 * i) for i, x in enumerate(w))
            assert v == s + bias, (B, s)                     # no carry lost off the top word
            assert v >> (B * windows) == 0, (B, s)
            d = _kernel_digits(B, windows, words, w)
            assert sum(x << (B * j) for j, x in enumerate(d)) == s, (B, s)
            assert all(lo <= x <= hi and abs(x) <= stored for x in d), (B, s)
    assert arith.arith_bounds_violations() == 0, arith.arith_last_violation()


def test_edge_list_reaches_every_extreme_digit(arith):
    """coverage of the named edge values: at each width, window 0 and a middle window see the digits -2^(B-1), 0 and
    2^(B-1) - 1, and the top window its largest reachable digit (that of L - 1: the top digit does not decrease with s).  The
    issuer keys of tests/edge_values.py have width-5 NAF weights 0, 1 and the maximum, 51."""
    from tests.edge_values import NAF_MAX, edge_key, naf5, naf_weight
    consts, words = _recoding_constants(arith)
    edge, _ = _recoding_inputs(arith)
    for B, (windows, _) in consts.items():
        lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
        digits = [_kernel_digits(B, windows, words, _recode(arith, B, s, words)) for s in edge]
        mid = windows // 2
        for j in (0, mid):
            seen = {d[j] for d in digits}
            assert {lo, 0, hi} <= seen, (B, j, sorted(seen))
        top = _kernel_digits(B, windows, words, _recode(arith, B, L - 1, words))[-1]
        assert top == max(d[-1] for d in digits), B
        assert top >= 0 and any(d[-1] == top for d in digits)
    key_weights = {naf_weight(s) for which in (0, 1) for s in edge_key(8, which)}
    assert {0, 1, 51} <= key_weights, sorted(key_weights)
    d = naf5(NAF_MAX)
    assert set(x for x in d if x) == {-15, 15, 1} and all(d[i] == 0 for i in range(len(d)) if i % 5)
    for s in edge + [NAF_MAX]:       # the restatement itself: digits sum back, odd, at most one nonzero in any 5 positions
        d = naf5(s)
        assert sum(x << i for i, x in enumerate(d)) == s
        nz = [i for i, x in enumerate(d) if x]
        assert all(d[i] % 2 and -15 <= d[i] <= 15 for i in nz) and all(b - a >= 5 for a, b in zip(nz, nz[1:]))


# field multiplications / squarings per building block: the constants behind afx_plan_stats.field_mul / field_sq
# (aeonflux_amd/csrc/engine.cpp Assembler::msm, plan.h AFX_DECODE_* / AFX_ENCODE_*) and DESIGN.md section 3
OP_COUNTS = {"decode": (27, 257), "encode": (32, 255), "double_to_p2": (3, 4), "double_to_p3": (4, 4), "table_entry": (1, 0),
             "add_var_to_p3": (8, 0), "add_fixed_to_p3": (7, 0), "add_var_to_p2": (7, 0)}


def test_chain_operations_are_the_published_share(arith):
    """the inversion / square-root chains run in the 10-limb form (fe10.cuh): 251 squarings + 11 products of a decode or an
    encode, 254 + 11 of a plain inversion - plan.h AFX_CHAIN_*, what afx_plan_stats.chain_mul / chain_sq count"""
    out = ((C.c_uint64 * 2) * 3)()
    arith.arith_chain_op_counts(out)
    assert [(int(r[0]), int(r[1])) for r in out] == [(11, 251), (11, 251), (11, 254)]


def test_operation_counts_are_the_published_ones(arith):
    out = ((C.c_uint64 * 2) * 8)()
    arith.arith_op_counts(out)
    got = {k: (int(out[i][0]), int(out[i][1])) for i, k in enumerate(OP_COUNTS)}
    assert got == OP_COUNTS, got
