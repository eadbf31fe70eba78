"""Plaintexts from bytes, derived keypairs, encryption, decryption and SHA-512 on the device (aeonflux_amd/csrc/sha512.cuh, k_sha512,
k_encode_to_group; the four *_dev plans of statements_setup.cpp) against hashlib and the oracle, item by item."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H = bytes.fromhex
TSUNAMI = b"This is a tsunami alert test.."


@pytest.fixture(scope="module")
def user():
    import oracle
    import aeonflux_amd as afx
    st = hashlib.shake_256(b"afx-tests/plaintext-context/v1").digest(1 << 15)
    params, used = oracle.system_parameters_generate(5, st)
    key, ip = oracle.issuer_new(params, st[used:used + 64 * 9])
    ctx = afx.Context(params, None, ip)
    yield ctx, oracle.Ctx(params, None, ip)
    ctx.close()


def rows(a):
    return [r.tobytes() for r in a]


def dev(a):
    """the rows of a host array in device memory (no PyTorch: tests/helpers.py DevMem)"""
    from tests.helpers import DevMem
    return DevMem(np.ascontiguousarray(a).view(np.uint8))


def out(*shape):
    from tests.helpers import DevMem
    return DevMem(np.full(shape, 0xEE, np.uint8))


def plaintexts_dev(ctx, msgs):
    from aeonflux_amd import batch
    n = len(msgs)
    o = [out(n, 32), out(n, 32), out(n, 32), out(n, 4), out(n)]
    batch.plaintexts_from_bytes_dev(ctx, dev(msgs), n, *o)
    ctx.synchronize()
    M1, M2, m3, ctr, st = (x.numpy() for x in o)
    return M1, M2, m3, ctr.view(np.uint32).reshape(n), st


def derive_dev(ctx, ms):
    from aeonflux_amd import batch
    n = len(ms)
    o = {f: out(n, 32) for f in ("a", "a0", "a1", "pk")}
    batch.keypairs_derive_dev(ctx, dev(ms), n, o["a"], o["a0"], o["a1"], o["pk"])
    ctx.synchronize()
    return {f: o[f].numpy() for f in o}


def encrypt_dev(ctx, kp, M1, M2, m3):
    from aeonflux_amd import batch
    n = len(M1)
    o = [out(n, 32), out(n, 32), out(n)]
    batch.encrypt_dev(ctx, {f: dev(kp[f]) for f in kp}, dev(M1), dev(M2), dev(m3), n, *o)
    ctx.synchronize()
    return [x.numpy() for x in o]


def decrypt_dev(ctx, kp, E1, E2):
    from aeonflux_amd import batch
    n = len(E1)
    o = [out(n, 32), out(n, 32), out(n, 32), out(n, 30), out(n)]
    batch.decrypt_dev(ctx, {f: dev(kp[f]) for f in kp}, dev(E1), dev(E2), n, *o)
    ctx.synchronize()
    return [x.numpy() for x in o]


def test_sha512_vectors_and_every_length(user):
    from aeonflux_amd import batch
    ctx, _ = user
    two_blocks = b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"
    want = {
        b"": "cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e",
        b"abc": "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
        two_blocks: "8e959b75dae313da8cf4f72814fc143f8f7779c6eb9f7fa17299aeadb6889018501d289e4900f7e4331b99dec4b5433ac7d329eeb6dd26545e96e55b874be909",
    }
    for msg, hexd in want.items():
        got = batch.sha512(ctx, np.frombuffer(msg * 3, np.uint8).reshape(3, len(msg)))
        assert [r.hex() for r in rows(got)] == [hexd] * 3, msg
    src = hashlib.shake_256(b"afx-tests/sha512-lengths").digest(70 * 260)
    for n in range(261):          # 70 items: more than a wave
        msgs = np.frombuffer(src[:70 * n], np.uint8).reshape(70, n)
        got = batch.sha512(ctx, msgs)
        assert rows(got) == [hashlib.sha512(m.tobytes()).digest() for m in msgs], n
    long = np.frombuffer(hashlib.shake_256(b"afx-tests/sha512-long").digest(5 * 1024), np.uint8).reshape(5, 1024)
    assert rows(batch.sha512(ctx, long)) == [hashlib.sha512(m.tobytes()).digest() for m in long]


def plaintext_messages(primitives):
    msgs = hashlib.shake_256(b"afx-tests/plaintext-messages/v1").digest(30 << 14)
    extra = [bytes(30), TSUNAMI] + [H(v["msg"]) for v in primitives["encode_to_group"] if len(H(v["msg"])) == 30]
    return np.frombuffer(msgs + b"".join(extra), np.uint8).reshape(-1, 30), len(extra)


def check_plaintexts(msgs, M1, M2, m3, counters, status=None):
    import oracle
    for i, m in enumerate(msgs):
        want, ctr = oracle.plaintext_from_bytes(m.tobytes())
        assert M1[i].tobytes() + M2[i].tobytes() + m3[i].tobytes() == want and int(counters[i]) == ctr, (i, m.tobytes().hex(), int(counters[i]), ctr)
    assert status is None or not status.any()


def test_plaintexts_from_bytes_vs_oracle(user, primitives):
    from aeonflux_amd import batch
    ctx, _ = user
    msgs, n_extra = plaintext_messages(primitives)
    assert len(msgs) == (1 << 14) + n_extra and n_extra >= 3
    M1, M2, m3, counters = batch.plaintexts_from_bytes(ctx, msgs)
    # the fixture crosses what used to be a round of 16 counters (and the mean is the four tries a quarter's chance gives)
    assert (counters >= 16).sum() >= 1 and counters.max() < 128 and 3.5 < counters[:1 << 14].mean() + 1 < 4.5, (counters.max(), counters.mean())
    check_plaintexts(msgs, M1, M2, m3, counters)
    assert counters[1 << 14] == 0 and M1[1 << 14].tobytes() == bytes(32)      # [0u8; 30] encodes to the identity at counter 0
    for v in primitives["encode_to_group"]:
        if len(H(v["msg"])) == 30:
            i = [m.tobytes() for m in msgs[1 << 14:]].index(H(v["msg"]))
            assert M1[(1 << 14) + i].tobytes().hex() == v["point"]
    # the *_dev form, and both with passes of 256 items
    d = plaintexts_dev(ctx, msgs)
    assert all(np.array_equal(x, y) for x, y in zip(d[:4], (M1, M2, m3, counters))) and not d[4].any()
    ctx.set_chunk_items(256)
    try:
        sub = msgs[-(5 * 256 + 7):]
        c = batch.plaintexts_from_bytes(ctx, sub)
        assert all(np.array_equal(x, y[-len(sub):]) for x, y in zip(c, (M1, M2, m3, counters)))
        d = plaintexts_dev(ctx, sub)
        assert all(np.array_equal(x, y[-len(sub):]) for x, y in zip(d[:4], (M1, M2, m3, counters))) and not d[4].any()
    finally:
        ctx.set_chunk_items(0)


@pytest.mark.parametrize("secret_mode", [0, 2])
def test_keypairs_derive_vs_oracle(user, secret_mode):
    from aeonflux_amd import batch
    ctx, octx = user
    ms = np.frombuffer(hashlib.shake_256(b"afx-tests/master-secrets/v1").digest(64 * 4096), np.uint8).reshape(4096, 64)
    ctx.set_secret_independent_addressing(secret_mode)
    try:
        kp = batch.keypairs_derive(ctx, ms)
        for i in range(4096):
            assert b"".join(kp[f][i].tobytes() for f in ("a", "a0", "a1", "pk")) == octx.keypair_derive(ms[i].tobytes()), i
        kd = derive_dev(ctx, ms)
        assert all(np.array_equal(kd[f], kp[f]) for f in kp)
        ctx.set_chunk_items(256)
        kc = batch.keypairs_derive(ctx, ms[:3 * 256 + 5])
        assert all(np.array_equal(kc[f], kp[f][:3 * 256 + 5]) for f in kp)
    finally:
        ctx.set_chunk_items(0)
        ctx.set_secret_independent_addressing(2)


def test_encrypt_decrypt_vs_oracle(user, primitives):
    import oracle
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    ctx, octx = user
    n = 1024
    msgs = np.frombuffer(hashlib.shake_256(b"afx-tests/decrypt-messages/v1").digest(30 * (n - 2)) + bytes(30) + TSUNAMI, np.uint8).reshape(n, 30)
    ms = np.frombuffer(hashlib.shake_256(b"afx-tests/decrypt-keys/v1").digest(64 * n), np.uint8).reshape(n, 64)
    kp = batch.keypairs_derive(ctx, ms)
    M1, M2, m3, _ = batch.plaintexts_from_bytes(ctx, msgs)
    okp = [b"".join(kp[f][i].tobytes() for f in ("a", "a0", "a1", "pk")) for i in range(n)]
    # honest items
    E1, E2, st = batch.encrypt(ctx, kp, M1, M2, m3)
    assert not st.any()
    for i in range(n):
        assert E1[i].tobytes() + E2[i].tobytes() == oracle.encrypt(okp[i], M1[i].tobytes() + M2[i].tobytes() + m3[i].tobytes()), i
    dE1, dE2, dst = encrypt_dev(ctx, kp, M1, M2, m3)
    assert np.array_equal(dE1, E1) and np.array_equal(dE2, E2) and not dst.any()

    def check(kp_, E1_, E2_, expect_some_bad):
        got = batch.decrypt(ctx, kp_, E1_, E2_)
        gd = decrypt_dev(ctx, kp_, E1_, E2_)
        assert all(np.array_equal(x, y) for x, y in zip(got, gd))
        g1, g2, g3, gm, gst = got
        bad = 0
        for i in range(len(E1_)):
            key = b"".join(kp_[f][i].tobytes() for f in ("a", "a0", "a1", "pk"))
            rc, pt = oracle.decrypt(key, E1_[i].tobytes() + E2_[i].tobytes())
            # the oracle's "does not decode" (-1) and "does not decrypt" (1) are both CredentialError::UndecryptableAttribute here
            assert gst[i] == (afx.ST_OK if rc == 0 else afx.ST_UNDECRYPTABLE), (i, rc, gst[i])
            if rc == 0:
                assert g1[i].tobytes() + g2[i].tobytes() + g3[i].tobytes() == pt and gm[i].tobytes() == pt[1:31], i
            bad += rc != 0
        assert (bad > 0) == expect_some_bad
        return got

    g1, g2, g3, gm, gst = check(kp, E1, E2, False)
    assert np.array_equal(gm, msgs) and np.array_equal(g1, M1) and np.array_equal(g2, M2) and np.array_equal(g3, m3)
    assert batch.decrypt(ctx, kp, E1, E2, messages=False)[3] is None
    # the wrong keypair: every item's neighbour's
    wrong = {f: np.roll(kp[f], 1, axis=0) for f in kp}
    assert (check(wrong, E1, E2, True)[4] == afx.ST_UNDECRYPTABLE).all()
    # one flipped bit in E1 or E2 at seeded positions
    r = np.random.default_rng(20261017)
    F1, F2 = E1.copy(), E2.copy()
    for i in range(n):
        (F1 if r.integers(2) else F2)[i, r.integers(32)] ^= 1 << r.integers(8)
    full = check(kp, F1, F2, True)
    # passes of 256 items
    ctx.set_chunk_items(256)
    try:
        m = 3 * 256 + 5
        c = batch.decrypt(ctx, {f: kp[f][:m] for f in kp}, F1[:m], F2[:m])
        assert all(np.array_equal(x, y[:m]) for x, y in zip(c, full))
    finally:
        ctx.set_chunk_items(0)


def test_a_million_plaintexts_in_one_call(user):
    from aeonflux_amd import batch
    ctx, _ = user
    n = 1 << 20
    msgs = np.frombuffer(hashlib.shake_256(b"afx-tests/plaintext-million/v1").digest(30 * n), np.uint8).reshape(n, 30)
    M1, M2, m3, counters = batch.plaintexts_from_bytes(ctx, msgs)
    s = slice(0, n, n >> 12)
    check_plaintexts(msgs[s], M1[s], M2[s], m3[s], counters[s])
    check_plaintexts(msgs[-3:], M1[-3:], M2[-3:], m3[-3:], counters[-3:])
