"""GPU: the calls of tests/test_launch_kinds_host.py on honest inputs, with the plan self-check (AFX_VARIANT_SELFCHECK: every plan
assembled twice and compared after relocation) on and off: byte-identical outputs and statuses, outputs that verify or round-trip as
the neighbouring tests assert for the same calls, and at least one launch of every kind of the engine's table
(aeonflux_amd/csrc/launch_kinds.hpp).  3 items take the latency plan, 5 items the plan of large passes; secret-independent addressing
off and on the prover side, because some kernels run only under one of the two (k_msm_naf: the key's NAF terms of a large pass
in mode 0; k_table_affine: a large prover pass in mode 2).  The whole-message calls run on messages of 0, 30 and 31 bytes: an empty
one, an exact chunk, one that straddles two chunks."""
import hashlib

import numpy as np
import pytest

from tests.helpers import DevMem, make_credentials
from tests.test_blind_ref import make_case
from tests.test_launch_kinds_host import KIND_NAMES

pytestmark = pytest.mark.gpu

N, HIDE, BLIND_KINDS = 4, [0, 3], [4, 2, 3, 1]
MESSAGES = [b"", bytes(range(30)), bytes(range(100, 131))]


@pytest.fixture(scope="module")
def world():
    import aeonflux_amd as afx
    d = make_credentials(N, "SSPE", 5, b"gpu-launch-kinds")
    b = make_case(N, BLIND_KINDS, 5, b"gpu-launch-kinds-blind")
    w = dict(d=d, b=b, ctx=afx.Context(d["params"], d["key"], d["ip"]), bctx=afx.Context(b["params"], b["key"], b["ip"]))
    w["draws"] = hashlib.shake_256(b"gpu-launch-kinds draws").digest(5 * 512)
    yield w
    w["ctx"].close()
    w["bctx"].close()


def col(items, w):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), w)


def flow(w, cnt):
    """every call over the first cnt items; returns every output and status (the checks that need no second run are made here)"""
    from aeonflux_amd import batch
    d, ctx, user = w["d"], w["ctx"], w["d"]["user"]
    creds = d["creds"][:cnt]
    kinds = list(creds[0]["kinds"])
    part = lambda lo: np.stack([col([c["values"][i][lo:lo + 32] for c in creds], 32) for i in range(N)])
    values, M2, m3 = part(0), part(32), part(64)
    draw = lambda i, at, k: w["draws"][512 * i + at:512 * i + at + k]
    out = {}
    # issue (issuer.rs:111-124): the oracle's bytes; the issuances verify
    iss, st = batch.issue(ctx, kinds, values, col([c["rnd"][0] for c in creds], 64), col([c["rnd"][1] for c in creds], 64), col([c["rnd"][2] for c in creds], 32))
    assert not st.any()
    for f in ("t", "U", "V", "challenge"):
        assert iss[f].tobytes() == b"".join(c[f] for c in creds), f
    assert iss["responses"].tobytes() == b"".join(c["responses"][k] for k in range(N + 5) for c in creds)
    out["issue"] = (iss, st)
    out["verify_issuances"] = batch.verify_issuances(ctx, kinds, values, iss)
    assert not out["verify_issuances"].any()
    # keypairs (symmetric.rs:197-215): the oracle's
    ms = col([draw(i, 0, 64) for i in range(cnt)], 64)
    kp = batch.keypairs_derive(ctx, ms)
    for i in range(cnt):
        assert b"".join(kp[f][i].tobytes() for f in ("a", "a0", "a1", "pk")) == bytes(user.keypair_derive(ms[i].tobytes())), i
    out["keypairs"] = kp
    # show with a hidden scalar and a hidden encrypted point (credential.rs:37-46), compact and batchable; both verify
    shown = [1 if (i in HIDE and k == 0) else 4 if i in HIDE else k for i, k in enumerate(kinds)]
    nsp = sum(1 for k in shown if k == 4)
    args = (shown, values, iss["t"], iss["U"], iss["V"], kp, col([draw(i, 64, 64) for i in range(cnt)], 64), col([draw(i, 128, 32) for i in range(cnt)], 32),
            np.stack([col([draw(i, 160 + 32 * e, 32) for i in range(cnt)], 32) for e in range(nsp)]), M2, m3)
    pres, shape, st = batch.show(ctx, *args)
    assert not st.any()
    out["show"] = (pres, bytes(shape), st)
    out["verify_presentations"] = batch.verify_presentations(ctx, shape, pres)
    assert not out["verify_presentations"].any()
    bpres, cm, bshape, st = batch.show_batchable(ctx, *args)
    assert not st.any() and bytes(bshape) == bytes(shape)
    out["show_batchable"] = (bpres, cm, st)
    out["verify_batchable"] = batch.verify_presentations_batchable(ctx, bshape, bpres, cm, draw(0, 256, 32))
    assert not out["verify_batchable"].any()
    # the blind flow: the credential is the one the plain path issues from the same draws (the oracle's)
    b, bctx = w["b"], w["bctx"]
    its = b["items"][:cnt]
    bvalues = np.stack([col([it["values"][i] for it in its], 32) for i in range(N)])
    h = len(its[0]["r_wide"])
    dd = col([it["d"] for it in its], 32)
    req, st_req = batch.blind_request(bctx, BLIND_KINDS, bvalues, dd, np.stack([col([it["r_wide"][j] for it in its], 64) for j in range(h)]), col([it["req_seed"] for it in its], 32))
    st_ver = batch.verify_blind_requests(bctx, BLIND_KINDS, req)
    biss, st_iss = batch.issue_blind(bctx, BLIND_KINDS, bvalues, req, col([it["t_wide"] for it in its], 64), col([it["U_wide"] for it in its], 64),
                                     col([it["rprime_wide"] for it in its], 64), col([it["iss_seed"] for it in its], 32))
    V, st_unb = batch.unblind_issuances(bctx, BLIND_KINDS, bvalues, dd, req, biss)
    assert not (st_req.any() or st_ver.any() or st_iss.any() or st_unb.any())
    for f, mine in (("t", biss["t"]), ("U", biss["U"]), ("V", V)):
        assert [r.tobytes() for r in mine] == [it["oracle"][f] for it in its], f
    out["blind"] = (req, biss, V, st_req, st_ver, st_iss, st_unb)
    # plaintexts, encryption, decryption (symmetric.rs:135-143, 252-261, 273-289): the round trip returns the messages
    msgs = col([draw(i, 288, 30) for i in range(cnt)], 30)
    M1, pM2, pm3, ctr = batch.plaintexts_from_bytes(ctx, msgs)
    E1, E2, st = batch.encrypt(ctx, kp, M1, pM2, pm3)
    assert not st.any()
    dM1, dM2, dm3, back, st = batch.decrypt(ctx, kp, E1, E2)
    assert not st.any() and np.array_equal(back, msgs) and np.array_equal(dM1, M1) and np.array_equal(dM2, pM2) and np.array_equal(dm3, pm3)
    out["plaintexts"] = (M1, pM2, pm3, ctr, E1, E2, back)
    # the candidate at the known counter: the same plaintexts without the search
    dev = [DevMem(np.full((cnt, 32), 0xEE, np.uint8)) for _ in range(3)] + [DevMem(np.full(cnt, 0xEE, np.uint8))]
    batch.plaintexts_from_bytes_at_dev(ctx, DevMem(msgs), DevMem(ctr.view(np.uint8)), cnt, *dev)
    ctx.synchronize()
    at = [m.numpy() for m in dev]
    assert not at[3].any() and all(np.array_equal(a.reshape(cnt, 32), b_) for a, b_ in zip(at[:3], (M1, pM2, pm3)))
    out["plaintexts_at"] = at
    # whole messages, one key per message
    kp3 = {f: v[:3] for f, v in kp.items()}
    mE1, mE2, mctr, cf, st = batch.encrypt_messages(ctx, kp3, MESSAGES)
    assert not st.any() and cf.tolist() == [0, 0, 1, 3]
    back, st = batch.decrypt_messages(ctx, kp3, mE1, mE2, cf)
    assert not st.any() and [m[:len(want)] for m, want in zip(back, MESSAGES)] == MESSAGES and not any(any(m[len(want):]) for m, want in zip(back, MESSAGES))
    out["messages"] = (mE1, mE2, mctr, back)
    return out


def flat(x):
    if isinstance(x, dict):
        return b"".join(k.encode() + flat(v) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return b"".join(flat(v) for v in x)
    return x if isinstance(x, bytes) else b"" if x is None else np.ascontiguousarray(x).tobytes()


def test_every_call_is_the_same_under_the_self_check_and_every_kind_is_launched(world):
    import aeonflux_amd as afx
    ctxs = (world["ctx"], world["bctx"])
    for c in ctxs:
        c.set_timing(True)
    for cnt, small in ((3, 4096), (5, 0)):       # the latency plan and the plan of large passes
        for secret in (0, 2):
            got = []
            for flags in (afx.VARIANT_SELFCHECK, 0):
                for c in ctxs:
                    c.set_small_batch_items(small)
                    c.set_secret_independent_addressing(secret)
                    c.set_plan_variants(flags)
                got.append({k: flat(v) for k, v in flow(world, cnt).items()})
            differ = [k for k in got[0] if got[0][k] != got[1][k]]
            assert not differ, (cnt, small, secret, differ)
    launches = {name: sum(c.get_timing(name)[1] for c in ctxs) for name in KIND_NAMES}
    for c in ctxs:
        c.set_timing(False)
        c.set_small_batch_items(4096)
        c.set_secret_independent_addressing(2)
    assert all(launches.values()), [k for k, v in launches.items() if not v]
