"""Blind issuance on the device (aeonflux_amd/csrc/statements_blind.cpp, k_mask_rows) against the yardstick tests/blind_ref.py, the
oracle's plain `issue` and the engine's own: every output byte of the four calls, the per-item verdicts on damaged requests and
issuances with the failed items' outputs zeroed, blind-issued credentials through show and verify, and byte identity across secret
modes, key schedules, plan variants, passes and the _dev forms.

One case of 300 items per layout (tests/test_blind_ref.make_case) serves every count - 1, 70 (more than a wave, no multiple of 64) and
300 (past the 256-item plan switch, several blocks) take its first items - and the yardstick runs once per (layout, item)."""
import random

import numpy as np
import pytest

from tests import blind_ref as BR
from tests.test_blind_ref import LAYOUTS, make_case

pytestmark = pytest.mark.gpu

GPU_LAYOUTS = LAYOUTS + [(2, [0, 2])]          # (3, [0, 2, 3]) and (2, [0, 2]) hide nothing
COUNTS = (1, 70, 300)
REQ, ISS = ("D", "A", "B", "challenge", "responses"), ("t", "U", "S1", "S2", "challenge", "responses")


class Case:
    def __init__(self, n, kinds):
        import aeonflux_amd as afx
        self.n, self.kinds = n, list(kinds)
        self.c = make_case(n, self.kinds, 300, b"gpu-blind-%d-%s" % (n, bytes(kinds)))
        self.issuer = afx.Context(self.c["params"], self.c["key"], self.c["ip"])
        self.user = afx.Context(self.c["params"], None, self.c["ip"])
        self.H = BR.hidden_positions(self.kinds)
        self.h, self.hs = len(self.H), sum(1 for k in kinds if k == 1)
        its = self.c["items"]
        col = lambda f, w: np.frombuffer(b"".join(it[f] for it in its), np.uint8).reshape(len(its), w)
        self.values = np.stack([np.frombuffer(b"".join(it["values"][i] for it in its), np.uint8).reshape(len(its), 32) for i in range(n)])
        self.d, self.req_seed, self.iss_seed = col("d", 32), col("req_seed", 32), col("iss_seed", 32)
        self.t_wide, self.U_wide, self.rprime_wide = col("t_wide", 64), col("U_wide", 64), col("rprime_wide", 64)
        self.r_wide = np.stack([np.frombuffer(b"".join(it["r_wide"][j] for it in its), np.uint8).reshape(len(its), 64) for j in range(self.h)]) \
            if self.h else np.zeros((0, len(its), 64), np.uint8)
        self.ref, self.flows = {}, {}

    def close(self):
        self.issuer.close()
        self.user.close()

    def reference(self, i):
        """the yardstick's flow of item i: (request, issuance, V)"""
        if i not in self.ref:
            from tests.test_blind_ref import run_flow
            self.ref[i] = run_flow(self.c, self.c["items"][i])
        return self.ref[i]

    def inputs(self, cnt):
        cut = lambda a: np.ascontiguousarray(a[..., :cnt, :])
        return dict(values=cut(self.values), d=cut(self.d), r_wide=cut(self.r_wide), req_seed=cut(self.req_seed), t_wide=cut(self.t_wide), U_wide=cut(self.U_wide),
                    rprime_wide=cut(self.rprime_wide), iss_seed=cut(self.iss_seed))

    def flow(self, cnt, dev=False, keep=False):
        """the four calls over the first cnt items; dict(req, iss, V, st = the four status arrays)"""
        if keep and (cnt, dev) in self.flows:
            return self.flows[(cnt, dev)]
        out = (flow_dev if dev else flow_host)(self, self.inputs(cnt), cnt)
        if keep:
            self.flows[(cnt, dev)] = out
        return out


def flow_host(case, x, cnt):
    from aeonflux_amd import batch
    req, st_req = batch.blind_request(case.user, case.kinds, x["values"], x["d"], x["r_wide"], x["req_seed"])
    st_ver = batch.verify_blind_requests(case.user, case.kinds, req)
    iss, st_iss = batch.issue_blind(case.issuer, case.kinds, x["values"], req, x["t_wide"], x["U_wide"], x["rprime_wide"], x["iss_seed"])
    V, st_unb = batch.unblind_issuances(case.user, case.kinds, x["values"], x["d"], req, iss)
    return dict(req=req, iss=iss, V=V, st=[st_req, st_ver, st_iss, st_unb])


def flow_dev(case, x, cnt):
    from aeonflux_amd import batch
    from tests.helpers import DevMem
    dev = lambda a: DevMem(a) if a.size else None
    out = lambda *shape: DevMem(np.full(shape, 0xEE, np.uint8)) if int(np.prod(shape)) else None
    n, h, hs = case.n, case.h, case.hs
    dx = {k: dev(v) for k, v in x.items()}
    # the issuer's copy of the values holds 0xEE in the rows of hidden positions: they are never read
    blinded = x["values"].copy()
    for i in case.H:
        blinded[i] = 0xEE
    d_blinded = dev(blinded)
    req = dict(D=out(cnt, 32), A=out(h, cnt, 32), B=out(h, cnt, 32), challenge=out(cnt, 32), responses=out(1 + h + hs, cnt, 32))
    iss = dict(t=out(cnt, 32), U=out(cnt, 32), S1=out(cnt, 32), S2=out(cnt, 32), challenge=out(cnt, 32), responses=out(n + 6, cnt, 32))
    V, st = out(cnt, 32), [out(cnt) for _ in range(4)]
    batch.blind_request_dev(case.user, case.kinds, dx["values"], dx["d"], dx["r_wide"], dx["req_seed"], cnt, req, st[0])
    batch.verify_blind_requests_dev(case.user, case.kinds, req, 1 + h + hs, cnt, st[1])
    case.user.synchronize()          # the issuer is another context: its stream does not wait for the user's
    batch.issue_blind_dev(case.issuer, case.kinds, d_blinded, req, 1 + h + hs, dx["t_wide"], dx["U_wide"], dx["rprime_wide"], dx["iss_seed"], cnt, iss, st[2])
    case.issuer.synchronize()
    batch.unblind_issuances_dev(case.user, case.kinds, dx["values"], dx["d"], req, iss, n + 6, cnt, V, st[3])
    case.user.synchronize()
    host = lambda m, shape: m.numpy() if m is not None else np.zeros(shape, np.uint8)
    return dict(req={f: host(req[f], (0, cnt, 32)) for f in REQ}, iss={f: iss[f].numpy() for f in ISS}, V=V.numpy(), st=[s.numpy() for s in st])


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, kinds):
        key = (n, tuple(kinds))
        if key not in made:
            made[key] = Case(n, kinds)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def item_of(rec, fields, i):
    """item i of a dict of arrays as the yardstick's record: single fields as bytes, repeated ones as lists of bytes"""
    return {f: (rec[f][i].tobytes() if rec[f].ndim == 2 else [row[i].tobytes() for row in rec[f]]) for f in fields}


def same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in a)


# ---- 1. every output byte, every layout, every count ----
@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("n,kinds", GPU_LAYOUTS)
def test_outputs_equal_the_yardstick_and_the_plain_credential(cases, n, kinds, cnt):
    from aeonflux_amd import batch
    case = cases(n, kinds)
    got = case.flow(cnt, keep=True)
    for name, st in zip(("request", "verify", "issue", "unblind"), got["st"]):
        assert st.tolist() == [0] * cnt, name
    assert got["req"]["responses"].shape == (1 + case.h + case.hs, cnt, 32) and got["iss"]["responses"].shape == (n + 6, cnt, 32)
    for i in sorted({0, cnt // 2, cnt - 1}):
        req, iss, V = case.reference(i)
        assert item_of(got["req"], REQ, i) == {f: req[f] for f in REQ}, i
        assert item_of(got["iss"], ISS, i) == {f: iss[f] for f in ISS}, i
        assert got["V"][i].tobytes() == V, i
    # the credential the oracle-pinned path issues from the same draws, item by item: the oracle's and the engine's own
    x = case.inputs(cnt)
    plain, st = batch.issue(case.issuer, case.kinds, x["values"], x["t_wide"], x["U_wide"], x["iss_seed"])
    assert not st.any()
    for f, mine in (("t", got["iss"]["t"]), ("U", got["iss"]["U"]), ("V", got["V"])):
        assert np.array_equal(mine, plain[f]), f
        assert [r.tobytes() for r in mine] == [it["oracle"][f] for it in case.c["items"][:cnt]], f


# ---- 2, 3. damaged requests and issuances: the yardstick's verdict item by item, zeros for the failed, the others untouched ----
DAMAGE_LAYOUT = (4, [4, 2, 3, 1])


def damage(rec, fields, cnt, seed):
    """a seeded choice per item: leave it, or damage ONE cell (a flipped bit, zeros, 0xff bytes, or the next item's cell).  Returns
    (damaged copy, {item: what})"""
    rng = random.Random(seed)
    out = {f: rec[f].copy() for f in fields}
    cells = []
    for f in fields:
        cells += [(f, None)] if out[f].ndim == 2 else [(f, k) for k in range(out[f].shape[0])]
    done = {}
    for i in range(cnt):
        if rng.random() >= 0.28:
            continue
        f, k = cells[rng.randrange(len(cells))]
        row = out[f] if k is None else out[f][k]
        src = rec[f] if k is None else rec[f][k]
        what = rng.choice(("bit", "zeros", "ff", "next"))
        if what == "bit":
            row[i, rng.randrange(32)] ^= 1 << rng.randrange(8)
        elif what == "zeros":
            row[i] = 0
        elif what == "ff":
            row[i] = 0xFF
        else:
            row[i] = src[(i + 1) % cnt]
        done[i] = (f, k, what)
    return out, done


def test_damaged_requests_fail_alone_and_release_nothing(cases):
    from aeonflux_amd import batch
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 70
    good = case.flow(cnt, keep=True)
    bad_req, done = damage(good["req"], REQ, cnt, 0xB11D)
    assert 10 <= len(done) <= 30, len(done)          # the seed's doing, before the engine is asked
    honest = [i for i in range(cnt) if i not in done][:3]
    verdict = {i: BR.verify_request(case.c["params"], kinds, item_of(bad_req, REQ, i)) for i in sorted(done) + honest}
    assert set(verdict.values()) == {0, 1} and all(verdict[i] == 0 for i in honest)
    x = case.inputs(cnt)
    st_ver = batch.verify_blind_requests(case.user, kinds, bad_req)
    iss, st_iss = batch.issue_blind(case.issuer, kinds, x["values"], bad_req, x["t_wide"], x["U_wide"], x["rprime_wide"], x["iss_seed"])
    for i, v in verdict.items():
        assert st_ver[i] == v and st_iss[i] == v, (i, done.get(i), v, st_ver[i], st_iss[i])
    assert st_ver.tolist() == st_iss.tolist() and all(st_ver[i] == 0 for i in range(cnt) if i not in done)
    for i in range(cnt):
        for f in ISS:
            cell, ref = iss[f][..., i, :], good["iss"][f][..., i, :]
            if st_iss[i]:
                assert not cell.any(), (i, f)          # no S1, S2 or response for a request that was not accepted
            else:
                assert np.array_equal(cell, ref), (i, f)
    assert any(st_iss) and not all(st_iss)


def test_damaged_issuances_fail_alone_with_V_zero(cases):
    from aeonflux_amd import batch
    n, kinds = DAMAGE_LAYOUT
    case, cnt = cases(n, kinds), 70
    good = case.flow(cnt, keep=True)
    bad_iss, done = damage(good["iss"], ISS, cnt, 0x155E)
    assert 10 <= len(done) <= 30, len(done)
    honest = [i for i in range(cnt) if i not in done][:3]
    its = case.c["items"]
    verdict = {i: BR.unblind(case.c["params"], case.c["ip"], kinds, its[i]["values"], item_of(good["req"], REQ, i), its[i]["d"], item_of(bad_iss, ISS, i))
               for i in sorted(done) + honest}
    assert {v[0] for v in verdict.values()} == {0, 1} and all(verdict[i][0] == 0 for i in honest)
    x = case.inputs(cnt)
    V, st = batch.unblind_issuances(case.user, kinds, x["values"], x["d"], good["req"], bad_iss)
    for i, (v, V_ref) in verdict.items():
        assert st[i] == v, (i, done.get(i), v, st[i])
        assert V[i].tobytes() == (V_ref if v == 0 else bytes(32)), (i, done.get(i))
    for i in range(cnt):
        if st[i]:
            assert not V[i].any(), i
        elif i not in done:
            assert np.array_equal(V[i], good["V"][i]), i
    assert all(st[i] == 0 for i in range(cnt) if i not in done)


# ---- 4. end to end: blind-issued credentials, their hidden positions shown hidden ----
def test_blind_issued_credentials_show_and_verify():
    import hashlib
    import oracle
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    n, kinds, cnt = 3, [0, 1, 4], 70
    s = hashlib.shake_256(b"gpu-blind-end-to-end").digest(1 << 16)
    params, used = oracle.system_parameters_generate(n, s)
    key, ip = oracle.issuer_new(params, s[used:used + 64 * (4 + n)])
    draw = np.random.default_rng(20191416)
    rb = lambda *shape: draw.integers(0, 256, shape, dtype=np.uint8)
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    try:
        # the hidden SECRET_POINT is an application message: M1 (the attribute), M2 and m3 from the device's own encoding
        M1, M2, m3, _ = batch.plaintexts_from_bytes(user, rb(cnt, 30))
        values = np.stack([batch.scalars_from_wide(user, rb(cnt, 64)), batch.scalars_from_wide(user, rb(cnt, 64)), M1])
        d = batch.scalars_from_wide(user, rb(cnt, 64))
        req, st = batch.blind_request(user, kinds, values, d, rb(2, cnt, 64), rb(cnt, 32))
        assert not st.any()
        seen = values.copy()
        seen[1:] = 0          # what the issuer is given of the hidden positions: nothing
        iss, st = batch.issue_blind(issuer, kinds, seen, req, rb(cnt, 64), rb(cnt, 64), rb(cnt, 64), rb(cnt, 32))
        assert not st.any()
        V, st = batch.unblind_issuances(user, kinds, values, d, req, iss)
        assert not st.any()
        kp = batch.keypairs_derive(user, rb(cnt, 64))
        zeros = np.zeros((cnt, 32), np.uint8)
        pres, shape, st = batch.show(user, kinds, values, iss["t"], iss["U"], V, kp, rb(cnt, 64), rb(cnt, 32), rb(1, cnt, 32),
                                     np.stack([zeros, zeros, M2]), np.stack([zeros, zeros, m3]))
        assert not st.any()
        assert batch.verify_presentations(issuer, shape, pres).tolist() == [0] * cnt
        # ... and a V the issuer did not make is no credential
        V[3, 0] ^= 1
        V[4] = V[5]
        pres, shape, st = batch.show(user, kinds, values, iss["t"], iss["U"], V, kp, rb(cnt, 64), rb(cnt, 32), rb(1, cnt, 32),
                                     np.stack([zeros, zeros, M2]), np.stack([zeros, zeros, m3]))
        verdict = batch.verify_presentations(issuer, shape, pres)
        assert verdict[4] == 1 and verdict[6:].tolist() == [0] * (cnt - 6)
    finally:
        issuer.close()
        user.close()


# ---- 5. byte identity ----
# AFX_VARIANT_ALL is the mask of the variant bits; a context takes at most one SEGMENTS choice, so "all" is each of the three with
# every other bit (AFX_VARIANT_SELFCHECK among them)
ALL_VARIANTS = (0x79, 0x7a, 0x7c)


@pytest.mark.parametrize("cnt", (70, 300))
def test_byte_identity_across_modes_variants_passes_and_forms(cases, cnt):
    n, kinds = 8, [0, 1, 2, 4, 3, 1, 4, 0]
    case = cases(n, kinds)
    base = case.flow(cnt, keep=True)
    assert not any(st.any() for st in base["st"])

    def check(what, got):
        assert all(st.tolist() == [0] * cnt for st in got["st"]), what
        assert same(base["req"], got["req"]) and same(base["iss"], got["iss"]) and np.array_equal(base["V"], got["V"]), what
    both = (case.issuer, case.user)
    try:
        for c in both:
            c.set_secret_independent_addressing(0)
        check("secret mode 0", case.flow(cnt))
        for c in both:
            c.set_secret_independent_addressing(2)
        case.issuer.set_fixed_key_schedule(1)
        check("fixed key schedule", case.flow(cnt))
        case.issuer.set_fixed_key_schedule(0)
        for v in ALL_VARIANTS:
            for c in both:
                c.set_plan_variants(v)
            check("plan variants %#x" % v, case.flow(cnt))
        for c in both:
            c.set_plan_variants(0)
        if cnt == 300:
            for c in both:
                c.set_chunk_items(256)
            check("two passes", case.flow(cnt))
            check("two passes, device rows", case.flow(cnt, dev=True))
            for c in both:
                c.set_chunk_items(0)
        check("device rows", case.flow(cnt, dev=True))
    finally:
        for c in both:
            c.set_secret_independent_addressing(2)
            c.set_plan_variants(0)
            c.set_chunk_items(0)
        case.issuer.set_fixed_key_schedule(0)
