"""GPU: every multiscalar path driven with CHOSEN scalars, keys and points, against the ORACLE's bytes.

The other parity tests draw their scalars from a hash (uniform mod l) and their issuer keys from oracle.issuer_new over hash draws,
so the digits they feed the recodings are uniform too: a 13-bit window reads its entry 0 or 4096 once in 8192 lookups, a zero
scalar or a key of empty / one-digit / maximum-weight width-5 NAF never occurs.  Here the named values of tests/edge_values.py
go through each recoding the kernels run (kernels.hip msm_add_var's 4-bit windows, narrow_fetch / narrow_select's 2-bit windows,
msm_add_positional's 13-bit and msm_add_positional_secret's 6-bit positional windows, the host's NAF of the key) under every
secret mode, the fixed key schedule on and off, every plan variant and sizes on both sides of the thresholds, and every
output is compared with the oracle's - never with another GPU run.  The oracle runs once per module."""
import copy

import numpy as np
import pytest

from tests.edge_values import NON_CANONICAL, all_scalars, b32, edge_key, edge_points, key_draws
from tests.helpers import gpu_verify
from tests.test_gpu_plan_variants import HIDE, LAYOUT, N, SIZES, check_issue, check_show, variants
from tests.test_gpu_primitives import msm

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)   # afx_ctx_set_secret_independent_addressing: nowhere, everywhere, prover-side calls (the default)
EDGE = list(all_scalars().values())
EDGE_NONZERO = [s for s in EDGE if s]
MAX_TERMS = 72      # plan.h AFX_MSM_MAX_TERMS


def _pad(b):
    return b + bytes(96 - len(b))


def _generators(params):
    """G_a, G_a0, G_a1 from the serialized SystemParameters: n, B, G_w, G_w', G_x0, G_x1, G_y[g], G_m[n], G_V, G_a, G_a0, G_a1"""
    n = int.from_bytes(params[:4], "little")
    g = max(n, 3)
    at = 4 + 32 * (1 + 4 + g + n + 1)
    return [params[at + 32 * k:at + 32 * k + 32] for k in range(3)]


@pytest.fixture(scope="module")
def world(primitives):
    """max(SIZES) credentials issued by the oracle under an edge key, with edge t, edge scalar attributes, U = identity for every
    seventh item, and the oracle's presentations of them with edge z and edge keypairs"""
    import hashlib
    import oracle
    s = hashlib.shake_256(b"gpu-edge-scalars").digest(1 << 20)
    pos = [0]

    def take(k):
        pos[0] += k
        return s[pos[0] - k:pos[0]]
    params, used = oracle.system_parameters_generate(N, s)
    pos[0] = used
    key_scalars = edge_key(N, 0)
    key, ip = oracle.issuer_new(params, key_draws(key_scalars))
    assert key[4:4 + 32 * (4 + N)] == b"".join(b32(x) for x in key_scalars)   # the key holds exactly the chosen scalars
    issuer, user = oracle.Ctx(params, key, ip), oracle.Ctx(params, None, ip)
    pts = [p for k, p in edge_points(oracle, primitives).items()]
    cnt = max(SIZES)
    creds = []
    for i in range(cnt):
        kinds, vals = [], []
        for a, c in enumerate(LAYOUT):
            if c == "S":
                kinds.append(0)
                vals.append(_pad(b32(EDGE[(8 * i + 3 * a) % len(EDGE)])))          # stride prime to len(EDGE): every value at every position
            elif c == "P":
                kinds.append(2)
                vals.append(_pad(pts[(i + a) % len(pts)]))
            else:
                kinds.append(3)
                vals.append(oracle.plaintext_from_bytes(take(30))[0])
        t_wide = b32(EDGE[i % len(EDGE)]) + bytes(32)
        U_wide = bytes(64) if i % 7 == 3 else take(64)          # from_uniform(0^64) is the identity
        rnd = (t_wide, U_wide, take(32))
        st, t, U, V, ch, resp = issuer.issue(kinds, vals, *rnd)
        assert st == 0, i
        creds.append(dict(kinds=kinds, values=vals, t=t, U=U, V=V, challenge=ch, responses=resp, rnd=rnd))
    assert sum(c["U"] == bytes(32) for c in creds) >= cnt // 8
    kinds = list(creds[0]["kinds"])
    shown = [1 if (i in HIDE and k == 0) else 4 if i in HIDE else k for i, k in enumerate(kinds)]
    nsp = sum(1 for k in shown if k == 4)
    G = _generators(params)
    kps, zw, sd, es, pres = [], [], [], [], []
    for i, c in enumerate(creds):
        a = [EDGE[(5 * i + 11 * j) % len(EDGE)] for j in range(3)]
        pk = oracle.multiscalar([b32(x) for x in a], G)
        kps.append(b"".join(b32(x) for x in a) + pk)
        zw.append(b32(EDGE[(4 * i) % len(EDGE)]) + bytes(32))              # z = 0 for items 0, 63, 126, ...
        sd.append(take(32))
        es.append(take(32 * nsp))
        st, p = user.show(shown, c["values"], c["t"], c["U"], c["V"], kps[-1], zw[-1], sd[-1], es[-1])
        assert st == 0, i
        pres.append(p)
    # every edge value serves as t, as each scalar attribute (the hidden one included), as z and as each keypair scalar
    edge = set(EDGE)
    val = lambda b: int.from_bytes(b[:32], "little")
    assert {val(c["rnd"][0]) for c in creds} == edge
    for a, c in enumerate(LAYOUT):
        if c == "S":
            assert {val(cr["values"][a]) for cr in creds} == edge, a
    assert {val(z) for z in zw} == edge and val(zw[0]) == 0
    for j in range(3):
        assert {val(k[32 * j:32 * j + 32]) for k in kps} == edge, j
    d = dict(params=params, key=key, ip=ip, issuer=issuer, user=user, creds=creds)
    return dict(d=d, kinds=kinds, shown=shown, nsp=nsp, kps=kps, zw=zw, sd=sd, es=es, pres=pres)


# ---- afx_multiscalar_mul: per-item scalars on variable bases (msm_add_var; k_msm and k_msm_quad) ----

def _msm_case(oracle, pts, nt, cnt, salt):
    """[nt][cnt] scalars and points, a different edge value in each lane; lane 5k: term 1 = -(term 0) with the same scalar (the
    sum cancels), lane 5k+1: term 1 = term 0 (the same point twice)"""
    S = [[b32(EDGE[(i * nt + 7 * k + salt) % len(EDGE)]) for i in range(cnt)] for k in range(nt)]
    P = [[pts[(i + 3 * k + salt) % len(pts)] for i in range(cnt)] for k in range(nt)]
    if nt >= 2:
        for i in range(cnt):
            if i % 5 == 0:
                S[1][i], P[1][i] = S[0][i], oracle.point_sub(bytes(32), P[0][i])
            elif i % 5 == 1:
                P[1][i] = P[0][i]
    want = [oracle.multiscalar([S[k][i] for k in range(nt)], [P[k][i] for k in range(nt)]) for i in range(cnt)]
    return S, P, want


def test_multiscalar_mul_at_edge_scalars_and_points(primitives):
    import oracle
    import aeonflux_amd as afx
    pts = list(edge_points(oracle, primitives).values())
    cases = {}
    for nt in (1, 2, 5, MAX_TERMS):
        for cnt in (1, 63, 64, 65, 257):
            cases[nt, cnt] = _msm_case(oracle, pts, nt, cnt, nt + cnt)
    ctx = afx.Context(*_params_key_ip())
    for name, flags in variants(afx):
        ctx.set_plan_variants(flags)
        met, sums = set(), set()
        for (nt, cnt), (S, P, want) in cases.items():
            got, ok = msm(afx, ctx, S, P)
            assert ok.all(), (name, nt, cnt)
            assert got == want, (name, nt, cnt, [i for i in range(cnt) if got[i] != want[i]][:8])
            met |= {(S[k][i], P[k][i]) for k in range(nt) for i in range(cnt)}
            sums |= set(got)
        # under every variant, every edge scalar has met every edge point in a compared lane, and some sums were the identity
        assert {(b32(x), p) for x in EDGE for p in pts} <= met, name
        assert bytes(32) in sums and len(sums) > 500, name
    ctx.set_plan_variants(0)
    # n_terms beyond AFX_MSM_MAX_TERMS is refused
    S, P, _ = cases[1, 1]
    s = np.frombuffer(b"".join(S[0]) * (MAX_TERMS + 1), np.uint8).copy()
    p = np.frombuffer(b"".join(P[0]) * (MAX_TERMS + 1), np.uint8).copy()
    out, okv = np.zeros(32, np.uint8), np.zeros(1, np.uint8)
    assert afx.lib().afx_multiscalar_mul(ctx.h, MAX_TERMS + 1, s.ctypes.data, p.ctypes.data, 1, out.ctypes.data, okv.ctypes.data) == afx.E_BAD_ARGS
    # non-canonical scalars are flagged, their neighbours (edge scalars, both terms) unaffected
    bad = list(NON_CANONICAL.values())
    lanes = []
    for i in range(2 * len(bad) + 1):
        lanes.append(bad[i // 2] if i % 2 else EDGE[(5 * i) % len(EDGE)])
    for nt in (1, 2):
        S = [[b32(x) for x in lanes]] + ([[b32(EDGE[(i + 9) % len(EDGE)]) for i in range(len(lanes))]] if nt == 2 else [])
        P = [[pts[(i + k) % len(pts)] for i in range(len(lanes))] for k in range(nt)]
        got, ok = msm(afx, ctx, S, P)
        assert ok.tolist() == [0 if i % 2 else 1 for i in range(len(lanes))], nt
        for i in range(0, len(lanes), 2):
            assert got[i] == oracle.multiscalar([S[k][i] for k in range(nt)], [P[k][i] for k in range(nt)]), (nt, i)
    ctx.close()


def _params_key_ip():
    import hashlib
    import oracle
    params, _ = oracle.system_parameters_generate(N, hashlib.shake_256(b"gpu-edge-msm").digest(1 << 14))
    key, ip = oracle.issuer_new(params, key_draws(edge_key(N, 1)))
    return params, key, ip


def test_a_key_with_zero_scalars_is_accepted():
    """the reference takes any canonical key scalar (amacs.rs SecretKey is a plain struct of Scalars); key 1 has w = 0 and a y = 0"""
    import aeonflux_amd as afx
    assert 0 in edge_key(N, 1)[:1] and 0 in edge_key(N, 1)[4:]
    ctx = afx.Context(*_params_key_ip())
    ctx.close()


# ---- issue and show under an edge key: every recoding of the prover side ----

def test_issue_under_an_edge_key_returns_the_oracles_bytes(world):
    """Issuer::issue with edge t, edge scalar attributes, U = identity, under a key of NAF weights 0, 1 and 51: t, U, V, the
    challenge and all n + 5 responses are the oracle's.  Small passes (up to set_small_batch_items items, 4096 by default) assemble
    without NAF schedules (engine.cpp msm_split), so there V's key terms run the 4-bit windows whatever the key schedule setting:
    every secret mode x plan variant x size.  The plan of large passes (small_batch_items 0) runs them as width-5 NAF schedules
    (k_msm_naf) where no secret may address a table - mode 0 - unless the fixed key schedule is on: every secret mode x key
    schedule x size, with the NAF launches counted."""
    import aeonflux_amd as afx
    d = world["d"]
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    for mode in MODES:
        ctx.set_secret_independent_addressing(mode)
        for name, flags in variants(afx):
            ctx.set_plan_variants(flags)
            for count in SIZES:
                try:
                    check_issue(afx, ctx, world, count)
                except AssertionError as e:
                    raise AssertionError("issue: variant %r, secret mode %d, %d items: %s" % (name, mode, count, e))
    ctx.set_plan_variants(0)
    ctx.set_small_batch_items(0)
    naf = {}
    for mode in MODES:
        ctx.set_secret_independent_addressing(mode)
        for fixed in (False, True):
            ctx.set_fixed_key_schedule(fixed)
            ctx.set_timing(True)
            for count in SIZES:
                try:
                    check_issue(afx, ctx, world, count)
                except AssertionError as e:
                    raise AssertionError("issue, large-pass plan: secret mode %d, fixed key %s, %d items: %s" % (mode, fixed, count, e))
            naf[mode, fixed] = ctx.get_timing("k_msm_naf")[1]
            ctx.set_timing(False)
    assert naf[0, False] >= len(SIZES), naf
    assert all(v == 0 for k, v in naf.items() if k != (0, False)), naf
    ctx.close()


def _issuance_arrays(world, count):
    cr = world["d"]["creds"][:count]
    values = np.stack([np.stack([np.frombuffer(c["values"][k][:32], np.uint8) for c in cr]) for k in range(N)])
    iss = {f: np.stack([np.frombuffer(c[f], np.uint8) for c in cr]) for f in ("t", "U", "V", "challenge")}
    iss["responses"] = np.stack([np.stack([np.frombuffer(c["responses"][k], np.uint8) for c in cr]) for k in range(N + 5)])
    return values, iss


def test_verify_issuances_of_edge_issuances_match_the_oracle(world):
    """CredentialIssuance::verify on the GPU over the edge issuances (the ones with U = identity among them): statuses and recomputed
    challenges equal the oracle's, in every secret mode and plan variant"""
    import oracle
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    d = world["d"]
    kinds = world["kinds"]
    want = {}
    for count in SIZES:
        values, iss = _issuance_arrays(world, count)
        want[count] = oracle.verify_issuances_traced(d["user"], kinds, values, iss)
    assert 0 < want[max(SIZES)][0].sum() < max(SIZES), "the edge issuances hold refused and accepted ones"
    # the recomputed challenges compared: items whose t covers the edge values
    r300 = want[max(SIZES)][2].astype(bool)
    assert len({EDGE[i % len(EDGE)] for i in np.flatnonzero(r300)}) > len(EDGE) // 2
    uctx = afx.Context(d["params"], None, d["ip"])
    for mode in MODES:
        uctx.set_secret_independent_addressing(mode)
        for name, flags in variants(afx):
            uctx.set_plan_variants(flags)
            for count in SIZES:
                st, trace, reached = want[count]
                values, iss = _issuance_arrays(world, count)
                uctx.set_challenge_trace(1, count)
                got = batch.verify_issuances(uctx, kinds, values, iss)
                tr = uctx.get_challenge_trace()[0]
                uctx.set_challenge_trace(0, 0)
                assert got.tolist() == st.tolist(), (name, mode, count)
                r = reached.astype(bool)
                assert np.array_equal(tr[r], trace[r]), (name, mode, count)
                assert tr[r].any(axis=-1).all(), (name, mode, count)   # written, not left blank
    uctx.close()


def test_show_of_edge_credentials_returns_the_oracles_bytes(world):
    """AnonymousCredential::show with edge z (0 included), edge keypair scalars on the secret points, edge hidden scalars, of
    credentials with edge t and U = identity: every output byte is the oracle's, for every secret mode x plan variant x size"""
    import aeonflux_amd as afx
    d = world["d"]
    uctx = afx.Context(d["params"], None, d["ip"])
    runs = 0
    for mode in MODES:
        uctx.set_secret_independent_addressing(mode)
        for name, flags in variants(afx):
            uctx.set_plan_variants(flags)
            for count in SIZES:
                try:
                    check_show(afx, uctx, world, count)
                except AssertionError as e:
                    raise AssertionError("show: variant %r, secret mode %d, %d items: %s" % (name, mode, count, e))
                runs += 1
    assert runs == len(MODES) * len(variants(afx)) * len(SIZES)
    uctx.close()


def test_verify_of_edge_presentations_matches_the_oracle(world):
    """The oracle's statuses and recomputed challenges for the edge presentations, then for the same presentations with the
    challenge and every response (main proof and proofs of encryption) replaced by canonical edge scalars (c != 0): the responses
    drive the 13-bit positional windows, the challenge the 4-bit windows and the key's NAF, with digits at their extremes"""
    import oracle
    import aeonflux_amd as afx
    from tests.soa import pack_presentations
    d = world["d"]
    honest = world["pres"]
    forged = [copy.deepcopy(p) for p in honest]
    for i, p in enumerate(forged):
        c = b32(EDGE_NONZERO[i % len(EDGE_NONZERO)])
        for k in range(32):
            p.challenge[k] = c[k]
        for r in range(p.n_responses):
            v = b32(EDGE[(3 * i + r) % len(EDGE)])
            for k in range(32):
                p.responses[r][k] = v[k]
        for e in range(p.n_enc_proofs):
            c = b32(EDGE_NONZERO[(i + 5 * e + 1) % len(EDGE_NONZERO)])
            for k in range(32):
                p.enc[e].challenge[k] = c[k]
            for r in range(6):
                v = b32(EDGE[(5 * i + r + e) % len(EDGE)])
                for k in range(32):
                    p.enc[e].responses[r][k] = v[k]
    cnt = len(honest)
    want = {}
    for name, pres in (("honest", honest), ("forged", forged)):
        sh, soa, keep = pack_presentations(pres)
        st, trace, reached = oracle.verify_presentations_traced(d["issuer"], sh, soa, cnt)
        want[name] = (st.tolist(), trace, reached.astype(bool))
    assert 0 < sum(want["honest"][0]) < cnt          # refused and accepted ones among the edge presentations
    # the forged items whose challenge is recomputed carry every nonzero edge value as their challenge
    reached_main = want["forged"][2][0]
    assert reached_main.sum() > 0.8 * cnt
    assert {EDGE_NONZERO[i % len(EDGE_NONZERO)] for i in np.flatnonzero(reached_main)} == set(EDGE_NONZERO)
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    naf = {}
    for mode in (0, 1):
        ctx.set_secret_independent_addressing(mode)
        for fixed in (False, True):
            ctx.set_fixed_key_schedule(fixed)
            for small in (0, 4096, 16384):   # one chain per job, key job split, one chain per term (test_the_three_plans_agree)
                ctx.set_small_batch_items(small)
                ctx.set_timing(True)
                for name, pres in (("honest", honest), ("forged", forged)):
                    st, trace, reached = want[name]
                    ctx.set_challenge_trace(1 + world["nsp"], cnt)
                    got = gpu_verify(afx, ctx, pres)
                    tr = ctx.get_challenge_trace()
                    ctx.set_challenge_trace(0, 0)
                    assert got == st, (name, mode, fixed, small, [i for i in range(cnt) if got[i] != st[i]][:8])
                    assert np.array_equal(tr[reached], trace[reached]), (name, mode, fixed, small)
                naf[mode, fixed, small] = ctx.get_timing("k_msm_naf")[1]
                ctx.set_timing(False)
    # Z's key terms ran as width-5 NAF schedules in the large-pass plan of mode 0 without the fixed schedule, and nowhere else:
    # a 300-item pass is a small one under the other two limits (no NAF schedules), mode 1 keeps the key out of addresses
    assert naf[0, False, 0] >= 2, naf
    assert all(v == 0 for k, v in naf.items() if k != (0, False, 0)), naf
    ctx.close()
