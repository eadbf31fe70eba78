"""CPU-only: the two yardsticks of the batchable form against each other (tests/batchable_ref.py).  For every committed golden flow
with a presentation: the pure-Python verifier accepts the ORACLE's commitments exactly when the oracle accepts the compact
presentation; pyref's prover hashes the commitments the oracle's verifier recomputes; and the yardstick rejects what it must.

Then the WEIGHTED yardstick (ref_verify_batchable_weighted, the header's one sum under given weights) and the forgeries built to cancel
under one item's weights: they are what they claim - false constraint by constraint, accepted under exactly their own weights, rejected
under any other - before a GPU test leans on them (tests/test_gpu_batchable_weights.py)."""
import hashlib

import pytest

from tests import batchable_ref as B
from tests.helpers import pres_from_json
from tests.pyref import ristretto as R
from tests.pyref import statements as S

H = bytes.fromhex


def _flows_with_presentations(flows):
    import oracle
    for f in flows:
        if "presentation" not in f:
            continue
        params, key, ip = H(f["params"]), H(f["key"]), H(f["issuer_params"])
        yield f, params, key, ip, oracle.Ctx(params, key, ip), pres_from_json(f)


def test_yardstick_accepts_the_oracles_commitments_exactly_when_the_oracle_accepts(flows):
    n = accepted = 0
    for f, params, key, ip, issuer, p in _flows_with_presentations(flows):
        verdict = issuer.verify_presentation(p)
        assert verdict == f["verify"], f["name"]
        cm = B.to_batchable(issuer, p)
        if cm is None:
            assert verdict == 1, f["name"]      # some proof never reached its transcript: nothing to send, and the oracle rejects
        else:
            trace = []
            got = B.ref_verify_batchable(params, key, ip, B.pyref_presentation(p), cm, trace=trace)
            assert got == verdict, f["name"]
            if verdict == 0:
                assert len(trace) == 1 + p.n_enc_proofs
                assert trace[0] == bytes(p.challenge) and [bytes(p.enc[e].challenge) for e in range(p.n_enc_proofs)] == trace[1:], f["name"]
                accepted += 1
        n += 1
    assert n >= 15 and accepted >= 8, (n, accepted)


def test_pyref_show_hashes_the_commitments_the_oracle_recomputes(flows):
    n = 0
    for f, params, key, ip, issuer, p in _flows_with_presentations(flows):
        sh, iss = f.get("show"), f["issue"]
        if not sh or sh["status"] != 0 or f["verify"] != 0:
            continue                             # (a fixture tampered with after show no longer holds what show made)
        kp = H(sh["keypair"]) if sh.get("keypair") else None
        st, q = S.show(params, ip, sh["kinds"], [H(v) for v in sh["values"]], H(iss["t"]), H(iss["U"]), H(iss["V"]), kp, H(sh["z_wide"]),
                       H(sh["rng_seed"]), H(sh["enc_seeds"]))
        assert st == 0
        cm = B.to_batchable(issuer, p)
        assert cm["main"] == q["commitments"], f["name"]
        assert cm["enc"] == [e["commitments"] for e in q["enc"]], f["name"]
        n += 1
    assert n >= 8, n


def test_yardstick_rejects_damaged_commitments_and_unweighted_cancellations(flows):
    """what only a per-constraint check catches: R_0 + D, R_1 - D passes any UNWEIGHTED sum of the constraints"""
    for f, params, key, ip, issuer, p in _flows_with_presentations(flows):
        if f["verify"] != 0:
            continue
        cm = B.to_batchable(issuer, p)
        q = B.pyref_presentation(p)
        assert B.ref_verify_batchable(params, key, ip, q, cm) == 0
        D = R.mul(12345, R.decode(cm["main"][0]))
        shifted = dict(cm, main=[R.encode(R.add(R.decode(cm["main"][0]), D)), R.encode(R.sub(R.decode(cm["main"][1]), D))] + cm["main"][2:])
        assert B.ref_verify_batchable(params, key, ip, q, shifted) == 1
        for bad in (bytes(32), b"\xff" * 32, cm["main"][1]):
            assert B.ref_verify_batchable(params, key, ip, q, dict(cm, main=[bad] + cm["main"][1:])) == 1
        assert B.ref_verify_batchable(params, key, ip, q, dict(cm, main=cm["main"][:-1])) == 1
        if cm["enc"]:
            e0 = list(cm["enc"][0])
            e0[0], e0[1] = e0[1], e0[0]
            assert B.ref_verify_batchable(params, key, ip, q, dict(cm, enc=[e0] + cm["enc"][1:])) == 1
        return
    pytest.fail("no accepted flow among the fixtures")


FORGERY_CASES = [(4, "SSPE", [0, 3], False, [(0, 1), (4, 5), (9, 2)]), (8, "SSPPEEEE", [4, 5, 6, 7], False, [(1, 5), (6, 8), (10, 25)]),
                 (4, "SSPE", [0, 3], True, [(5, 0), (3, 6), (10, 7)])]
SEED, OTHER_SEED, STREAM = hashlib.sha256(b"forgery-seed").digest(), hashlib.sha256(b"forgery-other-seed").digest(), 2 ** 32 + 7


@pytest.mark.parametrize("n,layout,hide,strict,pairs", FORGERY_CASES)
def test_forgeries_cancel_under_their_own_weights_and_under_no_others(n, layout, hide, strict, pairs):
    """a forgery for ordinal i and weight indices a != b: constraints a and b are each false (the per-constraint yardstick rejects),
    the sum under weights(seed, stream, i, M) is the identity, and under the weights of the next ordinal, the next stream, another
    seed, the same weights cut to 64 bits, or with rho_a and rho_b exchanged, it is not"""
    from tests.helpers import make_credentials
    from tests.test_gpu_batchable import _show_inputs
    count = len(pairs) + 1
    d = make_credentials(n, layout, count, b"forgery-cpu-" + layout.encode() + bytes([strict]))
    _, _, x = _show_inputs(d, hide, count)
    args = (d["params"], d["key"], d["ip"])
    honest_p, honest_cm = B.forge(d, x, count - 1, {}, strict=strict)
    n_main = len(honest_cm["main"])
    M = n_main + 5 * len(honest_cm["enc"])
    assert M == {("SSPE", False): 10, ("SSPPEEEE", False): 26, ("SSPE", True): 11}[(layout, strict)]
    q = B.pyref_presentation(honest_p)
    assert B.ref_verify_batchable(*args, q, honest_cm, strict=strict) == 0
    for w in (B.weights(SEED, STREAM, count - 1, M), [1] * M, [0] * M):
        assert B.ref_verify_batchable_weighted(*args, q, honest_cm, w, strict=strict) == 0      # honest: accepted under any weights
    with pytest.raises(ValueError):
        B.ref_verify_batchable_weighted(*args, q, honest_cm, [1] * (M - 1), strict=strict)
    for i, (a, b) in enumerate(pairs):
        assert a < M and b < M
        rho = B.weights(SEED, STREAM, i, M)
        p, cm = B.forge(d, x, i, B.cancelling_shifts(rho, a, b, n_main), strict=strict)
        q = B.pyref_presentation(p)
        for w, (call, j) in ((a, B.constraint_of(a, n_main)), (b, B.constraint_of(b, n_main))):   # the two commitments are not the honest prover's
            h_p, h_cm = (honest_p, honest_cm) if i == count - 1 else B.forge(d, x, i, {}, strict=strict)
            sent = cm["main"][j] if call == 0 else cm["enc"][call - 1][j]
            assert sent != (h_cm["main"][j] if call == 0 else h_cm["enc"][call - 1][j]), w
        assert B.ref_verify_batchable(*args, q, cm, strict=strict) == 1
        assert B.ref_verify_batchable_weighted(*args, q, cm, rho, strict=strict) == 0, (i, a, b)
        cut = [r % 2 ** 64 for r in rho]
        swapped = list(rho)
        swapped[a], swapped[b] = rho[b], rho[a]
        assert cut[a] != rho[a] and cut[b] != rho[b] and rho[a] != rho[b]
        others = dict(next_ordinal=B.weights(SEED, STREAM, i + 1, M), next_stream=B.weights(SEED, STREAM + 1, i, M), other_seed=B.weights(OTHER_SEED, STREAM, i, M),
                      cut_to_64_bits=cut, swapped=swapped, ones=[1] * M)
        for name, w in others.items():
            assert B.ref_verify_batchable_weighted(*args, q, cm, w, strict=strict) == 1, (i, a, b, name)


def test_weighted_yardstick_equals_the_per_constraint_one_on_honest_and_damaged_items():
    from tests.test_gpu_batchable import DAMAGED, damaged_case
    for n, layout, hide, count, seed in DAMAGED[1:3]:
        d, pres, cms, classes, want = damaged_case(n, layout, hide, count, seed)
        assert 4 * want.count(0) >= count and 4 * want.count(1) >= count
        M = len(cms[0]["main"]) + 5 * len(cms[0]["enc"])
        got = []
        for i, (p, cm) in enumerate(zip(pres, cms)):
            if len(cm["main"]) + 5 * len(cm["enc"]) != M:
                pytest.fail("damaged_case changed the number of commitments")
            got.append(B.ref_verify_batchable_weighted(d["params"], d["key"], d["ip"], B.pyref_presentation(p), cm, B.weights(SEED, 1, i, M)))
        assert got == want, [(i, classes[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
