"""CPU-only: the two yardsticks of the batchable form against each other (tests/batchable_ref.py).  For every committed golden flow
with a presentation: the pure-Python verifier accepts the ORACLE's commitments exactly when the oracle accepts the compact
presentation; pyref's prover hashes the commitments the oracle's verifier recomputes; and the yardstick rejects what it must."""
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
