"""CPU-only: the blind-issuance yardstick (tests/blind_ref.py) against itself, tests/pyref and the oracle.  Every layout makes the
round trip request -> verify -> blind issue -> unblind; the unblinded V, t and U are byte for byte what pyref's and the oracle's plain
`issue` make from the same t_wide, U_wide and attribute values (the pin: a blind-issued credential IS the credential the
oracle-pinned path issues); response counts are as specified; every field of a request and of an issuance, damaged alone, is
rejected, and so are two items' rows swapped."""
import hashlib

import pytest

from tests import blind_ref as BR
from tests.pyref import ristretto as R
from tests.pyref import statements as S

# (n, kinds): the four layouts of the issue, n = 8, and n = 16 with 8 hidden positions (its transcripts span several blocks)
LAYOUTS = [(1, [1]), (3, [0, 1, 4]), (4, [4, 2, 3, 1]), (3, [0, 2, 3]), (8, [0, 1, 2, 4, 3, 1, 4, 0]),
           (16, [1, 0, 4, 2, 1, 3, 4, 0, 1, 2, 4, 3, 1, 0, 4, 2])]
_LETTER = {0: "S", 1: "S", 2: "P", 3: "E", 4: "E"}


def make_case(n, kinds, count, seed):
    """count items of one layout: system parameters, key and attribute values from the oracle (tests/helpers.make_credentials), and
    the draws of a blind flow from SHAKE256(seed).  The oracle's own `issue` of the same values and (t_wide, U_wide, seed) is kept."""
    from tests.helpers import make_credentials
    d = make_credentials(n, "".join(_LETTER[k] for k in kinds), count, seed)
    xof = hashlib.shake_256(b"blind draws" + seed).digest(count * (64 * (n + 3) + 64))
    pos = [0]

    def take(k):
        b = xof[pos[0]:pos[0] + k]
        pos[0] += k
        return b
    h = len(BR.hidden_positions(kinds))
    items = []
    for cr in d["creds"]:
        values = [v[:32] for v in cr["values"]]
        st, t, U, V, ch, resp = d["issuer"].issue(kinds, cr["values"], *cr["rnd"])
        assert st == 0
        items.append(dict(values=values, full_values=cr["values"], d=R.sc_bytes(R.sc_from_wide(take(64))), r_wide=[take(64) for _ in range(h)], req_seed=take(32),
                          t_wide=cr["rnd"][0], U_wide=cr["rnd"][1], rprime_wide=take(64), iss_seed=take(32), oracle=dict(t=t, U=U, V=V)))
    return dict(params=d["params"], key=d["key"], ip=d["ip"], n=n, kinds=kinds, items=items, issuer=d["issuer"], user=d["user"], take=d["take"])


def run_flow(case, it):
    """the four steps of one item through the yardstick; returns (request, issuance, V)"""
    kinds = case["kinds"]
    st, req = BR.blind_request(case["params"], kinds, it["values"], it["d"], it["r_wide"], it["req_seed"])
    assert st == S.OK
    assert BR.verify_request(case["params"], kinds, req) == S.OK
    H = BR.hidden_positions(kinds)
    revealed_only = [None if i in H else v for i, v in enumerate(it["values"])]          # the issuer never sees a hidden value
    st, iss = BR.blind_issue(case["params"], case["key"], case["ip"], kinds, revealed_only, req, it["t_wide"], it["U_wide"], it["rprime_wide"], it["iss_seed"])
    assert st == S.OK
    st, V = BR.unblind(case["params"], case["ip"], kinds, it["values"], req, it["d"], iss)
    assert st == S.OK
    return req, iss, V


@pytest.fixture(scope="module")
def cases():
    out = {}
    for n, kinds in LAYOUTS:
        c = make_case(n, kinds, 2 if n <= 4 else 1, b"blind-ref-%d-%s" % (n, bytes(kinds)))
        c["flows"] = [run_flow(c, it) for it in c["items"]]
        out[(n, tuple(kinds))] = c
    return out


@pytest.mark.parametrize("n,kinds", LAYOUTS)
def test_round_trip_and_the_pin(cases, n, kinds):
    c = cases[(n, tuple(kinds))]
    h = len(BR.hidden_positions(kinds))
    hs = sum(1 for k in kinds if k == S.SECRET_SCALAR)
    for it, (req, iss, V) in zip(c["items"], c["flows"]):
        assert len(req["responses"]) == 1 + h + hs == BR.n_request_responses(kinds) and len(req["A"]) == len(req["B"]) == h
        assert len(iss["responses"]) == n + 6
        # the credential the oracle-pinned path issues, from pyref and from the oracle
        st, plain = S.issue(c["params"], c["key"], c["ip"], kinds, it["values"], it["t_wide"], it["U_wide"], it["iss_seed"])
        assert st == S.OK
        for ref in (plain, it["oracle"]):
            assert V == ref["V"] and iss["t"] == ref["t"] and iss["U"] == ref["U"]
        if h:
            assert iss["S2"] != V          # what the issuer sees is not the credential
    # ... and the oracle shows it, hidden positions hidden, and verifies the presentation (the strict statement: the reference's own
    # uses a compact index as a position and rejects layouts such as [4, 2, 3, 1] whoever issued them)
    it, (req, iss, V) = c["items"][0], c["flows"][0]
    nsp = sum(1 for k in kinds if k == 4)
    kp = c["user"].keypair_derive(c["take"](64))
    for ctx in (c["user"], c["issuer"]):
        ctx.set_strict(1)
    st, p = c["user"].show(kinds, it["full_values"], iss["t"], iss["U"], V, kp, c["take"](64), c["take"](32), c["take"](32 * nsp))
    assert st == 0
    verdict = c["issuer"].verify_presentation(p)
    for ctx in (c["user"], c["issuer"]):
        ctx.set_strict(0)
    assert verdict == 0


def _damages(b):
    flipped = bytearray(b)
    flipped[5] ^= 0x10
    return [("bit", bytes(flipped)), ("zeros", bytes(32)), ("ff", b"\xff" * 32)]


def _request_fields(req):
    return [("D", None), ("challenge", None)] + [(f, j) for f in ("A", "B") for j in range(len(req["A"]))] + [("responses", k) for k in range(len(req["responses"]))]


def _issuance_fields(iss):
    return [(f, None) for f in ("t", "U", "S1", "S2", "challenge")] + [("responses", k) for k in range(len(iss["responses"]))]


def _with(rec, f, j, value):
    out = dict(rec)
    if j is None:
        out[f] = value
    else:
        out[f] = list(rec[f])
        out[f][j] = value
    return out


def _get(rec, f, j):
    return rec[f] if j is None else rec[f][j]


@pytest.mark.parametrize("n,kinds", [LAYOUTS[1], LAYOUTS[2]])
def test_every_damaged_field_is_rejected(cases, n, kinds):
    c = cases[(n, tuple(kinds))]
    it, (req, iss, V) = c["items"][0], c["flows"][0]
    it1, (req1, iss1, V1) = c["items"][1], c["flows"][1]
    H = BR.hidden_positions(kinds)
    revealed_only = [None if i in H else v for i, v in enumerate(it["values"])]
    for f, j in _request_fields(req):
        for what, value in _damages(_get(req, f, j)) + [("swapped", _get(req1, f, j))]:
            bad = _with(req, f, j, value)
            assert BR.verify_request(c["params"], kinds, bad) == S.VERIFICATION_FAILURE, (f, j, what)
            if what in ("bit", "swapped"):      # the issuer gives the same verdict and releases nothing
                st, out = BR.blind_issue(c["params"], c["key"], c["ip"], kinds, revealed_only, bad, it["t_wide"], it["U_wide"], it["rprime_wide"], it["iss_seed"])
                assert (st, out) == (S.VERIFICATION_FAILURE, None), (f, j, what)
    for f, j in _issuance_fields(iss):
        for what, value in _damages(_get(iss, f, j)) + [("swapped", _get(iss1, f, j))]:
            st, out = BR.unblind(c["params"], c["ip"], kinds, it["values"], req, it["d"], _with(iss, f, j, value))
            assert (st, out) == (S.VERIFICATION_FAILURE, None), (f, j, what)
    # the user's own side: another item's d, request or attribute values do not open this issuance
    assert BR.unblind(c["params"], c["ip"], kinds, it["values"], req1, it["d"], iss)[0] == S.VERIFICATION_FAILURE
    revealed = [i for i in range(n) if i not in H]
    if revealed:
        other = list(it["values"])
        other[revealed[0]] = it1["values"][revealed[0]]
        assert BR.unblind(c["params"], c["ip"], kinds, other, req, it["d"], iss)[0] == S.VERIFICATION_FAILURE
    st, V_wrong = BR.unblind(c["params"], c["ip"], kinds, it["values"], req, it1["d"], iss)
    assert st == S.OK and V_wrong != V          # d is not in the issuer's proof: a wrong d only yields a V that is no MAC


def test_request_refuses_malformed_inputs_and_whole_shapes(cases):
    n, kinds = LAYOUTS[1]
    c = cases[(n, tuple(kinds))]
    it, (req, iss, V) = c["items"][0], c["flows"][0]
    ff = b"\xff" * 32
    args = lambda values=it["values"], d=it["d"], k=kinds: BR.blind_request(c["params"], k, values, d, it["r_wide"][:len(BR.hidden_positions(k))], it["req_seed"])
    assert args(d=ff)[0] == S.MAC_CREATION
    assert args(d=bytes(32))[0] == S.MAC_CREATION                       # D would be the identity
    for i in range(n):
        v = list(it["values"])
        v[i] = ff
        assert args(values=v)[0] == S.MAC_CREATION, i
    assert args(k=kinds[:-1])[0] == S.MAC_CREATION
    assert BR.verify_request(c["params"], kinds[:-1], req) == S.VERIFICATION_FAILURE
    assert BR.blind_issue(c["params"], c["key"], c["ip"], kinds[:-1], it["values"], req, it["t_wide"], it["U_wide"], it["rprime_wide"], it["iss_seed"])[0] == S.MAC_CREATION
    assert BR.unblind(c["params"], c["ip"], kinds[:-1], it["values"], req, it["d"], iss)[0] == S.VERIFICATION_FAILURE
    short = dict(req, responses=req["responses"][:-1])
    assert BR.verify_request(c["params"], kinds, short) == S.VERIFICATION_FAILURE
    assert BR.unblind(c["params"], c["ip"], kinds, it["values"], req, it["d"], dict(iss, responses=iss["responses"][:-1]))[0] == S.VERIFICATION_FAILURE
    # a malformed revealed value fails the item at the issuer
    v = [ff if i == 0 else x for i, x in enumerate(it["values"])]
    assert BR.blind_issue(c["params"], c["key"], c["ip"], kinds, v, req, it["t_wide"], it["U_wide"], it["rprime_wide"], it["iss_seed"])[0] == S.VERIFICATION_FAILURE
