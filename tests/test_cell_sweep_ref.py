"""CPU-only: what the yardsticks say of one honest record of every wire format damaged once per (cell, damage) (tests/cell_sweep.py).
No engine is used: the swept sections are unpacked with aeonflux_amd.wire's unpack_* functions (byte shuffling) and given to the C
oracle (AFXP, AFXI, AFXR, a proof of encryption alone) or to the pure-Python yardsticks (AFXB tests/batchable_ref.py; AFXQ, AFXJ
tests/blind_ref.py).  Stated here, before any engine is asked:

  - every control is accepted;
  - `+l` is refused in every cell that holds a scalar the statement reads;
  - `bit255` and `neg` are refused in every cell that holds a point;
  - the cells a yardstick accepts damaged are printed (a value cell whose `other` is one more honest value, for instance).

The cases and verdicts of this module are the expectations of tests/test_gpu_cell_sweep.py: nothing the engine returns ever is."""
import functools
import hashlib

import numpy as np
import pytest

from tests import cell_sweep as CS

SMALL = "small"          # S S P E, positions 0 and 3 hidden
C3 = "c3"                # S S P P E E E E, the second scalar and the four plaintext attributes hidden: 4 responses, 4 proofs of encryption
LAYOUTS = {SMALL: (4, "SSPE", [0, 3]), C3: (8, "SSPPEEEE", [1, 4, 5, 6, 7])}
BLIND_KINDS = [1, 0, 2, 4]          # the small layout as a blind request: AFX_ATTR_* with positions 0 and 3 hidden
RECORD = 0                          # the honest record that is swept; `other` takes its cells from record 1


class Case:
    """one door's sweep: s (cell_sweep.Sweep), fields [(name, 's' | 'p')] per cell, want [count] the yardstick's status per record,
    and whatever the door's test needs beyond (keys, honest inputs, the yardstick's outputs)"""

    def __init__(self, door, s, fields, want, **more):
        self.door, self.s, self.fields, self.want = door, s, fields, np.asarray(want, np.uint8)
        assert len(fields) == s.cells and len(self.want) == s.count
        self.__dict__.update(more)

    def describe(self, k):
        return CS.describe(self.door, [f for f, _ in self.fields], self.s.entries[k])

    def numbers(self):
        """cells swept, records sent, records the yardstick refused, controls accepted"""
        return (self.s.cells, self.s.count, int((self.want != 0).sum()), sum(1 for k in self.s.controls if self.want[k] == 0))


def check_stated(case):
    """the statements of this module's docstring about one case; returns the damaged records the yardstick accepts"""
    s, want = case.s, case.want
    assert len(s.damaged) == s.cells * len(CS.DAMAGES)
    for k in s.controls:
        assert want[k] == 0, case.describe(k)
    for k in s.damaged:
        cell, damage = s.entries[k]
        kind = case.fields[cell][1]
        if (damage == "+l" and kind == "s") or (damage in ("bit255", "neg") and kind == "p"):
            assert want[k] != 0, case.describe(k)
    accepted = [k for k in s.damaged if want[k] == 0]
    print("%s: cells %d, records %d, refused %d, controls accepted %d" % ((case.door,) + case.numbers()))
    for k in accepted:
        print("  accepted damaged: " + case.describe(k))
    return accepted


def _draws(label, count, width):
    return np.frombuffer(hashlib.shake_256(b"cell-sweep draws " + label).digest(count * width), np.uint8).reshape(count, width).copy()


# ---- AFXP, and a proof of encryption alone ----
@functools.lru_cache(maxsize=None)
def presentations(name):
    """two honest presentations of a layout from the oracle: dict(params, key, ip, issuer, shape, arrays, blob)"""
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    from tests.helpers import make_batch
    from tests.soa import presentation_arrays, shape_of
    n, layout, hide = LAYOUTS[name]
    params, key, ip, issuer, pres = make_batch(n, layout, hide, 2, b"cell-sweep-afxp-" + name.encode())
    shape = afx.Shape.from_buffer_copy(bytes(shape_of(pres[0])))
    a = presentation_arrays(pres)
    return dict(params=params, key=key, ip=ip, issuer=issuer, shape=shape, arrays=a, blob=wire.pack_presentations(shape, a), pres=pres)


def oracle_verify_presentations(issuer, blob):
    import oracle
    from aeonflux_amd import batch, wire
    shape, p = wire.unpack_presentations(blob)
    soa, keep = batch.presentation_soa(p)
    st, _, _ = oracle.verify_presentations_traced(issuer, shape, soa, p["challenge"].shape[0])
    return st


@functools.lru_cache(maxsize=None)
def afxp_case(name):
    w = presentations(name)
    s = CS.sweep(w["blob"], RECORD)
    return Case("AFXP " + name, s, CS.presentation_fields(w["shape"]), oracle_verify_presentations(w["issuer"], s.blob), world=w)


ENC_ORDER = ("challenge", "responses", "pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p")


def enc_columns(rec):
    """records [count, 14, 32] of one proof of encryption -> its nine fields as columns"""
    c = lambda a: np.ascontiguousarray(a)
    d = {"challenge": c(rec[:, 0]), "responses": c(rec[:, 1:7].transpose(1, 0, 2))}
    d.update({f: c(rec[:, 7 + k]) for k, f in enumerate(ENC_ORDER[2:])})
    return d


@functools.lru_cache(maxsize=None)
def encproof_case():
    """the first proof of encryption of the small layout's presentations, alone: nine fields, 14 cells"""
    import oracle
    w = presentations(SMALL)
    d = w["arrays"]["enc"][0]
    rec = np.concatenate([d["challenge"][:, None], d["responses"].transpose(1, 0, 2)] + [d[f][:, None] for f in ENC_ORDER[2:]], axis=1)
    s = CS.sweep_records(np.ascontiguousarray(rec), RECORD)
    index = w["shape"].enc_indices[0]
    want = []
    for r in s.records:
        e = oracle.EncProof.from_buffer_copy(r.tobytes() + index.to_bytes(2, "little"))
        want.append(w["issuer"].verify_encryption_proof(e))
    fields = [("enc." + f, t) for f, t in zip(CS.ENC_FIELDS, CS.ENC_TYPES)]
    return Case("proof of encryption", s, fields, want, world=w, index=index)


# ---- AFXI, AFXR ----
@functools.lru_cache(maxsize=None)
def credentials(name):
    """two oracle-issued credentials of a layout, as the request and issuance sections"""
    from aeonflux_amd import wire
    from tests.helpers import make_credentials
    n, layout, _ = LAYOUTS[name]
    d = make_credentials(n, layout, 2, b"cell-sweep-afxi-" + name.encode())
    cr = d["creds"]
    kinds = cr[0]["kinds"]
    values = np.frombuffer(b"".join(c["values"][i][:32] for i in range(n) for c in cr), np.uint8).reshape(n, 2, 32)
    iss = {f: np.frombuffer(b"".join(c[f] for c in cr), np.uint8).reshape(2, 32) for f in ("t", "U", "V", "challenge")}
    iss["responses"] = np.frombuffer(b"".join(c["responses"][k] for k in range(n + 5) for c in cr), np.uint8).reshape(n + 5, 2, 32)
    return dict(d=d, kinds=kinds, values=values, afxi=wire.pack_issuances(kinds, values, iss), afxr=wire.pack_requests(kinds, values))


def oracle_verify_issuances(user, blob):
    import oracle
    from aeonflux_amd import wire
    kinds, values, iss = wire.unpack_issuances(blob)
    st, _, _ = oracle.verify_issuances_traced(user, kinds, values, iss)
    return st


@functools.lru_cache(maxsize=None)
def afxi_case(name):
    w = credentials(name)
    s = CS.sweep(w["afxi"], RECORD)
    return Case("AFXI " + name, s, CS.issuance_fields(w["kinds"], len(w["kinds"]) + 5), oracle_verify_issuances(w["d"]["user"], s.blob), world=w)


@functools.lru_cache(maxsize=None)
def afxr_case():
    """the small layout's requests; every swept request has draws of its own.  want: 0 where the oracle's issue accepts the request,
    1 where it refuses it (an attribute that does not parse is no request to the oracle: afxo_issue returns -1, not a status of the
    reference).  answer: the AFXI section the oracle's issue makes of the swept requests, the record of a refused request all zeros"""
    import oracle
    from aeonflux_amd import wire
    w = credentials(SMALL)
    s = CS.sweep(w["afxr"], RECORD)
    rnd = {"t_wide": _draws(b"afxr t", s.count, 64), "U_wide": _draws(b"afxr U", s.count, 64), "rng_seed": _draws(b"afxr seed", s.count, 32)}
    kinds, values = wire.unpack_requests(s.blob)
    o, st = oracle.issue_soa(w["d"]["issuer"], kinds, values, rnd["t_wide"], rnd["U_wide"], rnd["rng_seed"])
    for f in o:
        o[f][..., st != 0, :] = 0
    values = values.copy()
    values[:, st != 0] = 0
    assert set(st.tolist()) <= {0, 255}          # (255: the byte of -1)
    return Case("AFXR", s, CS.request_fields(kinds), (st != 0).astype(np.uint8), world=w, rnd=rnd, answer=wire.pack_issuances(kinds, values, o))


# ---- AFXB ----
def pyref_items(shape, p, cm):
    """the records of an unpacked AFXB section as tests/batchable_ref's pairs (presentation dict, commitments dict)"""
    n, count = shape.n_attributes, p["responses"].shape[1]
    b = lambda a: a.tobytes()
    out = []
    for i in range(count):
        q = dict(kinds=[shape.kinds[k] for k in range(n)], attr_values=[b(p["attr_values"][k, i]) for k in range(n)],
                 hidden_scalar_indices=[shape.hidden_scalar_indices[k] for k in range(shape.n_hidden_scalars)], challenge=bytes(32),
                 responses=[b(r[i]) for r in p["responses"]], C_x_0=b(p["C_x_0"][i]), C_x_1=b(p["C_x_1"][i]), C_V=b(p["C_V"][i]),
                 C_y=[b(p["C_y"][k, i]) for k in range(n)],
                 enc=[dict(index=shape.enc_indices[e], challenge=bytes(32), responses=[b(d["responses"][k, i]) for k in range(6)],
                           **{f: b(d[f][i]) for f in ENC_ORDER[2:]}) for e, d in enumerate(p["enc"])])
        out.append((q, dict(main=[b(r[i]) for r in cm["main"]], enc=[[b(r[i]) for r in c] for c in cm["enc"]])))
    return out


@functools.lru_cache(maxsize=None)
def afxb_case():
    """the small layout, every challenge replaced by the oracle's commitments (tests/batchable_ref.to_batchable)"""
    from aeonflux_amd import wire
    from tests import batchable_ref as B
    w = presentations(SMALL)
    cm = B.arrays_of([B.to_batchable(w["issuer"], p) for p in w["pres"]])
    n_main = cm["main"].shape[0]
    s = CS.sweep(wire.pack_batchable(w["shape"], w["arrays"], cm), RECORD)
    want = [B.ref_verify_batchable(w["params"], w["key"], w["ip"], q, c) for q, c in pyref_items(*wire.unpack_batchable(s.blob))]
    return Case("AFXB", s, CS.batchable_fields(w["shape"], n_main), want, world=w, n_main=n_main)


# ---- AFXQ, AFXJ ----
@functools.lru_cache(maxsize=None)
def blind_world():
    """two items of the small layout through the yardstick's blind flow: the honest AFXQ and AFXJ sections and the user's secrets"""
    from aeonflux_amd import wire
    from tests.test_blind_ref import make_case, run_flow
    c = make_case(4, BLIND_KINDS, 2, b"cell-sweep-blind")
    flows = [run_flow(c, it) for it in c["items"]]
    col = lambda rows: np.stack([np.frombuffer(r, np.uint8) for r in rows])
    rep = lambda recs, f: np.stack([col([r[f][k] for r in recs]) for k in range(len(recs[0][f]))])
    reqs, isss = [f[0] for f in flows], [f[1] for f in flows]
    req = dict(D=col([r["D"] for r in reqs]), challenge=col([r["challenge"] for r in reqs]), A=rep(reqs, "A"), B=rep(reqs, "B"), responses=rep(reqs, "responses"))
    iss = {f: col([r[f] for r in isss]) for f in ("t", "U", "S1", "S2", "challenge")}
    iss["responses"] = rep(isss, "responses")
    values = np.stack([col([it["values"][i] for it in c["items"]]) for i in range(4)])
    return dict(c=c, flows=flows, values=values, afxq=wire.pack_blind_requests(BLIND_KINDS, values, req), afxj=wire.pack_blind_issuances(BLIND_KINDS, iss))


def item_of(rec, i):
    return {f: (v[i].tobytes() if v.ndim == 2 else [row[i].tobytes() for row in v]) for f, v in rec.items()}


@functools.lru_cache(maxsize=None)
def afxq_case():
    """want: tests/blind_ref.verify_request per swept request (the request proof alone: what afx_verify_blind_requests_wire answers);
    issue_want and issued: status and issuance of tests/blind_ref.blind_issue, which reads the revealed values as well"""
    from aeonflux_amd import wire
    from tests import blind_ref as BR
    w = blind_world()
    c, it = w["c"], w["c"]["items"][RECORD]
    s = CS.sweep(w["afxq"], RECORD)
    kinds, values, req = wire.unpack_blind_requests(s.blob)
    H = BR.hidden_positions(kinds)
    rnd = {"t_wide": _draws(b"afxq t", s.count, 64), "U_wide": _draws(b"afxq U", s.count, 64), "rprime_wide": _draws(b"afxq r'", s.count, 64),
           "rng_seed": _draws(b"afxq seed", s.count, 32)}
    want, issue_want, issued = [], [], []
    for k in range(s.count):
        r = item_of(req, k)
        want.append(BR.verify_request(c["params"], kinds, r))
        vals = [None if i in H else values[i, k].tobytes() for i in range(4)]
        st, out = BR.blind_issue(c["params"], c["key"], c["ip"], kinds, vals, r, *(rnd[f][k].tobytes() for f in ("t_wide", "U_wide", "rprime_wide", "rng_seed")))
        issue_want.append(st)
        issued.append(out)
    return Case("AFXQ", s, CS.blind_request_fields(kinds), want, world=w, rnd=rnd, issue_want=np.asarray(issue_want, np.uint8), issued=issued, item=it)


@functools.lru_cache(maxsize=None)
def afxj_case():
    """want and V: tests/blind_ref.unblind of every swept issuance against the user's own request, values and d; d_alias: the verdict
    on the honest issuance under d + l"""
    from aeonflux_amd import wire
    from tests import blind_ref as BR
    w = blind_world()
    c, it, req = w["c"], w["c"]["items"][RECORD], w["flows"][RECORD][0]
    s = CS.sweep(w["afxj"], RECORD)
    kinds, iss = wire.unpack_blind_issuances(s.blob)
    out = [BR.unblind(c["params"], c["ip"], kinds, it["values"], req, it["d"], item_of(iss, k)) for k in range(s.count)]
    d_l = (int.from_bytes(it["d"], "little") + CS.L).to_bytes(32, "little")
    d_alias = BR.unblind(c["params"], c["ip"], kinds, it["values"], req, d_l, item_of(iss, s.count - 1))
    return Case("AFXJ", s, CS.blind_issuance_fields(len(kinds) + 6), [st for st, _ in out], world=w, V=[v for _, v in out], d_alias=d_alias, d_l=d_l, item=it)


# ---- the statements ----
def test_the_sweep_damages_every_cell_six_times_and_keeps_controls():
    s = afxi_case(SMALL).s
    assert s.cells == 4 + 9 + 4 and len(s.damaged) == s.cells * 6 and s.entries[16] is None and s.entries[-1] is None
    rec = s.records
    for k, e in enumerate(s.entries):
        changed = [c for c in range(s.cells) if not np.array_equal(rec[k, c], s.honest[c])]
        assert changed == ([] if e is None else [e[0]]), k
    v = lambda k, c: int.from_bytes(rec[k, c].tobytes(), "little")
    h = lambda c: int.from_bytes(s.honest[c].tobytes(), "little")
    for c in (0, 5, s.cells - 1):
        assert v(s.of("+l")[c], c) == h(c) + CS.L and v(s.of("bit255")[c], c) == h(c) + 2 ** 255 and v(s.of("neg")[c], c) == CS.P - h(c)
        assert v(s.of("zero")[c], c) == 0 and bin(v(s.of("bit")[c], c) ^ h(c)).count("1") == 1


@pytest.mark.parametrize("name", [SMALL, C3])
def test_afxp_oracle(name):
    case = afxp_case(name)
    accepted = check_stated(case)
    assert case.numbers()[0] == {SMALL: 1 + 4 + 3 + 4 + 2 + 14, C3: 1 + 4 + 3 + 8 + 3 + 4 * 14}[name]
    assert accepted == []          # every cell of a presentation is bound: the oracle refuses all six damages everywhere


def test_encryption_proof_alone_oracle():
    case = encproof_case()
    assert check_stated(case) == [] and case.s.cells == 14


@pytest.mark.parametrize("name", [SMALL, C3])
def test_afxi_oracle(name):
    case = afxi_case(name)
    assert check_stated(case) == []


def test_afxr_oracle_issue():
    """a request is attribute values alone: whatever is a canonical scalar or a decodable point is a request, so `other`, `bit` and `zero`
    may be issued; the aliases (+l in a scalar, bit255 and neg in a point) may not"""
    case = afxr_case()
    accepted = check_stated(case)
    assert {case.s.entries[k][1] for k in accepted} <= {"other", "bit", "zero"}
    assert all(case.s.entries[k][1] != "other" or case.want[k] == 0 for k in case.s.damaged)


def test_afxb_batchable_ref():
    """the whole sweep runs through tests/batchable_ref.ref_verify_batchable (about 0.1 s a record)"""
    case = afxb_case()
    assert check_stated(case) == []


def test_afxq_blind_ref():
    """verify_request reads the request proof alone, so every damage of a revealed value's cell is accepted by it; blind_issue reads the
    values too and refuses whatever is no canonical scalar and no point there - and issues, for another honest value, another credential"""
    case = afxq_case()
    accepted = check_stated(Case(case.door + " (blind_issue)", case.s, case.fields, case.issue_want))
    values = [c for c, (f, _) in enumerate(case.fields) if f.startswith("values")]
    assert all(case.s.entries[k][0] in values and case.s.entries[k][1] in ("other", "bit", "zero") for k in accepted)
    for k in case.s.damaged:
        cell = case.s.entries[k][0]
        assert case.want[k] == (0 if cell in values else 1), case.describe(k)
        assert cell in values or case.issue_want[k] == 1, case.describe(k)
    assert all(case.want[k] == 0 for k in case.s.controls)
    print("%s (verify_request): cells %d, records %d, refused %d, controls accepted %d" % ((case.door,) + case.numbers()))


def test_afxj_blind_ref():
    case = afxj_case()
    assert check_stated(case) == []
    assert case.d_alias == (1, None)          # d + l is no scalar: nothing is unblinded
    honest_V = case.world["flows"][RECORD][2]
    assert all(case.V[k] == honest_V for k in case.s.controls)
