"""Every cell of every verified record against aliases and swaps, on the device: the swept sections of tests/cell_sweep.py (one honest
record damaged once per (cell, damage): v + l, bit 255, p - v, another record's cell, zeros, one bit; a control after every 16) through
every door that reads them.  The expected status of every record is the yardstick's, computed by tests/test_cell_sweep_ref.py's cases
(the C oracle; tests/batchable_ref.py; tests/blind_ref.py) before the engine is asked - the engine's answer is never the expectation.
A missing canonicity job (k_sccheck) or decode job for ONE row shows as a false accept of that cell's `+l`, `bit255` or `neg` record;
a cell map (records.hpp) that sends two cells to one row, or a cell bound to nothing, as a false accept at `other`.

One test per door, under the default plan and with the small-pass plans switched off (afx_ctx_set_small_batch_items(0)), on one
context per issuer.  A mismatch report names the door, the cell, the field the cell belongs to and the damage."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import cell_sweep as CS
from tests import test_cell_sweep_ref as REF
from tests.test_cell_sweep_ref import C3, RECORD, SMALL

pytestmark = pytest.mark.gpu

PLANS = [4096, 0]          # afx_ctx_set_small_batch_items: the default, and the latency plans off
PLAN_IDS = ["default-plan", "small-batch-0"]
BATCHABLE_SEED = bytes(range(100, 132))


@pytest.fixture(scope="module")
def contexts():
    """one context per (issuer, with or without its key), made when first asked for"""
    import aeonflux_amd as afx
    made = {}

    def get(params, key, ip):
        k = (params, key, ip)
        if k not in made:
            made[k] = afx.Context(params, key, ip)
        return made[k]
    yield get
    for c in made.values():
        c.close()


class plan:
    """the contexts under afx_ctx_set_small_batch_items(items), the default put back afterwards"""

    def __init__(self, items, *ctxs):
        self.items, self.ctxs = items, ctxs

    def __enter__(self):
        for c in self.ctxs:
            c.set_small_batch_items(self.items)

    def __exit__(self, *exc):
        for c in self.ctxs:
            c.set_small_batch_items(4096)


def agree(case, got, want=None, what=""):
    """the door's statuses are the yardstick's, record by record"""
    want = case.want if want is None else want
    got = np.asarray(got)
    assert got.shape == want.shape, (case.door, what, got.shape, want.shape)
    bad = [("%s%s" % (case.describe(k), what), "engine %d" % got[k], "yardstick %d" % want[k]) for k in np.nonzero(got != want)[0]]
    assert not bad, ("%d of %d records" % (len(bad), len(want)), bad[:8])


def with_records(blob, hdr, records):
    """the section's header over other records"""
    h = bytearray(blob[:hdr])
    h[8:12] = struct.pack("<I", records.shape[0])
    return bytes(h) + np.ascontiguousarray(records).tobytes()


# ---- AFXP ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", [SMALL, C3])
def test_afxp_presentations(contexts, name, items):
    from aeonflux_amd import batch, wire
    case = REF.afxp_case(name)
    assert REF.check_stated(case) == []
    w = case.world
    issuer = contexts(w["params"], w["key"], w["ip"])
    with plan(items, issuer):
        agree(case, wire.verify_mixed_wire(issuer, case.s.blob), what=" [afx_verify_presentations_mixed_wire]")
        shape, p = wire.unpack_presentations(case.s.blob)
        agree(case, batch.verify_presentations(issuer, shape, p), what=" [afx_verify_presentations]")


# ---- a proof of encryption alone ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
def test_encryption_proofs_alone(contexts, items):
    import aeonflux_amd as afx
    case = REF.encproof_case()
    assert REF.check_stated(case) == []
    w = case.world
    issuer = contexts(w["params"], w["key"], w["ip"])
    cols = REF.enc_columns(case.s.records)
    soa = afx.EncProofSoA(*(cols[f].ctypes.data for f in REF.ENC_ORDER))
    with plan(items, issuer):
        got = np.full(case.s.count, 255, np.uint8)
        issuer.verify_encryption_proofs(case.index, soa, case.s.count, got.ctypes.data)
    agree(case, got, what=" [afx_verify_encryption_proofs]")


# ---- AFXB ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
def test_afxb_batchable_presentations(contexts, items):
    """under one fixed seed.  (The first of the two runs spends about five seconds in the pure-Python yardstick, 230 records of
    tests/batchable_ref.ref_verify_batchable; the door's call is a few milliseconds, and the second run shares the verdicts.)"""
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    case = REF.afxb_case()
    assert REF.check_stated(case) == []
    w = case.world
    issuer = contexts(w["params"], w["key"], w["ip"])
    assert afx.lib().afx_batchable_main_commitments(issuer.h, C.byref(w["shape"])) == case.n_main
    with plan(items, issuer):
        agree(case, wire.verify_batchable_wire(issuer, case.s.blob, seed=BATCHABLE_SEED), what=" [afx_verify_presentations_batchable_wire]")


# ---- AFXI ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", [SMALL, C3])
def test_afxi_issuances(contexts, name, items):
    from aeonflux_amd import batch, wire
    case = REF.afxi_case(name)
    assert REF.check_stated(case) == []
    d = case.world["d"]
    user = contexts(d["params"], None, d["ip"])
    with plan(items, user):
        agree(case, wire.verify_issuances_stream(user, case.s.blob), what=" [afx_verify_issuances_mixed_wire]")
        kinds, values, iss = wire.unpack_issuances(case.s.blob)
        agree(case, batch.verify_issuances(user, kinds, values, iss), what=" [afx_verify_issuances]")


# ---- AFXR ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
def test_afxr_requests(contexts, items):
    """a request is accepted exactly where the oracle's issue accepts it; the AFXI record of a refused request is all zeros; the record
    of every accepted request, controls included, is byte for byte the oracle's issuance from the same draws.  The oracle has no
    status for an attribute that does not parse (afxo_issue returns -1), so the byte of a refused request is the contract's:
    "undecodable points and non-canonical scalars give what afx_issue gives" (include/aeonflux_gpu.h, afx_issue_wire)."""
    from aeonflux_amd import batch, wire
    case = REF.afxr_case()
    REF.check_stated(case)
    d = case.world["d"]
    issuer = contexts(d["params"], d["key"], d["ip"])
    with plan(items, issuer):
        got, status = wire.issue_wire(issuer, case.s.blob, case.rnd)
        kinds, values = wire.unpack_requests(case.s.blob)
        _, st_col = batch.issue(issuer, kinds, values, case.rnd["t_wide"], case.rnd["U_wide"], case.rnd["rng_seed"])
    agree(case, (status != 0).astype(np.uint8), what=" [afx_issue_wire]")
    agree(case, status, st_col, what=" [afx_issue_wire against afx_issue]")
    hdr, cells, count = CS.layout(got)
    assert count == case.s.count and len(got) == len(case.answer)
    mine, want = (np.frombuffer(b, np.uint8, offset=hdr).reshape(count, cells * 32) for b in (got, case.answer))
    for k in range(count):
        if case.want[k]:
            assert not mine[k].any(), case.describe(k) + ": the record of a refused request is not zeros"
        else:
            assert np.array_equal(mine[k], want[k]), case.describe(k) + ": not the oracle's issuance"
    assert got == case.answer


# ---- AFXQ ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
def test_afxq_blind_requests(contexts, items):
    """afx_verify_blind_requests_wire answers tests/blind_ref.verify_request and afx_issue_blind_wire tests/blind_ref.blind_issue; the two
    agree in every cell of the request proof (a revealed value's cell is read by the issuer alone: "afx_verify_blind_requests on each
    section of the stream", include/aeonflux_gpu.h).  A refused request gets a zero AFXJ record; an accepted one the yardstick's
    issuance from the same draws, which for every record the request proof covers is the undamaged run's."""
    from aeonflux_amd import wire
    case = REF.afxq_case()
    c, s = case.world["c"], case.s
    issuer, user = contexts(c["params"], c["key"], c["ip"]), contexts(c["params"], None, c["ip"])
    honest = with_records(s.blob, s.hdr, np.repeat(s.honest[None], s.count, axis=0))
    with plan(items, issuer, user):
        st_ver = wire.verify_blind_requests_wire(user, s.blob)
        got, st_iss = wire.issue_blind_wire(issuer, s.blob, case.rnd)
        clean, st_clean = wire.issue_blind_wire(issuer, honest, case.rnd)
    agree(case, st_ver, what=" [afx_verify_blind_requests_wire]")
    agree(case, st_iss, case.issue_want, what=" [afx_issue_blind_wire]")
    assert not st_clean.any()
    values = {cell for cell, (f, _) in enumerate(case.fields) if f.startswith("values")}
    hdr, cells, count = CS.layout(got)
    mine, undamaged = (np.frombuffer(b, np.uint8, offset=hdr).reshape(count, cells * 32) for b in (got, clean))
    assert count == s.count
    for k in range(count):
        e = s.entries[k]
        if e is None or e[0] not in values:
            assert st_ver[k] == st_iss[k], case.describe(k) + ": the two doors disagree"
        if case.issue_want[k]:
            assert not mine[k].any(), case.describe(k) + ": the AFXJ record of a refused request is not zeros"
            continue
        iss = case.issued[k]
        assert mine[k].tobytes() == b"".join(iss[f] for f in ("t", "U", "S1", "S2", "challenge")) + b"".join(iss["responses"]), case.describe(k)
        if e is None or e[0] not in values:
            assert np.array_equal(mine[k], undamaged[k]), case.describe(k) + ": not the undamaged run's record"


# ---- AFXJ ----
@pytest.mark.parametrize("items", PLANS, ids=PLAN_IDS)
def test_afxj_blind_issuances(contexts, items):
    """afx_unblind_issuances_wire against the honest AFXQ stream: t, U and V are zeros for the refused and the undamaged run's for the
    rest; one more record, the honest issuance, is unblinded under d + l and refused"""
    from aeonflux_amd import wire
    case = REF.afxj_case()
    assert REF.check_stated(case) == []
    w, s = case.world, case.s
    c = w["c"]
    user = contexts(c["params"], None, c["ip"])
    total = s.count + 1
    q_hdr, q_cells, _ = CS.layout(w["afxq"])
    q_rec = np.frombuffer(w["afxq"], np.uint8, offset=q_hdr).reshape(-1, q_cells, 32)[RECORD]
    requests = with_records(w["afxq"], q_hdr, np.repeat(q_rec[None], total, axis=0))
    swept = with_records(s.blob, s.hdr, np.concatenate([s.records, s.honest[None]]))
    clean = with_records(s.blob, s.hdr, np.repeat(s.honest[None], total, axis=0))
    d = np.repeat(np.frombuffer(case.item["d"], np.uint8)[None], total, axis=0).copy()
    d_bad = d.copy()
    d_bad[-1] = np.frombuffer(case.d_l, np.uint8)
    want = np.concatenate([case.want, [case.d_alias[0]]]).astype(np.uint8)
    with plan(items, user):
        ref, st_ref = wire.unblind_issuances_wire(user, clean, requests, d)
        out, st = wire.unblind_issuances_wire(user, swept, requests, d_bad)
    assert st_ref.tolist() == [0] * total
    flow = w["flows"][RECORD]
    for f, v in (("t", flow[1]["t"]), ("U", flow[1]["U"]), ("V", flow[2])):
        assert all(r.tobytes() == v for r in ref[f]), f          # the undamaged run is the yardstick's credential
    assert st[-1] == want[-1] == 1, "AFXJ: the honest issuance under d + l"
    agree(case, st[:-1], what=" [afx_unblind_issuances_wire]")
    for k in range(total):
        for f in ("t", "U", "V"):
            if want[k]:
                assert not out[f][k].any(), (case.describe(k) if k < s.count else "d + l", f, "not zeros")
            else:
                assert np.array_equal(out[f][k], ref[f][k]), (case.describe(k), f, "not the undamaged run's")
