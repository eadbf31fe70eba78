"""GPU: the user side of the protocol on bytes.  afx_verify_issuances_mixed_wire takes the AFXI stream afx_issue_wire writes and must
give what afx_verify_issuances_wire gives section by section; afx_show_wire writes AFXP sections that equal afx_show_mixed +
afx_wire_pack_presentations for every item that succeeded (zeros for the others), the oracle's presentations byte for byte, and verify
on the issuer's side.  Then the whole loop on bytes - AFXR -> issue_wire -> verify -> show_wire -> verify_mixed_wire - and the edges:
size queries, short buffers, refused groups, many passes on both lanes, one-item calls of 32 threads, and a group of devices."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from tests.helpers import make_credentials

pytestmark = pytest.mark.gpu

N = 4
SEED = b"gpu-user-wire"
ENC = ("challenge", "responses", "pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p")


def col(items, f):
    return np.stack([np.frombuffer(f(c), np.uint8) for c in items])


@functools.lru_cache(maxsize=None)
def world(layout, count):
    """count oracle-issued credentials of one layout (every layout under the same parameters and issuer key)"""
    return make_credentials(N, layout, count, SEED)


def request_columns(d):
    cr = d["creds"]
    values = np.stack([col(cr, lambda c, i=i: c["values"][i][:32]) for i in range(N)])
    rnd = {k: col(cr, lambda c, j=j: c["rnd"][j]) for j, k in enumerate(("t_wide", "U_wide", "rng_seed"))}
    return cr[0]["kinds"], values, rnd


def show_item(d, hide, lo=0, hi=None, keys=True, seed_tag=b""):
    """a show_mixed item over credentials [lo, hi) of world d with positions `hide` hidden, and the randomness as oracle inputs"""
    import hashlib
    cr = d["creds"][lo:hi]
    kinds = list(cr[0]["kinds"])
    for i in hide:
        kinds[i] = 1 if kinds[i] == 0 else 4
    nsp = sum(1 for k in kinds if k == 4)
    s = hashlib.shake_256(SEED + seed_tag + bytes(kinds) + bytes([lo])).digest(len(cr) * (64 + 64 + 32 + 32 * nsp))
    take = iter(range(0, len(s), 32))
    nxt = lambda k: b"".join(s[o:o + 32] for o in [next(take) for _ in range(k // 32)])
    kps = [d["user"].keypair_derive(nxt(64)) for _ in cr]
    zw, sd, es = [nxt(64) for _ in cr], [nxt(32) for _ in cr], [nxt(32 * nsp) for _ in cr]
    item = dict(kinds=kinds, values=np.stack([col(cr, lambda c, i=i: c["values"][i][:32]) for i in range(N)]),
                M2=np.stack([col(cr, lambda c, i=i: c["values"][i][32:64]) for i in range(N)]),
                m3=np.stack([col(cr, lambda c, i=i: c["values"][i][64:96]) for i in range(N)]),
                t=col(cr, lambda c: c["t"]), U=col(cr, lambda c: c["U"]), V=col(cr, lambda c: c["V"]),
                keypairs={f: np.stack([np.frombuffer(k[32 * j:32 * j + 32], np.uint8) for k in kps]) for j, f in enumerate(("a", "a0", "a1", "pk"))} if keys else None,
                z_wide=np.stack([np.frombuffer(z, np.uint8) for z in zw]), rng_seed=np.stack([np.frombuffer(x, np.uint8) for x in sd]),
                enc_seeds=np.stack([np.stack([np.frombuffer(e[32 * j:32 * j + 32], np.uint8) for e in es]) for j in range(nsp)]) if nsp else None)
    return item, (kinds, cr, kps, zw, sd, es)


def take_items(it, idx):
    """the credentials idx of a show item (arrays with the item axis first, or second for [k][count][32] rows)"""
    out = {}
    for k, v in it.items():
        if k == "kinds" or v is None:
            out[k] = v
        elif k == "keypairs":
            out[k] = {f: np.ascontiguousarray(a[idx]) for f, a in v.items()}
        elif k in ("values", "M2", "m3", "enc_seeds"):
            out[k] = np.ascontiguousarray(v[:, idx])
        else:
            out[k] = np.ascontiguousarray(v[idx])
    return out


def afxi_with(sec, idx):
    """an AFXI section (n = 4: 32-byte header) made of the records idx of another one"""
    rec = np.frombuffer(sec, np.uint8, offset=32).reshape(-1, (4 + 9 + N) * 32)
    return sec[:8] + np.uint32(len(idx)).tobytes() + sec[12:32] + rec[idx].tobytes()


def oracle_record(pr):
    """one ProofOfValidCredential of the oracle as an AFXP record"""
    n = pr.n_attributes
    r = bytes(pr.challenge) + b"".join(bytes(pr.responses[k]) for k in range(pr.n_responses)) + bytes(pr.C_x_0) + bytes(pr.C_x_1) + bytes(pr.C_V)
    r += b"".join(bytes(pr.C_y[k]) for k in range(n)) + b"".join(bytes(pr.attr_values[k]) for k in range(n) if pr.kinds[k] in (0, 2))
    for e in range(pr.n_enc_proofs):
        q = pr.enc[e]
        r += bytes(q.challenge) + b"".join(bytes(q.responses[k]) for k in range(6)) + b"".join(bytes(getattr(q, f)) for f in ENC[2:])
    return r


def sections_of(blob, measure):
    out, off = [], 0
    while off < len(blob):
        sl = measure(blob[off:])
        out.append(blob[off:off + sl])
        off += sl
    return out


def afxp_sections(blob):
    import aeonflux_amd as afx
    def measure(b):
        n = C.c_size_t(0)
        afx.check(afx.lib().afx_wire_section_bytes(b, len(b), C.byref(n)))
        return n.value
    return sections_of(blob, measure)


def afxp_records(sec):
    import aeonflux_amd as afx
    shape, cnt, off = afx.Shape(), C.c_size_t(0), C.c_size_t(0)
    afx.check(afx.lib().afx_wire_parse(sec, len(sec), C.byref(shape), C.byref(cnt), C.byref(off)))
    cells = afx.lib().afx_wire_cells_per_record(C.byref(shape))
    return shape, np.frombuffer(sec, np.uint8, offset=off.value).reshape(cnt.value, cells * 32)


def mixed_then_pack(ctx, items):
    """today's user path: afx_show_mixed on columns, then afx_wire_pack_presentations per group (C)"""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    outs, status = batch.show_mixed(ctx, items)
    blob = b""
    for o, shape in outs:
        soa, keep = batch.presentation_soa(o)
        cnt, n = o["challenge"].shape[0], C.c_size_t(0)
        afx.check(afx.lib().afx_wire_pack_presentations(C.byref(shape), C.byref(soa), cnt, None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        afx.check(afx.lib().afx_wire_pack_presentations(C.byref(shape), C.byref(soa), cnt, buf.ctypes.data, buf.size, C.byref(n)))
        blob += buf.tobytes()
    return blob, [s for _, s in outs], status


def issuer_ctx(d):
    import aeonflux_amd as afx
    return afx.Context(d["params"], d["key"], d["ip"])


def user_ctx(d):
    import aeonflux_amd as afx
    return afx.Context(d["params"], None, d["ip"])


# ---- 1. stream statuses ------------------------------------------------------------------------------------------------------------
def issued_stream():
    """an AFXI stream from afx_issue_wire: a layout repeated apart, an n-mismatched section, count-1 sections"""
    from aeonflux_amd import wire
    a, b, c = world("SSPE", 12), world("PPPP", 5), world("SEEP", 2)
    ka, va, ra = request_columns(a)
    kb, vb, rb = request_columns(b)
    kc, vc, rc = request_columns(c)
    sl = lambda r, lo, hi: {k: v[lo:hi] for k, v in r.items()}
    z = lambda k: {"t_wide": np.zeros((k, 64), np.uint8), "U_wide": np.zeros((k, 64), np.uint8), "rng_seed": np.zeros((k, 32), np.uint8)}
    parts = [(ka, va[:, :8], sl(ra, 0, 8)), (kb, vb, rb), ([0, 0, 2], va[:3, :2], z(2)), (ka, va[:, 8:11], sl(ra, 8, 11)), (kc, vc[:, :1], sl(rc, 0, 1)),
             (ka, va[:, 11:12], sl(ra, 11, 12))]
    stream = b"".join(wire.pack_requests(k, v) for k, v, _ in parts)
    rnd = {k: np.concatenate([r[k] for _, _, r in parts]) for k in ("t_wide", "U_wide", "rng_seed")}
    ctx = issuer_ctx(a)
    got, status = wire.issue_wire(ctx, stream, rnd)
    ctx.close()
    return a, got, status


def test_stream_statuses_equal_the_per_section_calls_and_tampering_moves_only_its_items():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    a, got, issued = issued_stream()
    assert issued.tolist() == [0] * 13 + [afx.ST_MAC_CREATION] * 2 + [0] * 5
    user = user_ctx(a)
    secs = sections_of(got, wire.issuance_section_bytes)
    assert [wire.unpack_issuances(s)[2]["t"].shape[0] for s in secs] == [8, 5, 2, 3, 1, 1]
    per_section = np.concatenate([user.verify_issuances_wire(s) for s in secs])
    status = wire.verify_issuances_stream(user, got)
    assert status.tolist() == per_section.tolist()
    assert status.tolist() == [0] * 13 + [status[13], status[14]] + [0] * 5 and status[13] != 0 and status[14] != 0
    # one byte each in U, a challenge, a response and an attribute value of chosen records; the oracle's verdict for exactly those
    bad = bytearray(got)
    offs = np.cumsum([0] + [len(s) for s in secs])
    flips = []   # (stream item, section, record, the credential it came from)
    origin = {0: (world("SSPE", 12), 0), 1: (world("PPPP", 5), 0), 3: (world("SSPE", 12), 8), 4: (world("SEEP", 2), 0), 5: (world("SSPE", 12), 11)}
    for item, sec, rec, cell, byte in ((2, 0, 2, 1, 5), (9, 1, 1, 3, 0), (16, 3, 1, 4 + 6, 9), (18, 4, 0, 4 + 9 + 2, 3), (19, 5, 0, 0, 31)):
        kinds, _, _ = wire.unpack_issuances(secs[sec])
        cells = 4 + 9 + len(kinds)
        at = offs[sec] + 32 + rec * cells * 32 + cell * 32 + byte
        bad[at] ^= 0x10
        flips.append((item, sec, rec, origin[sec][0]["creds"][origin[sec][1] + rec]))
    bad = bytes(bad)
    got2 = wire.verify_issuances_stream(user, bad)
    bsecs = sections_of(bad, wire.issuance_section_bytes)
    assert got2.tolist() == np.concatenate([user.verify_issuances_wire(s) for s in bsecs]).tolist()
    want = status.copy()
    for item, sec, rec, cred in flips:
        kinds, values, iss = wire.unpack_issuances(bsecs[sec])
        vals = [values[k, rec].tobytes() + cred["values"][k][32:] for k in range(len(kinds))]
        want[item] = a["user"].issuance_verify(kinds, vals, *(iss[f][rec].tobytes() for f in ("t", "U", "V", "challenge")),
                                               [iss["responses"][k, rec].tobytes() for k in range(9)])
        assert want[item] != 0, item
    assert got2.tolist() == want.tolist()
    user.close()


# ---- 2. show bytes -----------------------------------------------------------------------------------------------------------------
def show_items():
    specs = [("SSPE", [0, 3], 0, 6, True), ("PPPP", [], 0, 3, True), ("SEEP", [1, 2], 0, 1, True), ("SSPE", [0], 6, 7, True), ("SEEP", [2], 1, 2, False),
             ("SSPE", [3], 7, 10, True)]
    items, metas = [], []
    for layout, hide, lo, hi, keys in specs:
        it, meta = show_item(world(layout, 12 if layout == "SSPE" else 5 if layout == "PPPP" else 2), hide, lo, hi, keys)
        items.append(it)
        metas.append(meta)
    total = sum(it["t"].shape[0] for it in items)
    perm = np.random.default_rng(3).permutation(total).astype(np.uint64)
    at = 0
    for it in items:
        it["positions"] = perm[at:at + it["t"].shape[0]]
        at += it["t"].shape[0]
    return items, metas


@pytest.mark.parametrize("mode", [2, 0])
def test_show_wire_is_show_mixed_plus_pack_the_oracles_bytes_and_verifies(mode):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    items, metas = show_items()
    d = world("SSPE", 12)
    user = user_ctx(d)
    user.set_secret_independent_addressing(mode)
    blob, shapes, status = wire.show_wire(user, items)
    want_blob, want_shapes, want_status = mixed_then_pack(user, items)
    user.close()
    assert status.tolist() == want_status.tolist()
    no_key = items[4]["positions"].astype(np.int64)
    assert all(status[i] == afx.ST_NO_SYMMETRIC_KEY for i in no_key) and int((status == 0).sum()) == len(status) - len(no_key)
    assert [bytes(s) for s in shapes] == [bytes(s) for s in want_shapes]
    secs, wsecs = afxp_sections(blob), afxp_sections(want_blob)
    assert len(secs) == len(items) and len(blob) == len(want_blob)
    for g, (sec, wsec, it, meta) in enumerate(zip(secs, wsecs, items, metas)):
        shape, rec = afxp_records(sec)
        _, wrec = afxp_records(wsec)
        assert sec[:afx.lib().afx_wire_header_bytes(C.byref(shape))] == wsec[:afx.lib().afx_wire_header_bytes(C.byref(shape))]
        st = status[it["positions"].astype(np.int64)]
        for i in range(rec.shape[0]):
            if st[i] == 0:
                assert rec[i].tobytes() == wrec[i].tobytes(), (g, i)
            else:
                assert not rec[i].any(), (g, i)
        # the first item against the oracle's show with the same randomness
        kinds, cr, kps, zw, sd, es = meta
        if st[0] == 0:
            ost, pr = d["user"].show(kinds, cr[0]["values"], cr[0]["t"], cr[0]["U"], cr[0]["V"], kps[0], zw[0], sd[0], es[0])
            assert ost == 0 and rec[0].tobytes() == oracle_record(pr), g
    issuer = issuer_ctx(d)
    verdict = wire.verify_mixed_wire(issuer, blob)
    issuer.close()
    stream_status = np.concatenate([status[it["positions"].astype(np.int64)] for it in items])
    assert ((verdict == 0) == (stream_status == 0)).all(), (verdict.tolist(), stream_status.tolist())


# ---- 3. the whole loop on bytes ----------------------------------------------------------------------------------------------------
def test_the_whole_protocol_on_bytes():
    import aeonflux_amd as afx
    from aeonflux_amd import batch, wire
    d = world("SSPE", 12)
    issuer, user = issuer_ctx(d), user_ctx(d)
    lib = afx.lib()
    rng = np.random.default_rng(33)
    # (hidden group elements in trailing positions only: elsewhere the reference's own presentations do not verify, see
    # afx_ctx_set_strict)
    layouts = [([0, 0, 3, 3], [1, 3], 40), ([0, 2, 0, 3], [0, 3], 7), ([0, 0, 0, 3], [1, 3], 1)]
    requests, rnds, plains = [], [], []
    for kinds, _, cnt in layouts:
        values = np.zeros((N, cnt, 32), np.uint8)
        M2, m3 = np.zeros((N, cnt, 32), np.uint8), np.zeros((N, cnt, 32), np.uint8)
        for i, k in enumerate(kinds):
            if k == 0:
                values[i] = batch.scalars_from_wide(user, rng.integers(0, 256, size=(cnt, 64), dtype=np.uint8))
            elif k == 2:
                values[i] = batch.points_from_uniform(user, rng.integers(0, 256, size=(cnt, 64), dtype=np.uint8))
            else:   # a point attribute made from a message: its M2 and m3 are what hiding it needs (symmetric.rs:135-143)
                msgs = np.ascontiguousarray(rng.integers(0, 256, size=(cnt, 30), dtype=np.uint8))
                M1, a2, a3 = (np.zeros((cnt, 32), np.uint8) for _ in range(3))
                afx.check(lib.afx_plaintexts_from_bytes(user.h, msgs.ctypes.data, cnt, M1.ctypes.data, a2.ctypes.data, a3.ctypes.data, None))
                values[i], M2[i], m3[i] = M1, a2, a3
        requests.append(wire.pack_requests(kinds, values))
        rnds.append({k: rng.integers(0, 256, size=(cnt, w), dtype=np.uint8) for k, w in (("t_wide", 64), ("U_wide", 64), ("rng_seed", 32))})
        plains.append((M2, m3))
    total = sum(c for _, _, c in layouts)
    afxi, issued = wire.issue_wire(issuer, b"".join(requests), {k: np.concatenate([r[k] for r in rnds]) for k in rnds[0]})
    assert issued.tolist() == [0] * total
    assert wire.verify_issuances_stream(user, afxi).tolist() == [0] * total
    items = []
    for (kinds, hide, cnt), sec, (M2, m3) in zip(layouts, sections_of(afxi, wire.issuance_section_bytes), plains):
        k2, values, iss = wire.unpack_issuances(sec)
        assert k2 == kinds
        shown = list(kinds)
        for i in hide:   # hide_attribute (credential.rs:53-75)
            shown[i] = 1 if kinds[i] == 0 else 4
        nsp = sum(1 for k in shown if k == 4)
        ms = np.ascontiguousarray(rng.integers(0, 256, size=(cnt, 64), dtype=np.uint8))
        kp = [np.zeros((cnt, 32), np.uint8) for _ in range(4)]
        afx.check(lib.afx_keypairs_derive(user.h, ms.ctypes.data, cnt, *(x.ctypes.data for x in kp)))
        items.append(dict(kinds=shown, values=values, M2=M2, m3=m3, t=iss["t"], U=iss["U"], V=iss["V"], keypairs=dict(zip(("a", "a0", "a1", "pk"), kp)),
                          z_wide=rng.integers(0, 256, size=(cnt, 64), dtype=np.uint8), rng_seed=rng.integers(0, 256, size=(cnt, 32), dtype=np.uint8),
                          enc_seeds=rng.integers(0, 256, size=(nsp, cnt, 32), dtype=np.uint8) if nsp else None))
    afxp, shapes, shown_status = wire.show_wire(user, items)
    assert shown_status.tolist() == [0] * total
    assert [s.n_hidden_scalars for s in shapes] == [1, 1, 1] and [s.n_enc_proofs for s in shapes] == [1, 1, 1]
    assert wire.verify_mixed_wire(issuer, afxp).tolist() == [0] * total
    issuer.close()
    user.close()


# ---- 4. size queries, short buffers, refused groups --------------------------------------------------------------------------------
def test_size_queries_short_buffers_and_refused_inputs_leave_the_buffers_alone():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    from aeonflux_amd.batch import _show_args
    lib = afx.lib()
    items, _ = show_items()
    d = world("SSPE", 12)
    user = user_ctx(d)
    arr = (afx.ShowGroup * len(items))()
    keep = []
    for g, it in enumerate(items):
        cs, kp, rnd, _, _, cnt, k = _show_args(it["kinds"], it["values"], it["t"], it["U"], it["V"], it.get("keypairs"), it["z_wide"], it["rng_seed"],
                                               it.get("enc_seeds"), it.get("M2"), it.get("m3"), outputs=False)
        arr[g].creds, arr[g].rnd, arr[g].count = cs, rnd, cnt
        if kp is not None:
            arr[g].keypairs = C.pointer(kp)
        arr[g].positions = it["positions"].ctypes.data_as(C.POINTER(C.c_uint64))
        keep.append((k, kp))
    total = sum(it["t"].shape[0] for it in items)
    need = C.c_size_t(0)
    afx.check(lib.afx_show_wire(user.h, arr, len(items), None, 0, C.byref(need), None, 0))
    blob, _, _ = wire.show_wire(user, items)
    assert need.value == len(blob)
    out = np.full(need.value, 0xEE, np.uint8)
    st = np.full(total, 0xEE, np.uint8)
    got = C.c_size_t(0)
    call = lambda cap, slen, a=arr, ng=len(items): lib.afx_show_wire(user.h, a, ng, out.ctypes.data, cap, C.byref(got), st.ctypes.data, slen)
    assert call(need.value - 1, total) == afx.E_BAD_ARGS
    assert call(need.value, total - 1) == afx.E_BAD_ARGS
    pos = np.array(items[0]["positions"])
    items[0]["positions"][1] = items[0]["positions"][0]   # a position used twice
    assert call(need.value, total) == afx.E_BAD_ARGS
    items[0]["positions"][:] = pos
    for field, value in (("n_attributes", 0), ("n_attributes", N + 1), ("kind", 5), ("values", None)):
        saved = bytes(arr[1])
        if field == "kind":
            arr[1].creds.kinds[2] = value
        else:
            setattr(arr[1].creds, field, value)
        assert call(need.value, total) == afx.E_BAD_ARGS, field
        C.memmove(C.addressof(arr[1]), saved, len(saved))
    assert (out == 0xEE).all() and (st == 0xEE).all()
    afx.check(call(need.value, total))
    assert out.tobytes() == blob and got.value == need.value
    # the issuance stream: a short status buffer, a malformed section behind valid ones, an empty stream
    a, afxi, _ = issued_stream()
    cnt = C.c_size_t(0)
    st = np.full(20, 0xEE, np.uint8)
    assert lib.afx_verify_issuances_mixed_wire(user.h, afxi, len(afxi), st.ctypes.data, 19, C.byref(cnt)) == afx.E_BAD_ARGS and cnt.value == 20
    for tail in (afxi[:40], b"AFXI", afxi[:32] + bytes(8), b"AFXR" + afxi[4:200]):
        assert lib.afx_verify_issuances_mixed_wire(user.h, afxi + tail, len(afxi) + len(tail), st.ctypes.data, st.size, C.byref(cnt)) == afx.E_BAD_ARGS
    assert (st == 0xEE).all()
    cnt.value = 7
    afx.check(lib.afx_verify_issuances_mixed_wire(user.h, b"", 0, None, 0, C.byref(cnt)))
    assert cnt.value == 0
    user.close()


# ---- 5. many passes on both lanes --------------------------------------------------------------------------------------------------
def test_many_passes_on_both_lanes_give_the_one_pass_bytes():
    from aeonflux_amd import wire
    d = world("SSPE", 12)
    it, _ = show_item(d, [0, 3], 0, 12)
    count = (1 << 16) + 3
    big = take_items(it, np.arange(count) % 12)
    rng = np.random.default_rng(5)
    big["z_wide"] = rng.integers(0, 256, size=(count, 64), dtype=np.uint8)
    big["rng_seed"] = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    big["enc_seeds"] = rng.integers(0, 256, size=(1, count, 32), dtype=np.uint8)
    _, afxi, _ = issued_stream()
    secs = sections_of(afxi, wire.issuance_section_bytes)
    stream = afxi_with(secs[0], np.arange(count) % 8) + secs[1] + afxi_with(secs[0], np.arange(3))
    user = user_ctx(d)
    one = wire.show_wire(user, [big])
    vone = wire.verify_issuances_stream(user, stream)
    user.set_chunk_items(4096)
    two = wire.show_wire(user, [big])
    vtwo = wire.verify_issuances_stream(user, stream)
    user.close()
    assert one[2].tolist() == [0] * count and two[2].tolist() == one[2].tolist()
    assert two[0] == one[0]
    assert vone.tolist() == [0] * (count + 5 + 3) and vtwo.tolist() == vone.tolist()


# ---- 6. one-item calls of 32 threads -----------------------------------------------------------------------------------------------
def test_one_item_calls_of_32_threads_are_collected_and_give_the_single_thread_results():
    from aeonflux_amd import wire
    d = world("SSPE", 12)
    it, _ = show_item(d, [0, 3], 0, 12)
    one = lambda i: take_items(it, [i])
    _, afxi, _ = issued_stream()
    sec = sections_of(afxi, wire.issuance_section_bytes)[0]
    single = lambda i: afxi_with(sec, [i])
    user = user_ctx(d)
    want_show = [wire.show_wire(user, [one(i)]) for i in range(12)]
    want_ver = [wire.verify_issuances_stream(user, single(i)).tolist() for i in range(8)]
    assert all(w[2].tolist() == [0] for w in want_show) and all(w == [0] for w in want_ver)
    for which in ("show", "verify"):
        user.close()
        user = user_ctx(d)
        errs = []

        def work(t):
            try:
                for r in range(6):
                    i = (6 * t + r) % 12
                    if which == "show":
                        got = wire.show_wire(user, [one(i)])
                        assert got[0] == want_show[i][0] and got[2].tolist() == [0], (t, r)
                    else:
                        assert wire.verify_issuances_stream(user, single(i % 8)).tolist() == want_ver[i % 8], (t, r)
            except BaseException as e:   # noqa: an assertion in a thread must fail the test
                errs.append((t, repr(e)[:400]))
        ths = [threading.Thread(target=work, args=(t,)) for t in range(32)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs[:3]
        s = user.coalescing_stats()
        assert s["sessions"] > 0 and s["max_calls"] > 1, (which, s)
    user.close()


# ---- 7. a group of devices ---------------------------------------------------------------------------------------------------------
def test_group_gives_the_one_context_bytes():
    import torch
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    d = world("SSPE", 12)
    devices = list(range(torch.cuda.device_count())) or [0]
    if len(devices) == 1:
        devices = [0, 0]
    items, _ = show_items()
    it, _ = show_item(d, [0, 3], 0, 12)
    count = 5000   # above the small-call bound: every group is split over the members
    big = take_items(it, np.arange(count) % 12)
    for it2 in items:
        it2.pop("positions")
    large = [big] + items
    _, afxi, _ = issued_stream()
    secs = sections_of(afxi, wire.issuance_section_bytes)
    stream = secs[1] + afxi_with(secs[0], np.arange(count) % 8) + secs[2] + secs[0]
    user = user_ctx(d)
    want = [wire.show_wire(user, items), wire.show_wire(user, large)]
    wver = [wire.verify_issuances_stream(user, afxi), wire.verify_issuances_stream(user, stream)]
    user.close()
    g = afx.Group(d["params"], None, d["ip"], devices)
    got = [wire.show_wire(g, items), wire.show_wire(g, large)]
    gver = [wire.verify_issuances_stream(g, afxi), wire.verify_issuances_stream(g, stream)]
    g.close()
    for w, x in zip(want, got):
        assert x[0] == w[0] and x[2].tolist() == w[2].tolist() and [bytes(s) for s in x[1]] == [bytes(s) for s in w[1]]
    assert want[1][2][:count].tolist() == [0] * count
    for w, x in zip(wver, gver):
        assert x.tolist() == w.tolist()
    assert wver[1][5:5 + count].tolist() == [0] * count


def test_one_section_and_the_stream_share_the_plan_cache():
    """afx_verify_issuances_wire and afx_verify_issuances_mixed_wire stage a section in one function (wire.cpp verify_records): on a fresh
    context the first call of a 3-item section of 2 attributes assembles the plans, the same call again and then the stream's entry point
    on the same bytes run on them - hits, and not one miss more (tests/hostsim/user_wire_fuzz.cpp shared_plan_cache is the host's half)."""
    from aeonflux_amd import wire
    d = world("SSPE", 12)
    rng = np.random.default_rng(31)
    iss = {k: rng.integers(0, 256, size=(3, 32), dtype=np.uint8) for k in ("t", "U", "V", "challenge")}
    iss["responses"] = rng.integers(0, 256, size=(N + 5, 3, 32), dtype=np.uint8)
    blob = wire.pack_issuances([0, 2], rng.integers(0, 256, size=(2, 3, 32), dtype=np.uint8), iss)
    user = user_ctx(d)
    s = [user.plan_cache_stats()]
    got = []
    for call in (user.verify_issuances_wire, user.verify_issuances_wire, lambda b: wire.verify_issuances_stream(user, b)):
        got.append(call(blob)[:3].tolist())
        s.append(user.plan_cache_stats())
    user.close()
    assert got[0] == got[1] == got[2] and 0 not in got[0]   # (random bytes verify nowhere)
    assert s[1]["misses"] > s[0]["misses"]
    for k in (2, 3):
        assert s[k]["hits"] > s[k - 1]["hits"] and s[k]["misses"] == s[k - 1]["misses"], s
