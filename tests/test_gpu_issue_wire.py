"""GPU: Issuer::issue over serialized requests (afx_issue_wire, afx_group_issue_wire: AFXR in, AFXI out).  The response must be the
oracle's credentials packed as AFXI, byte for byte, and what afx_issue + afx_issuance_wire_pack make of the same inputs; mixed
streams come back in request order with failed records zeroed; large streams run in many passes on both lanes; one-request calls of
many threads are collected into shared passes; a group of devices gives the one-context bytes."""
import ctypes as C
import functools
import hashlib
import struct
import threading

import numpy as np
import pytest

from tests.helpers import make_credentials

pytestmark = pytest.mark.gpu

C5 = "S" * 8 + "P" * 4 + "E" * 4


@functools.lru_cache(maxsize=None)
def world(n, layout, count):
    """count oracle-issued credentials of one layout, with the request columns, the randomness and the oracle's AFXI section"""
    from aeonflux_amd import wire
    d = make_credentials(n, layout, count, b"issue-wire-%d-%s" % (n, layout.encode()))
    cr = d["creds"]
    kinds = cr[0]["kinds"]
    col = lambda f: np.frombuffer(b"".join(c[f] for c in cr), np.uint8).reshape(count, 32)
    values = np.frombuffer(b"".join(c["values"][i][:32] for i in range(n) for c in cr), np.uint8).reshape(n, count, 32)
    iss = {f: col(f) for f in ("t", "U", "V", "challenge")}
    iss["responses"] = np.frombuffer(b"".join(c["responses"][k] for k in range(n + 5) for c in cr), np.uint8).reshape(n + 5, count, 32)
    rnd = {k: np.frombuffer(b"".join(c["rnd"][j] for c in cr), np.uint8).reshape(count, w) for j, (k, w) in enumerate((("t_wide", 64), ("U_wide", 64), ("rng_seed", 32)))}
    return dict(d=d, kinds=kinds, values=values, rnd=rnd, afxi=wire.pack_issuances(kinds, values, iss), request=wire.pack_requests(kinds, values))


def issue_then_pack(ctx, kinds, values, rnd):
    """today's server path: afx_issue on columns, then afx_issuance_wire_pack (C)"""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    o, status = batch.issue(ctx, kinds, values, rnd["t_wide"], rnd["U_wide"], rnd["rng_seed"])
    req = afx.AttributesSoA()
    req.n_attributes = len(kinds)
    for i, k in enumerate(kinds):
        req.kinds[i] = k
    values = np.ascontiguousarray(values)
    req.values = values.ctypes.data
    s = afx.IssuanceSoA(*(o[k].ctypes.data for k in ("t", "U", "V", "challenge", "responses")))
    count, nr, n = values.shape[1], ctx.n + 5, C.c_size_t(0)
    afx.check(afx.lib().afx_issuance_wire_pack(C.byref(req), C.byref(s), nr, count, None, 0, C.byref(n)))
    buf = np.zeros(n.value, np.uint8)
    afx.check(afx.lib().afx_issuance_wire_pack(C.byref(req), C.byref(s), nr, count, buf.ctypes.data, buf.size, C.byref(n)))
    return buf.tobytes(), status


def records(blob, hdr, cells):
    return np.frombuffer(blob, np.uint8, offset=hdr).reshape(-1, cells * 32)


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("n,layout,count", [(4, "SSPE", 70), (16, C5, 20), (1, "P", 3), (3, "SSP", 65)])
def test_issue_wire_is_the_oracles_afxi_and_the_column_path(n, layout, count, mode):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = world(n, layout, count)
    ctx = afx.Context(w["d"]["params"], w["d"]["key"], w["d"]["ip"])
    ctx.set_secret_independent_addressing(mode)
    got, status = wire.issue_wire(ctx, w["request"], w["rnd"])
    assert status.tolist() == [0] * count
    assert got == w["afxi"]
    want, st2 = issue_then_pack(ctx, w["kinds"], w["values"], w["rnd"])
    assert st2.tolist() == [0] * count and got == want
    ctx.close()


@pytest.mark.parametrize("count", [1, 63, 65])
@pytest.mark.parametrize("n,layout", [(1, "P"), (3, "SSP")])
def test_issue_wire_rng_then_the_stream_verification_are_the_column_calls(n, layout, count):
    """Below, at and above a wave, on padded passes (16, 64 and 128 items), with 1 and 3 attributes: afx_issue_wire_rng gives the statuses and
    the bytes of afx_issue on the same draws (SHAKE256, include/aeonflux_gpu.h afx_device_rng) packed as AFXI, and
    afx_verify_issuances_mixed_wire the statuses of afx_verify_issuances on the same records - as issued, and with the last one damaged."""
    import aeonflux_amd as afx
    from aeonflux_amd import batch, wire
    w = world(n, layout, 65)
    d, kinds, values = w["d"], w["kinds"], np.ascontiguousarray(w["values"][:, :count])
    seed, stream = bytes(range(32)), 5
    draw = lambda label, size: np.frombuffer(b"".join(hashlib.shake_256(b"aeonflux-amd/device-rng/v1" + seed + struct.pack("<QQB", stream, i, label)).digest(size)
                                                      for i in range(count)), np.uint8).reshape(count, size)
    issuer = afx.Context(d["params"], d["key"], d["ip"])
    got, status = wire.issue_wire_rng(issuer, wire.pack_requests(kinds, values), seed=seed, stream=stream)
    o, st_col = batch.issue(issuer, kinds, values, draw(0, 64), draw(1, 64), draw(2, 32))
    issuer.close()
    assert status.tolist() == st_col.tolist() == [0] * count
    assert got == wire.pack_issuances(kinds, values, o)
    cells = 4 + (n + 5) + n
    rec = records(got, 32, cells).copy()
    rec[count - 1, 2 * 32 + 3] ^= 1   # V of the last item
    o_bad = {k: v.copy() for k, v in o.items()}
    o_bad["V"][count - 1, 3] ^= 1
    user = afx.Context(d["params"], None, d["ip"])
    for blob, cols, want in ((got, o, [0] * count), (got[:32] + rec.tobytes(), o_bad, [0] * (count - 1) + [1])):
        st_wire = wire.verify_issuances_stream(user, blob).tolist()
        assert st_wire == batch.verify_issuances(user, kinds, values, cols).tolist() == want
    user.close()


def test_response_verifies_on_the_user_side_and_a_tampered_record_gets_the_oracles_verdict():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = world(4, "SSPE", 70)
    d = w["d"]
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    got, status = wire.issue_wire(ctx, w["request"], w["rnd"])
    ctx.close()
    user = afx.Context(d["params"], None, d["ip"])
    assert user.verify_issuances_wire(got).tolist() == [0] * 70
    cells = 4 + 9 + 4
    rec = records(got, 32, cells).copy()
    rec[5, 2 * 32 + 3] ^= 1             # V of item 5
    rec[9, (4 + 3) * 32] ^= 4           # a response of item 9
    rec[11, (4 + 9 + 1) * 32 + 7] ^= 2  # an attribute value of item 11
    bad = got[:32] + rec.tobytes()
    want = []
    for i in range(70):
        r = [rec[i, 32 * c:32 * c + 32].tobytes() for c in range(cells)]
        vals = [r[13 + k] + d["creds"][i]["values"][k][32:] for k in range(4)]
        want.append(d["user"].issuance_verify(w["kinds"], vals, r[0], r[1], r[2], r[3], r[4:13]))
    assert want[5] == 1 and want[9] == 1 and want[11] == 1 and sum(want) == 3
    assert user.verify_issuances_wire(bad).tolist() == want
    user.close()


def test_mixed_stream_statuses_records_and_section_order():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    a, b, c = world(4, "SSPE", 70), world(4, "PPPP", 5), world(4, "SEEP", 6)
    d = a["d"]
    # every layout under ONE issuer: the oracle issues b's and c's requests under a's key again (values are just values)
    cases = []
    for w, lo, hi in ((a, 0, 9), (b, 0, 5), (a, 9, 12), (c, 0, 6)):
        cases.append((w["kinds"], w["values"][:, lo:hi].copy(), {k: v[lo:hi] for k, v in w["rnd"].items()}, w["d"]["creds"][lo:hi]))
    # one item of the second section gets an undecodable point value (a P attribute)
    cases[1][1][0, 2] = 0xff
    other = wire.pack_requests([0, 0, 2], a["values"][:3, :2])      # n = 3 on a context of n = 4: MAC_CREATION, both items
    empty = wire.pack_requests(a["kinds"], a["values"][:, :0])       # count = 0
    sections = [wire.pack_requests(k, v) for k, v, _, _ in cases[:2]] + [other] + [wire.pack_requests(*cases[2][:2]), empty,
                                                                               wire.pack_requests(*cases[3][:2])]
    counts = [9, 5, 2, 3, 0, 6]
    z = lambda k, w: np.zeros((k, w), np.uint8)
    rnd_parts = [cases[0][2], cases[1][2], {"t_wide": z(2, 64), "U_wide": z(2, 64), "rng_seed": z(2, 32)}, cases[2][2], cases[3][2]]
    rnd = {k: np.concatenate([p[k] for p in rnd_parts]) for k in ("t_wide", "U_wide", "rng_seed")}
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    got, status = wire.issue_wire(ctx, b"".join(sections), rnd)
    # the column path's status for the damaged item, and the oracle for everything else
    _, st_b = issue_then_pack(ctx, cases[1][0], cases[1][1], cases[1][2])
    ctx.close()
    assert st_b[2] != 0 and st_b.tolist().count(0) == 4
    want_status = [0] * 9 + st_b.tolist() + [afx.ST_MAC_CREATION] * 2 + [0] * 3 + [0] * 6
    assert status.tolist() == want_status
    off = 0
    for si, (cnt, kinds) in enumerate(zip(counts, [cases[0][0], cases[1][0], [0, 0, 2], cases[2][0], a["kinds"], cases[3][0]])):
        n = len(kinds)
        hdr, cells = 32, 4 + 9 + n
        size = hdr + cnt * cells * 32
        sec = got[off:off + size]
        assert sec[:4] == b"AFXI" and np.frombuffer(sec[4:24], "<u4").tolist() == [1, cnt, cells, n, 9] and list(sec[24:24 + n]) == list(kinds), si
        rec = records(sec, hdr, cells)
        for i in range(cnt):
            if si == 2 or (si == 1 and i == 2):
                assert not rec[i].any(), (si, i)
                continue
            case = cases[[0, 1, None, 2, None, 3][si]]
            vals = [case[1][k, i].tobytes() + case[3][i]["values"][k][32:] for k in range(n)]
            r = case[2]
            st, t, U, V, ch, resp = d["issuer"].issue(kinds, vals, r["t_wide"][i].tobytes(), r["U_wide"][i].tobytes(), r["rng_seed"][i].tobytes())
            assert st == 0
            want = t + U + V + ch + b"".join(resp) + b"".join(v[:32] for v in vals)
            assert rec[i].tobytes() == want, (si, i)
        off += size
    assert off == len(got)


def test_size_query_short_buffers_and_a_keyless_context():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = world(4, "SSPE", 70)
    d = w["d"]
    stream = w["request"] + wire.pack_requests([0, 2], w["values"][:2, :3]) + wire.pack_requests(w["kinds"], w["values"][:, :4])
    lib = afx.lib()
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    afx.check(lib.afx_issue_wire(ctx.h, stream, len(stream), None, None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    assert cnt.value == 77
    assert out_len.value == (32 + 70 * 17 * 32) + (32 + 3 * 15 * 32) + (32 + 4 * 17 * 32)
    rnd = {k: np.concatenate([v, v[:7]]) for k, v in w["rnd"].items()}
    r = afx.IssueRandomness(*(rnd[k].ctypes.data for k in ("t_wide", "U_wide", "rng_seed")))
    out = np.full(out_len.value, 0xEE, np.uint8)
    status = np.full(77, 0xEE, np.uint8)
    args = lambda cap, scap: (ctx.h, stream, len(stream), C.byref(r), out.ctypes.data, cap, C.byref(out_len), status.ctypes.data, scap, C.byref(cnt))
    assert lib.afx_issue_wire(*args(out.size - 1, 77)) == afx.E_BAD_ARGS
    assert lib.afx_issue_wire(*args(out.size, 76)) == afx.E_BAD_ARGS
    assert (out == 0xEE).all() and (status == 0xEE).all()
    afx.check(lib.afx_issue_wire(*args(out.size, 77)))
    assert status.tolist() == [0] * 70 + [afx.ST_MAC_CREATION] * 3 + [0] * 4
    assert out[:len(w["afxi"])].tobytes() == w["afxi"]
    ctx.close()
    user = afx.Context(d["params"], None, d["ip"])
    assert lib.afx_issue_wire(user.h, stream, len(stream), C.byref(r), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, 77,
                              C.byref(cnt)) == afx.E_NO_KEY
    user.close()


def test_many_passes_on_both_lanes():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = world(4, "SSPE", 64)
    d = w["d"]
    count = (1 << 16) + 3
    idx = np.arange(count) % 64
    values = np.ascontiguousarray(w["values"][:, idx])
    rng = np.random.default_rng(16)
    rnd = {k: rng.integers(0, 256, size=(count, wd), dtype=np.uint8) for k, wd in (("t_wide", 64), ("U_wide", 64), ("rng_seed", 32))}
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    ctx.set_chunk_items(4096)
    got, status = wire.issue_wire(ctx, wire.pack_requests(w["kinds"], values), rnd)
    want, st2 = issue_then_pack(ctx, w["kinds"], values, rnd)
    ctx.close()
    assert status.tolist() == [0] * count and st2.tolist() == [0] * count
    assert got == want
    rec = records(got, 32, 17)
    for i in range(0, count, count // 256):
        vals = d["creds"][idx[i]]["values"]
        st, t, U, V, ch, resp = d["issuer"].issue(w["kinds"], vals, rnd["t_wide"][i].tobytes(), rnd["U_wide"][i].tobytes(), rnd["rng_seed"][i].tobytes())
        assert st == 0 and rec[i].tobytes() == t + U + V + ch + b"".join(resp) + b"".join(v[:32] for v in vals), i


def test_one_request_calls_of_32_threads_share_passes():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = world(4, "SSPE", 70)
    d = w["d"]
    cells = 17
    rec = records(w["afxi"], 32, cells)
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    errs = []

    def work(t):
        try:
            for r in range(8):
                i = (8 * t + r) % 70
                blob = wire.pack_requests(w["kinds"], w["values"][:, i:i + 1])
                got, status = wire.issue_wire(ctx, blob, {k: v[i:i + 1] for k, v in w["rnd"].items()})
                assert status.tolist() == [0] and got[32:] == rec[i].tobytes(), (t, r)
        except BaseException as e:   # noqa: an assertion in a thread must fail the test
            errs.append((t, repr(e)[:400]))
    ths = [threading.Thread(target=work, args=(t,)) for t in range(32)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs[:3]
    s = ctx.coalescing_stats()
    ctx.close()
    assert s["sessions"] > 0 and s["appended_calls"] > 0, s


def test_group_gives_the_one_context_bytes():
    import torch
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    a, b = world(4, "SSPE", 70), world(4, "PPPP", 5)
    d = a["d"]
    devices = list(range(torch.cuda.device_count())) or [0]
    if len(devices) == 1:
        devices = [0, 0]
    count = 5000   # above the small-call bound: every merged batch is split over the members
    idx = np.arange(count) % 70
    big = np.ascontiguousarray(a["values"][:, idx])
    stream = wire.pack_requests(a["kinds"], big[:, :3000]) + wire.pack_requests(b["kinds"], b["values"]) + wire.pack_requests(a["kinds"], big[:, 3000:])
    rng = np.random.default_rng(7)
    rnd = {k: rng.integers(0, 256, size=(count + 5, wd), dtype=np.uint8) for k, wd in (("t_wide", 64), ("U_wide", 64), ("rng_seed", 32))}
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    want, st1 = wire.issue_wire(ctx, stream, rnd)
    small, st3 = wire.issue_wire(ctx, b["request"], b["rnd"])
    ctx.close()
    g = afx.Group(d["params"], d["key"], d["ip"], devices)
    got, st2 = wire.issue_wire(g, stream, rnd)
    got_small, st4 = wire.issue_wire(g, b["request"], b["rnd"])
    g.close()
    assert st1.tolist() == [0] * (count + 5) and st2.tolist() == st1.tolist() and got == want
    assert st4.tolist() == st3.tolist() and got_small == small
