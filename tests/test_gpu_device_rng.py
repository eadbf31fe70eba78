"""GPU: randomness drawn on the device (include/aeonflux_gpu.h afx_device_rng; afx_rng_expand, afx_issue_wire_rng, afx_show_wire_rng and
their group forms).  The calls are specified as equivalences, and that is what is checked: an rng call returns the bytes, statuses and
error codes of the explicit call given draw(seed, stream, i, label) - computed here with hashlib's SHAKE256 - at each item's ordinal."""
import ctypes as C
import hashlib
import struct
import threading

import numpy as np
import pytest

from tests.test_gpu_issue_wire import C5, records
from tests.test_gpu_issue_wire import world as issue_world
from tests.test_gpu_user_wire import afxp_sections, issuer_ctx, show_item, take_items, user_ctx
from tests.test_gpu_user_wire import world as user_world

pytestmark = pytest.mark.gpu

PREFIX = b"aeonflux-amd/device-rng/v1"
SEED = bytes(range(32))


def draw(seed, stream, index, label):
    return hashlib.shake_256(PREFIX + seed + struct.pack("<QQB", stream, index, label)).digest(64 if label in (0, 1, 3) else 32)


def draws(seed, stream, first, count, label):
    return np.frombuffer(b"".join(draw(seed, stream, first + i, label) for i in range(count)), np.uint8).reshape(count, -1)


def issue_rnd(seed, stream, count):
    return {k: draws(seed, stream, 0, count, lab) for k, lab in (("t_wide", 0), ("U_wide", 1), ("rng_seed", 2))}


def show_rnd(items, seed, stream):
    """the explicit show randomness the device draws: each item's credentials at their ordinals over the items"""
    out, at = [], 0
    for it in items:
        it = dict(it)
        cnt = it["t"].shape[0]
        nsp = sum(1 for k in it["kinds"] if k == 4)
        it["z_wide"] = draws(seed, stream, at, cnt, 3)
        it["rng_seed"] = draws(seed, stream, at, cnt, 4)
        it["enc_seeds"] = np.stack([draws(seed, stream, at, cnt, 5 + j) for j in range(nsp)]) if nsp else None
        out.append(it)
        at += cnt
    return out


# ---- 1. the draws themselves ---------------------------------------------------------------------------------------------------
def test_rng_expand_is_shake256_for_every_label_across_the_32_bit_boundary():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    d = user_world("SSPE", 12)
    ctx = user_ctx(d)
    first, count = 2 ** 32 - 2 ** 15, 2 ** 16
    for label in range(37):
        got = wire.rng_expand(ctx, label, first, count, seed=SEED, stream=7)
        assert got.shape == (count, afx.draw_bytes(label))
        assert got.tobytes() == draws(SEED, 7, first, count, label).tobytes(), label
    assert wire.rng_expand(ctx, 0, 0, 1, seed=SEED, stream=0).tobytes().hex().startswith("52792efbfab0dd9c")
    ctx.close()


# ---- 2. issuance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("n,layout,count", [(16, C5, 20), (1, "P", 1), (3, "SSP", 70), (4, "SSPE", 300)])
def test_issue_wire_rng_is_issue_wire_on_the_hashlib_draws(n, layout, count, mode):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = issue_world(n, layout, min(count, 70))
    idx = np.arange(count) % w["values"].shape[1]
    blob = wire.pack_requests(w["kinds"], np.ascontiguousarray(w["values"][:, idx]))
    ctx = afx.Context(w["d"]["params"], w["d"]["key"], w["d"]["ip"])
    ctx.set_secret_independent_addressing(mode)
    got, status = wire.issue_wire_rng(ctx, blob, seed=SEED, stream=3)
    want, wst = wire.issue_wire(ctx, blob, issue_rnd(SEED, 3, count))
    ctx.close()
    assert status.tolist() == wst.tolist() == [0] * count
    assert got == want


def test_interleaved_stream_of_three_layouts_and_a_wrong_n_section():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    a, b = issue_world(4, "SSPE", 70), issue_world(4, "PPPP", 5)
    other = issue_world(3, "SSP", 70)
    stream = (wire.pack_requests(a["kinds"], a["values"][:, :30]) + wire.pack_requests(b["kinds"], b["values"]) +
              wire.pack_requests(other["kinds"], other["values"][:, :4]) + wire.pack_requests([2, 2, 0, 0], a["values"][:, 30:33]) +
              wire.pack_requests(a["kinds"], a["values"][:, 40:70]) + wire.pack_requests(b["kinds"], b["values"][:, :2]))
    total = 30 + 5 + 4 + 3 + 30 + 2
    ctx = afx.Context(a["d"]["params"], a["d"]["key"], a["d"]["ip"])
    got, status = wire.issue_wire_rng(ctx, stream, seed=SEED, stream=11)
    want, wst = wire.issue_wire(ctx, stream, issue_rnd(SEED, 11, total))
    ctx.close()
    assert status.tolist() == wst.tolist()
    # (the third layout's items carry scalars where it expects points: what afx_issue_wire answers them, the rng call answers too)
    assert wst[35:39].tolist() == [afx.ST_MAC_CREATION] * 4 and (wst[:35] == 0).all() and (wst[42:] == 0).all()
    assert got == want


def test_large_stream_crosses_the_first_host_slice_and_matches_the_column_path_on_samples():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = issue_world(16, C5, 20)
    count = 2 ** 16 + 1000
    blob = wire.pack_requests(w["kinds"], np.ascontiguousarray(w["values"][:, np.arange(count) % 20]))
    ctx = afx.Context(w["d"]["params"], w["d"]["key"], w["d"]["ip"])
    got, status = wire.issue_wire_rng(ctx, blob, seed=SEED, stream=2 ** 64 - 1)
    rnd = issue_rnd(SEED, 2 ** 64 - 1, count)
    want, wst = wire.issue_wire(ctx, blob, rnd)
    ctx.close()
    assert status.tolist() == wst.tolist() == [0] * count
    assert got == want
    # 64 sampled items against afx_issue on columns with the same draws (tests/test_gpu_issue_wire.py ties that path to the oracle)
    from aeonflux_amd import batch
    sample = np.random.default_rng(5).choice(count, 64, replace=False)
    octx = afx.Context(w["d"]["params"], w["d"]["key"], w["d"]["ip"])
    o, ost = batch.issue(octx, w["kinds"], np.ascontiguousarray(w["values"][:, sample % 20]), rnd["t_wide"][sample], rnd["U_wide"][sample], rnd["rng_seed"][sample])
    octx.close()
    cells = 4 + 21 + 16
    rec = records(got, len(got) - count * cells * 32, cells)
    for j, i in enumerate(sample):
        r = rec[i].reshape(cells, 32)
        assert r[0].tobytes() == o["t"][j].tobytes() and r[1].tobytes() == o["U"][j].tobytes() and r[2].tobytes() == o["V"][j].tobytes()
    assert ost.tolist() == [0] * 64


# ---- 3. show --------------------------------------------------------------------------------------------------------------------
def show_groups():
    """groups with 0, 1 and 4 hidden points (SECRET_POINT positions), one without keypairs"""
    specs = [("PPPP", [], 0, 5, True), ("SSPE", [3], 0, 12, True), ("SSPE", [0, 3], 3, 7, True), ("SEEP", [1, 2], 0, 2, True),
             ("SEEP", [2], 0, 2, False)]
    items = []
    for layout, hide, lo, hi, keys in specs:
        it, _ = show_item(user_world(layout, 12 if layout == "SSPE" else 5 if layout == "PPPP" else 2), hide, lo, hi, keys)
        items.append(it)
    # four hidden points: every position of a four-point layout
    it4, _ = show_item(user_world("EEEE", 3), [0, 1, 2, 3], 0, 3, True)
    items.append(it4)
    return items


@pytest.mark.parametrize("with_positions", [False, True])
def test_show_wire_rng_is_show_wire_on_the_hashlib_draws_and_verifies(with_positions):
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    items = show_groups()
    assert [sum(1 for k in it["kinds"] if k == 4) for it in items] == [0, 1, 1, 2, 1, 4]
    total = sum(it["t"].shape[0] for it in items)
    if with_positions:
        perm = np.random.default_rng(4).permutation(total).astype(np.uint64)
        at = 0
        for it in items:
            it["positions"] = perm[at:at + it["t"].shape[0]]
            at += it["t"].shape[0]
    d = user_world("SSPE", 12)
    user = user_ctx(d)
    blob, shapes, status = wire.show_wire_rng(user, items, seed=SEED, stream=5)
    want, wshapes, wst = wire.show_wire(user, show_rnd(items, SEED, 5))
    user.close()
    assert status.tolist() == wst.tolist()
    assert [bytes(s) for s in shapes] == [bytes(s) for s in wshapes]
    assert blob == want
    no_key = items[4]
    first = sum(it["t"].shape[0] for it in items[:4])
    pos = no_key["positions"].astype(np.int64) if with_positions else np.arange(first, first + 2)
    assert all(status[p] == afx.ST_NO_SYMMETRIC_KEY for p in pos)
    sec = afxp_sections(blob)[4]
    assert not np.frombuffer(sec, np.uint8)[afx.lib().afx_wire_header_bytes(C.byref(shapes[4])):].any()
    assert int((status == 0).sum()) == total - 2
    issuer = issuer_ctx(d)
    verdict = wire.verify_mixed_wire(issuer, blob)
    issuer.close()
    order = [it["positions"].astype(np.int64) if with_positions else None for it in items]
    stream_status = np.concatenate([status[o] for o in order]) if with_positions else status
    assert ((verdict == 0) == (stream_status == 0)).all(), (verdict.tolist(), stream_status.tolist())


# ---- 4. many threads, small calls -----------------------------------------------------------------------------------------------
def test_small_rng_calls_of_32_threads_are_collected_and_equal_the_lone_calls():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = issue_world(4, "SSPE", 70)
    d = w["d"]
    calls = [(t, r) for t in range(32) for r in range(4)]
    blob_of = lambda t, r: wire.pack_requests(w["kinds"], np.ascontiguousarray(w["values"][:, (7 * t + r) % 60:(7 * t + r) % 60 + 1 + (t + r) % 3]))
    seed_of = lambda t, r: hashlib.sha256(b"thread-seed %d %d" % (t, r)).digest()
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    want = {c: wire.issue_wire_rng(ctx, blob_of(*c), seed=seed_of(*c), stream=1000 * c[0] + c[1]) for c in calls}
    ctx.close()
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    errs = []

    def work(t):
        try:
            for r in range(4):
                got, st = wire.issue_wire_rng(ctx, blob_of(t, r), seed=seed_of(t, r), stream=1000 * t + r)
                assert st.tolist() == want[(t, r)][1].tolist() and got == want[(t, r)][0], (t, r)
        except BaseException as e:   # noqa: an assertion in a thread must fail the test
            errs.append((t, repr(e)[:400]))
    ths = [threading.Thread(target=work, args=(t,)) for t in range(32)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    s = ctx.coalescing_stats()
    ctx.close()
    assert not errs, errs[:3]
    assert s["sessions"] > 0 and s["appended_calls"] > 0, s
    # show
    du = user_world("SSPE", 12)
    it, _ = show_item(du, [0, 3], 0, 12)
    item_of = lambda t, r: take_items(it, [(t + k) % 12 for k in range(1 + (t + r) % 3)])
    user = user_ctx(du)
    want_s = {c: wire.show_wire_rng(user, [item_of(*c)], seed=seed_of(*c), stream=c[1]) for c in calls}
    user.close()
    user = user_ctx(du)
    errs = []

    def work_s(t):
        try:
            for r in range(4):
                got = wire.show_wire_rng(user, [item_of(t, r)], seed=seed_of(t, r), stream=r)
                assert got[0] == want_s[(t, r)][0] and got[2].tolist() == want_s[(t, r)][2].tolist(), (t, r)
        except BaseException as e:   # noqa
            errs.append((t, repr(e)[:400]))
    ths = [threading.Thread(target=work_s, args=(t,)) for t in range(32)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    s = user.coalescing_stats()
    user.close()
    assert not errs, errs[:3]
    assert s["sessions"] > 0 and s["max_calls"] > 1, s


# ---- 5. a group that lists the device twice ---------------------------------------------------------------------------------------
def test_group_gives_the_one_context_bytes():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = issue_world(4, "SSPE", 70)
    d = w["d"]
    count = 5000   # above the small-call bound: split over the members
    stream = wire.pack_requests(w["kinds"], np.ascontiguousarray(w["values"][:, np.arange(3000) % 70])) + issue_world(4, "PPPP", 5)["request"] + \
        wire.pack_requests(w["kinds"], np.ascontiguousarray(w["values"][:, np.arange(2000) % 70]))
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    want = wire.issue_wire_rng(ctx, stream, seed=SEED, stream=9)
    ctx.close()
    g = afx.Group(d["params"], d["key"], d["ip"], [0, 0])
    got = wire.issue_wire_rng(g, stream, seed=SEED, stream=9)
    g.close()
    assert got[1].tolist() == want[1].tolist() == [0] * (count + 5) and got[0] == want[0]
    du = user_world("SSPE", 12)
    it, _ = show_item(du, [0, 3], 0, 12)
    items = [take_items(it, np.arange(4500) % 12)] + show_groups()[:3]
    user = user_ctx(du)
    want = wire.show_wire_rng(user, items, seed=SEED, stream=10)
    user.close()
    g = afx.Group(du["params"], None, du["ip"], [0, 0])
    got = wire.show_wire_rng(g, items, seed=SEED, stream=10)
    g.close()
    assert got[0] == want[0] and got[2].tolist() == want[2].tolist()


# ---- 6. a seed from getrandom ---------------------------------------------------------------------------------------------------
def test_without_a_seed_two_calls_differ_and_both_verify():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    w = issue_world(4, "SSPE", 70)
    d = w["d"]
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    one, s1 = wire.issue_wire_rng(ctx, w["request"])
    two, s2 = wire.issue_wire_rng(ctx, w["request"])
    ctx.close()
    assert s1.tolist() == s2.tolist() == [0] * 70
    r1, r2 = records(one, 32, 17), records(two, 32, 17)
    for i in range(70):
        for c in range(3):   # t, U, V
            assert r1[i, 32 * c:32 * c + 32].tobytes() != r2[i, 32 * c:32 * c + 32].tobytes(), (i, c)
    user = user_ctx(d)
    assert wire.verify_issuances_stream(user, one).tolist() == [0] * 70
    assert wire.verify_issuances_stream(user, two).tolist() == [0] * 70
    du = user_world("SSPE", 12)
    it, _ = show_item(du, [0, 3], 0, 12)
    user.close()
    user = user_ctx(du)
    p1, _, st1 = wire.show_wire_rng(user, [it])
    p2, _, st2 = wire.show_wire_rng(user, [it])
    user.close()
    assert st1.tolist() == st2.tolist() == [0] * 12 and p1 != p2
    issuer = issuer_ctx(du)
    assert wire.verify_mixed_wire(issuer, p1).tolist() == [0] * 12
    assert wire.verify_mixed_wire(issuer, p2).tolist() == [0] * 12
    issuer.close()


# ---- 7. argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_are_the_explicit_calls_and_write_nothing():
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    lib = afx.lib()
    w = issue_world(4, "SSPE", 70)
    d = w["d"]
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    rng = afx.DeviceRng(SEED, 1)
    blob = w["request"]
    need, cnt = C.c_size_t(0), C.c_size_t(0)
    assert lib.afx_issue_wire_rng(ctx.h, blob, len(blob), C.byref(rng), None, 0, C.byref(need), None, 0, C.byref(cnt)) == 0
    assert need.value == len(w["afxi"]) and cnt.value == 70
    assert lib.afx_issue_wire_rng(ctx.h, blob, len(blob), None, None, 0, C.byref(need), None, 0, C.byref(cnt)) == afx.E_BAD_ARGS
    rnd = afx.IssueRandomness(*(w["rnd"][k].ctypes.data for k in ("t_wide", "U_wide", "rng_seed")))
    out = np.full(need.value, 0xab, np.uint8)
    st = np.full(70, 0xcd, np.uint8)
    cases = [(blob, need.value - 1, 70), (blob, need.value, 69), (blob[:-1], need.value, 70), (b"AFXQ" + blob[4:], need.value, 70)]
    for b, cap, scap in cases:
        e1 = lib.afx_issue_wire(ctx.h, b, len(b), C.byref(rnd), out.ctypes.data, cap, C.byref(need), st.ctypes.data, scap, C.byref(cnt))
        e2 = lib.afx_issue_wire_rng(ctx.h, b, len(b), C.byref(rng), out.ctypes.data, cap, C.byref(need), st.ctypes.data, scap, C.byref(cnt))
        assert e1 == e2 == afx.E_BAD_ARGS, (e1, e2)
        assert (out == 0xab).all() and (st == 0xcd).all()
    e = lib.afx_issue_wire_rng(ctx.h, blob, len(blob), None, out.ctypes.data, out.size, C.byref(need), st.ctypes.data, 70, C.byref(cnt))
    assert e == afx.E_BAD_ARGS and (out == 0xab).all() and (st == 0xcd).all()
    user = user_ctx(d)
    keyless = afx.lib().afx_issue_wire_rng(user.h, blob, len(blob), C.byref(rng), out.ctypes.data, out.size, C.byref(need), st.ctypes.data, 70, C.byref(cnt))
    assert keyless == afx.E_NO_KEY and (out == 0xab).all() and (st == 0xcd).all()
    # expand: bad label, null rng
    buf = np.zeros((4, 64), np.uint8)
    assert lib.afx_rng_expand(ctx.h, C.byref(rng), 37, 0, 4, buf.ctypes.data) == afx.E_BAD_ARGS
    assert lib.afx_rng_expand(ctx.h, None, 0, 0, 4, buf.ctypes.data) == afx.E_BAD_ARGS
    assert not buf.any()
    ctx.close()
    # show: short buffers, a position used twice, a null rng
    du = user_world("SSPE", 12)
    it, _ = show_item(du, [0, 3], 0, 12)
    user.close()
    user = user_ctx(du)
    blob_s, _, _ = wire.show_wire_rng(user, [it], seed=SEED, stream=1)
    from aeonflux_amd import ShowGroup
    from aeonflux_amd.batch import _show_args
    arr = (ShowGroup * 1)()
    cs, kp, rnd_s, _, _, n_it, keep = _show_args(it["kinds"], it["values"], it["t"], it["U"], it["V"], it["keypairs"], it["z_wide"], it["rng_seed"],
                                                 it.get("enc_seeds"), it.get("M2"), it.get("m3"), outputs=False)
    arr[0].creds, arr[0].rnd, arr[0].count, arr[0].keypairs = cs, rnd_s, n_it, C.pointer(kp)
    pos = np.array([0] * 12, np.uint64)
    out = np.full(len(blob_s), 0xab, np.uint8)
    st = np.full(12, 0xcd, np.uint8)
    got = C.c_size_t(0)
    for cap, slen, p in ((len(blob_s) - 1, 12, None), (len(blob_s), 11, None), (len(blob_s), 12, pos)):
        arr[0].positions = p.ctypes.data_as(C.POINTER(C.c_uint64)) if p is not None else None
        e1 = lib.afx_show_wire(user.h, arr, 1, out.ctypes.data, cap, C.byref(got), st.ctypes.data, slen)
        e2 = lib.afx_show_wire_rng(user.h, arr, 1, C.byref(rng), out.ctypes.data, cap, C.byref(got), st.ctypes.data, slen)
        assert e1 == e2 == afx.E_BAD_ARGS, (e1, e2)
        assert (out == 0xab).all() and (st == 0xcd).all()
    arr[0].positions = None
    assert lib.afx_show_wire_rng(user.h, arr, 1, None, out.ctypes.data, out.size, C.byref(got), st.ctypes.data, 12) == afx.E_BAD_ARGS
    assert (out == 0xab).all() and (st == 0xcd).all()
    user.close()
    del keep
