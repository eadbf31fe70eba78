"""GPU: batchable presentation proofs (include/aeonflux_gpu.h "Batchable presentation proofs") against the CPU yardsticks of
tests/batchable_ref.py - the oracle's commitments for what an honest show must write, the per-constraint pure-Python verifier for
every verdict.  Seeds are fixed; every case conditions on its inputs, so that no test passes by accepting or rejecting everything."""
import hashlib

import numpy as np
import pytest

from tests import batchable_ref as B
from tests.helpers import corrupt, make_credentials
from tests.soa import presentation_arrays, shape_of

pytestmark = pytest.mark.gpu

LAYOUTS = [(1, "S", []), (3, "ESS", [0]), (4, "SSPE", [0, 3]), (8, "SSPPEEEE", [4, 5, 6, 7]), (16, "SSSSSSSSPPPPEEEE", [12, 13, 14, 15])]
SEED_A, SEED_B, SEED_C = bytes(range(32)), hashlib.sha256(b"weights-b").digest(), hashlib.sha256(b"weights-c").digest()


def _show_inputs(d, hide, count):
    """the oracle's honest presentations of d's credentials and the same inputs as the column arrays batch.show takes"""
    creds, user, take = d["creds"], d["user"], d["take"]
    n = len(creds[0]["kinds"])
    skinds = list(creds[0]["kinds"])
    for i in hide:
        skinds[i] = 1 if skinds[i] == 0 else 4
    nsp = sum(1 for k in skinds if k == 4)
    kps = [user.keypair_derive(take(64)) for _ in range(count)]
    zw, sd, es = [take(64) for _ in range(count)], [take(32) for _ in range(count)], [take(32 * nsp) for _ in range(count)]
    want = []
    for c, kp, z, s, e in zip(creds, kps, zw, sd, es):
        st, p = user.show(skinds, c["values"], c["t"], c["U"], c["V"], kp, z, s, e)
        assert st == 0
        want.append(p)
    col = lambda f: np.stack([np.frombuffer(f(c), np.uint8) for c in creds])
    part = lambda a, b: np.stack([col(lambda c, i=i: c["values"][i][a:b]) for i in range(n)])
    kpd = {f: np.stack([np.frombuffer(k[32 * j:32 * j + 32], np.uint8) for k in kps]) for j, f in enumerate(("a", "a0", "a1", "pk"))}
    esr = np.stack([np.stack([np.frombuffer(e[32 * j:32 * j + 32], np.uint8) for e in es]) for j in range(nsp)]) if nsp else None
    args = (skinds, part(0, 32), col(lambda c: c["t"]), col(lambda c: c["U"]), col(lambda c: c["V"]), kpd, np.stack([np.frombuffer(z, np.uint8) for z in zw]),
            np.stack([np.frombuffer(s, np.uint8) for s in sd]), esr, part(32, 64) if nsp else None, part(64, 96) if nsp else None)
    return want, args, dict(keypairs=kps, z_wide=zw, seeds=sd, enc_seeds=es, skinds=skinds)


def _gpu_verify(afx, batch, ctx, pres, cms, seed, stream=0):
    shape = afx.Shape.from_buffer_copy(bytes(shape_of(pres[0])))
    return batch.verify_presentations_batchable(ctx, shape, presentation_arrays(pres), B.arrays_of(cms), seed, stream).tolist()


@pytest.mark.parametrize("count", [1, 70, 300])
@pytest.mark.parametrize("n,layout,hide", LAYOUTS)
def test_honest_show_writes_both_encodings_and_verify_accepts(n, layout, hide, count):
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    d = make_credentials(n, layout, count, b"batchable-honest-%d-%s" % (count, layout.encode()))
    want, args, _ = _show_inputs(d, hide, count)
    issuer = d["issuer"]
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    pres, cm, shape, st = batch.show_batchable(ctx, *args)
    assert st.tolist() == [0] * count
    assert cm["main"].shape[0] == afx.lib().afx_batchable_main_commitments(ctx.h, shape) > 0
    a = presentation_arrays(want)
    for f in ("challenge", "responses", "C_x_0", "C_x_1", "C_V", "C_y", "attr_values"):      # every compact byte is the oracle's show
        assert np.array_equal(pres[f], a[f]), f
    for e, ea in enumerate(a["enc"]):
        for f, v in ea.items():
            assert np.array_equal(pres["enc"][e][f], v), (e, f)
    compact = [issuer.verify_presentation(p) for p in want]
    assert compact == ([1] * count if layout == "ESS" else [0] * count)                        # (ESS: the constraint-#3 quirk rejects honest proofs)
    oracle_cm = [B.to_batchable(issuer, p) for p in want]
    assert all(c is not None for c in oracle_cm)
    assert cm["main"].shape[0] == len(oracle_cm[0]["main"])                                     # n_main is the oracle's number of commitments
    ref = B.arrays_of(oracle_cm)
    if layout != "ESS":   # (a rejected compact proof's RECOMPUTED commitments are not the ones its prover hashed)
        assert np.array_equal(cm["main"], ref["main"])
        for e in range(len(ref["enc"])):
            assert np.array_equal(cm["enc"][e], ref["enc"][e]), e
    got = batch.verify_presentations_batchable(ctx, shape, pres, cm, SEED_A).tolist()
    assert got == compact
    assert batch.verify_presentations(ctx, shape, pres).tolist() == compact                    # both forms, one verdict
    # the yardstick on a few of them (all of a single-item case)
    for i in sorted(set([0, count // 2, count - 1])):
        item = dict(main=[cm["main"][j, i].tobytes() for j in range(cm["main"].shape[0])], enc=[[c[j, i].tobytes() for j in range(5)] for c in cm["enc"]])
        assert B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(want[i]), item) == compact[i]
    ctx.close()


CLASSES = ("compact-field", "main-bit", "enc-bit", "zero", "ff", "other-point", "swap")


def damaged_case(n, layout, hide, count, seed):
    """honest batchable items, damaged by a seeded choice per item; returns (d, pres, cms, class per item or None, yardstick verdicts)"""
    import oracle
    d = make_credentials(n, layout, count, seed)
    pres, _, _ = _show_inputs(d, hide, count)
    cms = [B.to_batchable(d["issuer"], p) for p in pres]
    before = [bytes(p) for p in pres]
    corrupt(pres, seed + b"-corrupt")       # (its challenge flip touches a field this form does not read: such an item stays honest)
    rnd = hashlib.shake_256(seed + b"-commitments").digest(8 * count + 64)
    other = oracle.point_from_uniform(rnd[-64:])
    ne = pres[0].n_enc_proofs
    classes = []
    for i, (p, cm) in enumerate(zip(pres, cms)):
        r = rnd[8 * i:8 * i + 8]
        q = oracle.Presentation.from_buffer_copy(bytes(p))
        for k in range(32):
            q.challenge[k] = before[i][k + type(p).challenge.offset]
        if bytes(q) != before[i]:            # damaged in a field this form reads
            classes.append("compact-field")
            continue
        if r[0] % 24 >= 7:
            classes.append(None)
            continue
        kind = CLASSES[1 + r[0] % 24 % 6]
        if kind == "enc-bit" and not ne:
            kind = "main-bit"
        main = list(cm["main"])
        j = r[1] % len(main)
        if kind == "main-bit":
            b = bytearray(main[j]); b[r[2] % 31] ^= 1 << (r[3] % 8); main[j] = bytes(b)
        elif kind == "enc-bit":
            e, k = r[1] % ne, r[2] % 5
            b = bytearray(cm["enc"][e][k]); b[r[3] % 31] ^= 1 << (r[4] % 8)
            cm["enc"][e] = cm["enc"][e][:k] + [bytes(b)] + cm["enc"][e][k + 1:]
        elif kind == "zero":
            main[j] = bytes(32)
        elif kind == "ff":
            main[j] = b"\xff" * 32
        elif kind == "other-point":
            main[j] = other
        elif kind == "swap":
            k = (j + 1) % len(main)
            main[j], main[k] = main[k], main[j]
        cm["main"] = main
        classes.append(kind)
    want = [B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(p), cm) for p, cm in zip(pres, cms)]
    return d, pres, cms, classes, want


DAMAGED = [(1, "S", [], 64, b"batchable-damaged-S"), (4, "SSPE", [0, 3], 64, b"batchable-damaged-SSPE"),
           (8, "SSPPEEEE", [4, 5, 6, 7], 64, b"batchable-damaged-C3"), (16, "SSSSSSSSPPPPEEEE", [12, 13, 14, 15], 64, b"batchable-damaged-16-0")]


def check_conditions(layout, classes, want):
    """the inputs themselves keep the test honest: a quarter accepted, a quarter rejected, every applicable class present"""
    assert 4 * want.count(0) >= len(want) and 4 * want.count(1) >= len(want), (want.count(0), want.count(1))
    for c in CLASSES:
        if c == "enc-bit" and "E" not in layout:
            continue
        assert c in classes, c


@pytest.mark.parametrize("n,layout,hide,count,seed", DAMAGED)
def test_damaged_items_get_the_yardsticks_verdicts(n, layout, hide, count, seed):
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    d, pres, cms, classes, want = damaged_case(n, layout, hide, count, seed)
    check_conditions(layout, classes, want)
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    got = _gpu_verify(afx, batch, ctx, pres, cms, SEED_A)
    ctx.close()
    assert got == want, [(i, classes[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]


def _pyref_show_all(d, hide, count, shifts, strict=False):
    """pyref as prover over d's credentials, every item under the same `shifts` (tests/batchable_ref.py ShiftingProver: proof `call`,
    constraint j sends R_j + shifts[(call, j)] * D); returns (oracle.Presentation list, commitments list)"""
    _, _, x = _show_inputs(d, hide, count)
    pres, cms = [], []
    for c, kp, z, s, e in zip(d["creds"], x["keypairs"], x["z_wide"], x["seeds"], x["enc_seeds"]):
        p, cm = B.show_shifted(d["params"], d["ip"], x["skinds"], c, kp, z, s, e, shifts, strict=strict)
        pres.append(p)
        cms.append(cm)
    return pres, cms


def test_weights_are_really_applied():
    """commitments R_0 + D, R_1 - D (and +D in the main proof, -D in a proof of encryption), hashed as sent, responses honest: an
    unweighted sum of the constraints accepts these, the yardstick rejects them, and so must the engine under every seed"""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    count = 12
    d = make_credentials(4, "SSPE", count, b"batchable-weights")
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    honest, honest_cm = _pyref_show_all(d, [0, 3], count, {})
    assert [B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(p), cm) for p, cm in zip(honest[:3], honest_cm[:3])] == [0] * 3
    for seed in (SEED_A, SEED_B):
        assert _gpu_verify(afx, batch, ctx, honest, honest_cm, seed) == [0] * count      # the same honest batch, two seeds, the same statuses
    assert _gpu_verify(afx, batch, ctx, honest, honest_cm, None) == [0] * count          # ... and under a seed of the library's own
    for shifts in ({(0, 0): +1, (0, 1): -1}, {(0, 0): +1, (1, 0): -1}, {(0, 2): -1, (1, 4): +1}):
        pres, cms = _pyref_show_all(d, [0, 3], count, shifts)
        want = [B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(p), cm) for p, cm in zip(pres[:4], cms[:4])]
        assert want == [1] * 4
        # the responses are honest for the challenge sent: the COMPACT twin (that challenge, those responses) recomputes the honest
        # commitments, hashes them to another challenge and is rejected as well
        for seed in (SEED_A, SEED_B, SEED_C):
            assert _gpu_verify(afx, batch, ctx, pres, cms, seed) == [1] * count, (shifts, seed.hex())
        # one dishonest item among honest ones fails alone
        mixed_p, mixed_c = list(honest), list(honest_cm)
        mixed_p[5], mixed_c[5] = pres[5], cms[5]
        assert _gpu_verify(afx, batch, ctx, mixed_p, mixed_c, SEED_C) == [0] * 5 + [1] + [0] * (count - 6)
    ctx.close()


@pytest.mark.parametrize("count", [1, 70, 300])
def test_every_plan_variant_mode_and_schedule_gives_the_yardsticks_statuses_and_challenges(count):
    """strict mode on and off, the three secret modes, the fixed key schedule, the large-pass plan at every size and the
    plan variants: the statuses and, through the challenge trace, the squeezed challenges are the yardstick's"""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    for strict in (False, True):
        if not strict:
            d, pres, cms, classes, _ = damaged_case(8, "SSPPEEEE", [4, 5, 6, 7], 24, b"batchable-variants")
        else:        # the strict statement differs from the oracle's: honest items are pyref's own strict show, two of them damaged
            d = make_credentials(4, "SSPE", 24, b"batchable-variants-strict")
            pres, cms = _strict_items(d, [0, 3], 24)
            b = bytearray(cms[1]["main"][2]); b[3] ^= 4; cms[1]["main"][2] = bytes(b)
            pres[2].C_V[1] ^= 2
        traces = [[] for _ in pres]
        want = [B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(p), cm, strict=strict, trace=traces[i])
                for i, (p, cm) in enumerate(zip(pres, cms))]
        assert 0 in want and 1 in want
        first = want.index(0)            # a call of one item gets an accepted one: its transcripts are all reached
        rot = lambda x: x[first:] + x[:first]
        reps = -(-count // len(pres))
        pres, cms, want, traces = ((rot(x) * reps)[:count] for x in (pres, cms, want, traces))
        ne = pres[0].n_enc_proofs
        ctx = afx.Context(d["params"], d["key"], d["ip"])
        ctx.set_strict(strict)
        settings = [dict(variants=v) for v in (0, afx.VARIANT_ONE_WAVE_CHAINS, afx.VARIANT_HASH_HALF_WAVE, afx.VARIANT_NO_POINTSUM_TREE,
                                               afx.VARIANT_ONE_WAVE_CHAINS | afx.VARIANT_HASH_HALF_WAVE | afx.VARIANT_NO_POINTSUM_TREE, afx.VARIANT_SELFCHECK)]
        settings += [dict(secret=m) for m in (0, 1, 2)] + [dict(fixed=1), dict(fixed=1, secret=1), dict(small=0), dict(small=0, secret=1)]
        for s in settings:
            ctx.set_plan_variants(s.get("variants", 0))
            ctx.set_secret_independent_addressing(s.get("secret", 2))
            ctx.set_fixed_key_schedule(s.get("fixed", 0))
            ctx.set_small_batch_items(s.get("small", 4096))
            ctx.set_challenge_trace(1 + ne, count)
            got = _gpu_verify(afx, batch, ctx, pres, cms, SEED_B)
            tr = ctx.get_challenge_trace()
            ctx.set_challenge_trace(0, 0)
            assert got == want, (strict, s, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
            reached = 0
            for i, t in enumerate(traces):
                for r, c in enumerate(t):
                    assert tr[r, i].tobytes() == c, (strict, s, r, i)
                    reached += 1
            assert reached >= count
        ctx.close()


def _strict_items(d, hide, count):
    """honest strict-mode items: pyref's strict show (the oracle's show restated with the strict statement)"""
    return _pyref_show_all(d, hide, count, {}, strict=True)


def test_edge_scalars_in_the_responses_and_weights_at_both_ends():
    """responses 0, 1, l-1, the extreme-digit scalars of the 4-bit recoding and non-canonical values (tests/edge_values.py): statuses
    as the yardstick says - mostly rejected, so no quarter rule here; instead the squeezed challenge equals the yardstick's for every
    item that reaches a transcript - under seeds whose first item's weights have bit 127 set in some and clear in others, so that
    the recoding of the products rho * resp and of the 128-bit coefficients is driven at both ends"""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    from tests import edge_values as EV
    values = list(EV.SCALARS.items()) + list(EV.extreme_digit_scalars(4).items()) + list(EV.NON_CANONICAL.items())
    count = len(values) + 4
    d = make_credentials(4, "SSPE", count, b"batchable-edge")
    pres, _, _ = _show_inputs(d, [0, 3], count)
    cms = [B.to_batchable(d["issuer"], p) for p in pres]
    for i, (name, v) in enumerate(values):          # (the last four items stay honest)
        p, b = pres[i], v.to_bytes(32, "little")
        k = i % (p.n_responses + 6)
        tgt = p.responses[k] if k < p.n_responses else p.enc[0].responses[k - p.n_responses]
        for j in range(32):
            tgt[j] = b[j]
    traces = [[] for _ in pres]
    want = [B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(p), cm, trace=traces[i]) for i, (p, cm) in enumerate(zip(pres, cms))]
    assert want[-4:] == [0] * 4 and want.count(1) >= len(values) - 2
    m = len(cms[0]["main"]) + 5 * len(cms[0]["enc"])
    seeds = []
    for k in range(64):                              # chosen on the CPU, from the hashlib restatement of the draw
        s = hashlib.sha256(b"edge-seed-%d" % k).digest()
        w = B.weights(s, 0, 0, m)
        if any(x >> 127 for x in w) and any(not (x >> 127) for x in w):
            seeds.append(s)
        if len(seeds) == 3:
            break
    assert len(seeds) == 3
    for s in seeds:
        w = B.weights(s, 0, 0, m)
        assert any(x >> 127 for x in w) and any(not (x >> 127) for x in w)
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    for small in (4096, 0):
        ctx.set_small_batch_items(small)
        for s in seeds:
            ctx.set_challenge_trace(2, count)
            got = _gpu_verify(afx, batch, ctx, pres, cms, s)
            tr = ctx.get_challenge_trace()
            ctx.set_challenge_trace(0, 0)
            assert got == want, [(i, values[i][0] if i < len(values) else "honest", g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
            reached = 0
            for i, t in enumerate(traces):
                for r, c in enumerate(t):
                    assert tr[r, i].tobytes() == c, (r, i)
                    reached += 1
            assert reached >= count // 2
    ctx.close()


def test_the_two_wire_doors_against_the_column_calls():
    """afx_show_batchable_wire writes pack_batchable of the column call's output; afx_verify_presentations_batchable_wire on a stream of
    sections of four shapes, interleaved, gives the column statuses in stream order; failed items are zero records; the error contract"""
    import ctypes as C
    import aeonflux_amd as afx
    from aeonflux_amd import batch, wire
    cases = [(4, "SSPE", [0, 3]), (4, "SSPE", [3]), (4, "SSPE", [0]), (4, "SSPE", [])]      # four shapes of one issuer
    d = make_credentials(4, "SSPE", 14, b"batchable-wire")
    ctx = afx.Context(d["params"], d["key"], d["ip"])
    items, column, want_sections = [], [], []
    for k, (n, layout, hide) in enumerate(cases):
        sub = dict(d, creds=d["creds"][3 * k:3 * k + 5])
        want, args, x = _show_inputs(sub, hide, 5)
        pres, cm, shape, st = batch.show_batchable(ctx, *args)
        assert st.tolist() == [0] * 5
        column.append((shape, pres, cm))
        want_sections.append(wire.pack_batchable(shape, pres, cm))
        items.append(dict(kinds=args[0], values=args[1], t=args[2], U=args[3], V=args[4], keypairs=args[5], z_wide=args[6], rng_seed=args[7],
                          enc_seeds=args[8], M2=args[9], m3=args[10]))
    blob, shapes, st = wire.show_batchable_wire(ctx, items)
    assert st.tolist() == [0] * 20
    assert blob == b"".join(want_sections)                                   # the door's bytes are the packer's over the column output
    assert [bytes(s) for s in shapes] == [bytes(c[0]) for c in column]
    # a credential the prover cannot show (t is not canonical): status 1 and a record of zeros, its neighbours untouched
    broken = dict(items[1], t=items[1]["t"].copy())
    broken["t"][2, :] = 0xff
    b2, _, st2 = wire.show_batchable_wire(ctx, [items[0], broken])
    assert st2.tolist() == [0] * 7 + [1] + [0] * 2
    sh1, p1, cm1 = wire.unpack_batchable(b2[len(want_sections[0]):])
    rec = len(want_sections[1]) - afx.lib().afx_batchable_wire_header_bytes(C.byref(sh1))
    hdr = len(want_sections[1]) - rec
    body = b2[len(want_sections[0]) + hdr:]
    per = rec // 5
    assert body[2 * per:3 * per] == bytes(per) and body[:2 * per] == want_sections[1][hdr:hdr + 2 * per]
    # the verifier's door: sections interleaved (shape 0, 1, 2, 3, 1, 0), two items damaged
    order = [0, 1, 2, 3, 1, 0]
    secs = []
    col_status = []
    for j, k in enumerate(order):
        shape, pres, cm = column[k]
        pres = dict(pres, responses=pres["responses"].copy(), enc=pres["enc"])
        cm = dict(cm, main=cm["main"].copy())
        if j == 2:
            cm["main"][1, 3, 7] ^= 0x10
        if j == 4:
            pres["responses"][0, 0, 1] ^= 0x01
        secs.append(wire.pack_batchable(shape, pres, cm))
        col_status += batch.verify_presentations_batchable(ctx, shape, pres, cm, SEED_A).tolist()
    stream = b"".join(secs)
    assert col_status == [0] * 13 + [1] + [0] * 6 + [1] + [0] * 9
    for seed in (SEED_A, SEED_B, None):
        assert wire.verify_batchable_wire(ctx, stream, seed).tolist() == col_status
    # the error contract: a malformed section anywhere fails the call and writes nothing; a short status array; the size query
    L = afx.lib()
    rng = batch.device_rng(SEED_A)
    stt, cnt = np.full(64, 0x77, np.uint8), C.c_size_t(0)
    for bad in (stream[:-32], stream + b"\0" * 32, stream[:len(secs[0])] + b"AFXP" + stream[len(secs[0]) + 4:]):
        assert L.afx_verify_presentations_batchable_wire(ctx.h, bad, len(bad), C.byref(rng), stt.ctypes.data, 64, C.byref(cnt)) == afx.E_BAD_ARGS
        assert stt.tolist() == [0x77] * 64
    assert L.afx_verify_presentations_batchable_wire(ctx.h, stream, len(stream), C.byref(rng), stt.ctypes.data, 10, C.byref(cnt)) == afx.E_BAD_ARGS and cnt.value == 30
    assert stt.tolist() == [0x77] * 64
    # a section whose n_main_commitments is the strict statement's while the context verifies the reference's
    strict_main = [m for m in range(40) if L.afx_batchable_wire_cells_per_record(C.byref(column[0][0]), m)]
    assert len(strict_main) == 2 and strict_main[0] == column[0][2]["main"].shape[0]
    shape, pres, cm = column[0]
    padded = dict(cm, main=np.concatenate([cm["main"]] + [cm["main"][:1]] * (strict_main[1] - strict_main[0])))
    other = wire.pack_batchable(shape, pres, padded)
    assert L.afx_verify_presentations_batchable_wire(ctx.h, other, len(other), C.byref(rng), stt.ctypes.data, 64, C.byref(cnt)) == afx.E_BAD_ARGS
    out_len = C.c_size_t(0)
    arr = (afx.ShowGroup * 1)()
    assert L.afx_show_batchable_wire(ctx.h, arr, 1, None, 0, C.byref(out_len), None, 0) == afx.E_BAD_ARGS       # (an empty credential layout)
    assert L.afx_show_batchable_wire(ctx.h, None, 0, None, 0, C.byref(out_len), None, 0) == 0 and out_len.value == 0
    ctx.close()
