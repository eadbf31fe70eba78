"""GPU: the BYTES of the batchable verifier's weights (include/aeonflux_gpu.h "Batchable presentation proofs": item `index` draws
draw(seed, stream, index, AFX_DRAW_BATCH_WEIGHTS), weight w = bytes [16 w, 16 w + 16), the main proof's constraints first, then five
per proof of encryption; the wire door's group g under stream + g, ordinals within the group), pinned with the one kind of input
whose verdict depends on them: forgeries built to cancel.

An honest item passes under any weights and a damaged one fails under almost any.  A forgery for ordinal i and weight indices a != b
(tests/batchable_ref.py cancelling_shifts) has constraint a off by rho_b * D and constraint b by -rho_a * D with rho the prescribed
weights of ordinal i: both constraints are false, and the header's one sum is the identity under exactly those 128-bit values at
exactly those places.  tests/test_batchable_ref.py proves that of the inputs without a GPU.  Here every expected status is the
weighted yardstick's (ref_verify_batchable_weighted under B.weights of the prescribed seed, stream and ordinal), never the engine's,
and every test asserts on its inputs first: forgeries expected accepted, others expected rejected, honest items present.

What the engine must get right for a forgery to pass: k_batch_weights' draw per ordinal (index0 + item) and its [w][item] layout, the
stride and the per-pass offset of the weight rows in later passes of a call, all 128 bits in k_coef, weight w at constraint w, and
stream + g on the wire door.  The controls (another seed, stream + 1, a seed of the library's own, the items moved by one ordinal,
weights cut to 64 or 127 bits, ordinals counted per section, no + g) must all be rejected.

CPU preparation, measured and not asserted: pyref proves one item in 0.2 - 0.6 s and the weighted yardstick takes 0.1 - 0.4 s per
verdict on a slow build machine, where the whole file prepares in about 190 s (the 16-attribute case of the first test: about 90 s);
on the GPU host the whole file, GPU calls included, ran in 56 s (that case: 26 s).  The pyref-made items are the forgeries (one per
weight index and layout) and the strict statement's honest items; everything else is the oracle's."""
import ctypes as C
import hashlib
import math
import random

import pytest

from tests import batchable_ref as B
from tests.helpers import DevMem, make_credentials
from tests.soa import presentation_arrays, shape_of
from tests.test_gpu_batchable import LAYOUTS, _show_inputs

pytestmark = pytest.mark.gpu

SEED, OTHER_SEED = hashlib.sha256(b"weights-pinned").digest(), hashlib.sha256(b"weights-pinned-other").digest()


class Case:
    """credentials of one layout and what to make of them: item i is always a show of credential i"""

    def __init__(self, n, layout, hide, count, tag, strict=False):
        self.d = make_credentials(n, layout, count, tag)
        self.oracle_pres, _, self.x = _show_inputs(self.d, hide, count)
        self.strict, self.count = strict, count
        _, cm = self.honest(0)
        self.n_main, self.M = len(cm["main"]), len(cm["main"]) + 5 * len(cm["enc"])

    def honest(self, i):
        """the oracle's show and the commitments its verifier recomputes; in strict mode (a statement the oracle does not have) pyref's"""
        if self.strict:
            return B.forge(self.d, self.x, i, {}, strict=True)
        return self.oracle_pres[i], B.to_batchable(self.d["issuer"], self.oracle_pres[i])

    def damaged(self, i, k):
        """an honest item with one bit of commitment k flipped"""
        p, cm = self.honest(i)
        call, j = B.constraint_of(k % self.M, self.n_main)
        row = list(cm["main"] if call == 0 else cm["enc"][call - 1])
        b = bytearray(row[j])
        b[k % 31] ^= 1 << (k % 8)
        row[j] = bytes(b)
        return p, (dict(cm, main=row) if call == 0 else dict(cm, enc=cm["enc"][:call - 1] + [row] + cm["enc"][call:]))

    def forgery(self, i, rho, a, b):
        return B.forge(self.d, self.x, i, B.cancelling_shifts(rho, a, b, self.n_main), strict=self.strict)

    def weights(self, seed, stream, ordinal):
        return B.weights(seed, stream, ordinal, self.M)

    def yardstick(self, item, rho):
        d = self.d
        return B.ref_verify_batchable_weighted(d["params"], d["key"], d["ip"], B.pyref_presentation(item[0]), item[1], rho, strict=self.strict)

    def per_constraint(self, item):
        d = self.d
        return B.ref_verify_batchable(d["params"], d["key"], d["ip"], B.pyref_presentation(item[0]), item[1], strict=self.strict)

    def context(self, afx):
        ctx = afx.Context(self.d["params"], self.d["key"], self.d["ip"])
        ctx.set_strict(self.strict)
        return ctx

    @classmethod
    def of(cls, d, hide, count):
        """over credentials made elsewhere (several cases of one issuer)"""
        c = cls.__new__(cls)
        c.d, c.strict, c.count = d, False, count
        c.oracle_pres, _, c.x = _show_inputs(d, hide, count)
        _, cm = c.honest(0)
        c.n_main, c.M = len(cm["main"]), len(cm["main"]) + 5 * len(cm["enc"])
        return c


def arrays(items):
    pres = [p for p, _ in items]
    return shape_of(pres[0]), presentation_arrays(pres), B.arrays_of([cm for _, cm in items])


def gpu(afx, batch, ctx, items, seed, stream):
    shape, pa, ca = arrays(items)
    return batch.verify_presentations_batchable(ctx, afx.Shape.from_buffer_copy(bytes(shape)), pa, ca, seed, stream).tolist()


def pair_kinds(pairs, n_main):
    """which proofs each pair joins: main-main, main-enc, two constraints of one proof of encryption, two proofs of encryption"""
    out = set()
    for a, b in pairs:
        (ca, _), (cb, _) = B.constraint_of(a, n_main), B.constraint_of(b, n_main)
        out.add("main-main" if ca == cb == 0 else "main-enc" if 0 in (ca, cb) else "same-enc" if ca == cb else "enc-enc")
    return out


EVERY_INDEX = [(4, "SSPE", [0, 3], False, 10, 5), (8, "SSPPEEEE", [4, 5, 6, 7], False, 26, 2 ** 32 + 9), LAYOUTS[4] + (False, 34, 2 ** 63 + 1),
               (4, "SSPE", [0, 3], True, 11, 2 ** 40)]


@pytest.mark.parametrize("n,layout,hide,strict,M,stream", EVERY_INDEX)
def test_a_forgery_at_every_weight_index_passes_under_the_prescribed_weights_and_no_others(n, layout, hide, strict, M, stream):
    """pairs (w, w + 1 mod M): every weight index is once the `a` and once the `b` of a forgery, and the pairs join two constraints of
    the main proof, the main proof and a proof of encryption (both ways round), two constraints of one proof of encryption and two
    proofs of encryption.  The streams are nonzero, three of the four at or above 2^32."""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    pairs = [(w, (w + 1) % M) for w in range(M)]
    F, H = len(pairs), 3
    Dm = math.ceil((F + H) / 3)
    kinds = ["forgery"] * F + ["honest"] * H + ["damaged"] * Dm
    random.Random(M).shuffle(kinds)
    count = len(kinds)
    case = Case(n, layout, hide, count, b"weights-every-index-" + layout.encode() + bytes([strict]), strict)
    assert case.M == M and stream != 0
    assert sorted(a for a, _ in pairs) == sorted(b for _, b in pairs) == list(range(M)) and all(a != b for a, b in pairs)
    assert pair_kinds(pairs, case.n_main) == {"main-main", "main-enc", "same-enc"} | ({"enc-enc"} if case.M > case.n_main + 5 else set())
    assert (case.n_main - 1, case.n_main) in pairs and (M - 1, 0) in pairs          # main -> enc and enc -> main
    todo = list(pairs)
    items = []
    for i, k in enumerate(kinds):
        items.append(case.forgery(i, case.weights(SEED, stream, i), *todo.pop(0)) if k == "forgery" else case.honest(i) if k == "honest" else case.damaged(i, 7 * i + 3))
    forged = [i for i, k in enumerate(kinds) if k == "forgery"]
    others = [i for i, k in enumerate(kinds) if k != "forgery"]

    def verdicts(seed, strm, its):
        return [case.yardstick(it, case.weights(seed, strm, i)) for i, it in enumerate(its)]
    want = verdicts(SEED, stream, items)
    plain = [case.per_constraint(it) for it in items]
    # the inputs: every forgery is false constraint by constraint and accepted by the header's sum; the others are what they were made as
    assert [plain[i] for i in forged] == [1] * F and [want[i] for i in forged] == [0] * F
    assert [want[i] for i in others] == [plain[i] for i in others] == [0 if kinds[i] == "honest" else 1 for i in others]
    assert 4 * F >= count and 4 * want.count(1) >= count and want.count(0) > F
    ctx = case.context(afx)
    got = gpu(afx, batch, ctx, items, SEED, stream)
    assert got == want, [(i, kinds[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    # controls on the same arrays: under any other weights every forgery is rejected and the honest items still pass
    for name, seed, strm in (("another seed", OTHER_SEED, stream), ("stream + 1", SEED, stream + 1)):
        w2 = verdicts(seed, strm, items)
        assert w2 == plain, name
        got = gpu(afx, batch, ctx, items, seed, strm)
        assert got == w2, (name, [(i, kinds[i], g, w) for i, (g, w) in enumerate(zip(got, w2)) if g != w])
    got = gpu(afx, batch, ctx, items, None, stream)                  # a seed of the library's own: nobody's forgery fits it
    assert got == plain, [(i, kinds[i], g, w) for i, (g, w) in enumerate(zip(got, plain)) if g != w]
    moved = items[1:] + items[:1]                                    # every item one ordinal early (the first one last)
    w3 = verdicts(SEED, stream, moved)
    assert w3 == plain[1:] + plain[:1]
    got = gpu(afx, batch, ctx, moved, SEED, stream)
    assert got == w3, [(i, g, w) for i, (g, w) in enumerate(zip(got, w3)) if g != w]
    ctx.close()


def test_all_128_bits_of_a_weight_count():
    """forgeries against rho mod 2^64 and against rho with bit 127 cleared, at pairs whose two weights really lose something by it, are
    rejected; forgeries against the whole weights, in the same call, pass"""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    stream, cuts = 77, (("whole", lambda r: r), ("mod 2^64", lambda r: r % 2 ** 64), ("bit 127 cleared", lambda r: r & (2 ** 127 - 1)))
    kinds = [c for c in cuts for _ in range(4)] + [None, None]
    random.Random(128).shuffle(kinds)
    case = Case(4, "SSPE", [0, 3], len(kinds), b"weights-width")
    items, used = [], []
    for i, k in enumerate(kinds):
        if k is None:
            items.append(case.honest(i))
            continue
        rho = case.weights(SEED, stream, i)
        top = [w for w in range(case.M) if rho[w] >> 127]
        if len(top) < 2:            # (no two weights of this ordinal have bit 127 set: an honest item in its place)
            kinds[i] = None
            items.append(case.honest(i))
            continue
        a, b = top[i % len(top)], top[(i + 1) % len(top)]
        cut = [k[1](r) for r in rho]
        items.append(case.forgery(i, cut, a, b))
        if k[0] != "whole":
            assert cut[a] != rho[a] and cut[b] != rho[b]
            assert case.yardstick(items[-1], cut) == 0          # (it does cancel under the weights it was built for)
        used.append((a, b))
    want = [case.yardstick(it, case.weights(SEED, stream, i)) for i, it in enumerate(items)]
    assert want == [0 if k is None or k[0] == "whole" else 1 for k in kinds]
    n_whole, n_cut = sum(1 for k in kinds if k and k[0] == "whole"), sum(1 for k in kinds if k and k[0] != "whole")
    assert 4 * n_whole >= len(kinds) and n_cut >= 6 and None in kinds and all(sum(1 for k in kinds if k and k[0] == c[0]) >= 3 for c in cuts)
    ctx = case.context(afx)
    got = gpu(afx, batch, ctx, items, SEED, stream)
    ctx.close()
    assert got == want, [(i, kinds[i] and kinds[i][0], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]


def _dev_verify(afx, batch, ctx, shape, pa, ca, seed, stream):
    """the *_dev entry point on device-resident copies of the arrays"""
    keep = []

    def up(a):
        keep.append(DevMem(a))
        return keep[-1].ptr
    dpres = {f: up(pa[f]) for f in batch.PRES_FIELDS if f != "challenge"}
    dpres["challenge"] = 0
    dpres["enc"] = [{f: (up(d[f]) if f != "challenge" else 0) for f in batch.ENC_FIELDS} for d in pa["enc"]]
    dcm = {"main": up(ca["main"]), "enc": [up(a) for a in ca["enc"]]}
    soa, k1 = batch.presentation_soa(dpres, ptr=lambda x: x)
    csoa, k2 = batch.commitments_soa(dcm, ptr=lambda x: x)
    count = ca["main"].shape[1]
    status = DevMem(nbytes=count, fill=255)
    rng = batch.device_rng(seed, stream)
    afx.check(afx.lib().afx_verify_presentations_batchable_dev(ctx.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), count, status.ptr))
    ctx.synchronize()
    got = status.numpy().tolist()
    for m in keep + [status]:
        m.free()
    return got


def test_forgeries_in_every_pass_of_a_chunked_call_under_every_plan():
    """602 items in passes of 256 (256, 256 and a ragged 90): forgeries at ordinals 0, 255, 256, 257, 511, 512 and 601 - both ends of
    every pass - pass only if each pass reads ITS rows of the call's weights (stride = the call's items, offset = the pass's first
    item).  The rest are 40 oracle items by turns, every fifth damaged; only the seven forgeries are pyref's, so here a quarter of the
    items cannot be forgeries: the conditions are that all seven are expected accepted and that honest and damaged items lie in every
    pass.  The verdict of a repeated oracle item is the weighted yardstick's at the first ordinal it occupies and at the ordinals next
    to the forgeries; at its other ordinals it is taken over: neither an honest nor a damaged item's verdict depends on the weights
    (tests/test_batchable_ref.py compares the two yardsticks on such items)."""
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    chunk, count, stream, base = 256, 602, 2 ** 33 + 3, 40
    at = [0, 255, 256, 257, 511, 512, 601]
    assert count > 2 * chunk and count % chunk and at[4] == 2 * chunk - 1 and at[5] == 2 * chunk and at[6] == count - 1
    case = Case(4, "SSPE", [0, 3], base + len(at), b"weights-chunks")
    fill = [case.damaged(k, 11 * k + 1) if k % 5 == 2 else case.honest(k) for k in range(base)]
    items = [fill[i % base] for i in range(count)]
    pairs = [(0, 9), (4, 5), (7, 2), (9, 8), (3, 0), (5, 6), (1, 4)]
    for k, (o, (a, b)) in enumerate(zip(at, pairs)):
        items[o] = case.forgery(base + k, case.weights(SEED, stream, o), a, b)
    # a repeated item's verdict: at the first ordinal it occupies
    base_want = [case.yardstick(fill[k], case.weights(SEED, stream, k if k not in at else k + base)) for k in range(base)]
    assert base_want == [1 if k % 5 == 2 else 0 for k in range(base)]
    want = [base_want[o % base] for o in range(count)]
    for o in sorted(set(at) | {o + s for o in at for s in (-1, 1) if 0 <= o + s < count}):
        v = case.yardstick(items[o], case.weights(SEED, stream, o))
        assert o in at or v == want[o], o
        want[o] = v
    assert [want[o] for o in at] == [0] * len(at) and [case.per_constraint(items[o]) for o in at] == [1] * len(at)
    for lo in range(0, count, chunk):
        assert {0, 1} <= set(want[o] for o in range(lo, min(lo + chunk, count)) if o not in at)
    shape, pa, ca = arrays(items)
    shape = afx.Shape.from_buffer_copy(bytes(shape))
    ctx = case.context(afx)
    ctx.set_chunk_items(chunk)
    try:
        def run(what, seed=SEED, strm=stream):
            got = batch.verify_presentations_batchable(ctx, shape, pa, ca, seed, strm).tolist()
            return what, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:12]
        settings = [dict(small=0), dict(small=4096)]
        settings += [dict(variants=v) for v in (afx.VARIANT_ONE_WAVE_CHAINS, afx.VARIANT_HASH_HALF_WAVE, afx.VARIANT_NO_POINTSUM_TREE,
                                                afx.VARIANT_ONE_WAVE_CHAINS | afx.VARIANT_HASH_HALF_WAVE | afx.VARIANT_NO_POINTSUM_TREE, afx.VARIANT_SELFCHECK)]
        settings += [dict(secret=m) for m in (0, 1, 2)] + [dict(fixed=1), dict(fixed=1, secret=1), dict(small=0, secret=1)]
        for s in settings:
            ctx.set_plan_variants(s.get("variants", 0))
            ctx.set_secret_independent_addressing(s.get("secret", 2))
            ctx.set_fixed_key_schedule(s.get("fixed", 0))
            ctx.set_small_batch_items(s.get("small", 4096))
            assert run(s) == (s, [])
        ctx.set_plan_variants(0)
        ctx.set_secret_independent_addressing(2)
        ctx.set_fixed_key_schedule(0)
        ctx.set_small_batch_items(4096)
        # the same call with the weights of stream + 1: the seven forgeries are rejected and nothing else changes
        got = batch.verify_presentations_batchable(ctx, shape, pa, ca, SEED, stream + 1).tolist()
        assert got == [1 if o in at else w for o, w in enumerate(want)]
        assert [case.yardstick(items[o], case.weights(SEED, stream + 1, o)) for o in at] == [1] * len(at)
        # the device-resident entry point, then both lanes of a pipelining context: successive calls alternate between them
        assert _dev_verify(afx, batch, ctx, shape, pa, ca, SEED, stream) == want
        ctx.set_pipelining(True)
        for call in range(4):
            assert run(("pipelining", call)) == (("pipelining", call), [])
        for call in range(2):
            assert _dev_verify(afx, batch, ctx, shape, pa, ca, SEED, stream) == want, call
        ctx.set_pipelining(False)
    finally:
        ctx.set_chunk_items(0)
        ctx.close()


def test_the_wire_door_draws_each_merged_group_under_its_own_stream_at_ordinals_within_the_group():
    """sections of three shapes interleaved (0, 1, 0, 2, 1).  F: a forgery for its ordinal within its MERGED group under stream + g, g
    counted in order of first appearance - expected accepted, in a first and in a later section of every shape that has both.  S: built
    for its ordinal within its own section (in later sections, where that differs); G: built under the call's stream without + g (in
    groups 1 and 2, where that differs): expected rejected.  H honest, D damaged."""
    import aeonflux_amd as afx
    from aeonflux_amd import wire
    stream = 2 ** 32 - 1            # (stream + g crosses 2^32)
    hides = [[0, 3], [3], [0]]
    plan = [(0, "FHDF"), (1, "FGHD"), (0, "FSHD"), (2, "FGDH"), (1, "FSGD")]
    group_of, first = {}, {}
    for s, (k, _) in enumerate(plan):
        group_of.setdefault(k, len(group_of))
        first.setdefault(k, s)
    assert group_of == {0: 0, 1: 1, 2: 2}
    d = make_credentials(4, "SSPE", sum(len(t) for _, t in plan), b"weights-wire")
    cases, nxt = {}, 0
    for k, hide in enumerate(hides):
        n_k = sum(len(t) for kk, t in plan if kk == k)
        cases[k] = Case.of(dict(d, creds=d["creds"][nxt:nxt + n_k]), hide, n_k)
        nxt += n_k
    assert [cases[k].M for k in range(3)] == [10, 10, 6]
    filled = {k: 0 for k in cases}      # items of the group so far = the ordinal of the group's next item
    secs, placed, kinds = [], [], []
    for s, (k, types) in enumerate(plan):
        c, g = cases[k], group_of[k]
        sec = []
        for j, t in enumerate(types):
            o = filled[k]               # ordinal within the merged group; also the credential of the case this item shows
            a, b = (o + s) % c.M, (o + s + 1 + j) % c.M
            assert a != b
            if t == "F":
                it = c.forgery(o, c.weights(SEED, stream + g, o), a, b)
            elif t == "S":
                assert s != first[k] and j != o
                it = c.forgery(o, c.weights(SEED, stream + g, j), a, b)
            elif t == "G":
                assert g != 0
                it = c.forgery(o, c.weights(SEED, stream, o), a, b)
            else:
                it = c.honest(o) if t == "H" else c.damaged(o, 5 * o + s)
            sec.append(it)
            placed.append((c, it, g, o))
            kinds.append((s, t))
            filled[k] += 1
        shape, pa, ca = arrays(sec)
        secs.append(wire.pack_batchable(afx.Shape.from_buffer_copy(bytes(shape)), pa, ca))

    def verdicts(seed, strm):
        """the header's: group g draws under strm + g, an item at its ordinal within the group"""
        return [c.yardstick(it, c.weights(seed, strm + g, o)) for c, it, g, o in placed]
    want = verdicts(SEED, stream)
    assert want == [0 if t in "FH" else 1 for _, t in kinds]
    n_f = sum(1 for _, t in kinds if t == "F")
    assert 4 * n_f >= len(want) and 4 * want.count(1) >= len(want) and any(t == "H" for _, t in kinds)
    for k in (0, 1):                    # accepted forgeries in a first and in a later section of the shapes that have both
        assert {s for s, t in kinds if t == "F" and plan[s][0] == k} >= {first[k], max(s for s, (kk, _) in enumerate(plan) if kk == k)}
    blob = b"".join(secs)
    ctx = cases[0].context(afx)
    got = wire.verify_batchable_wire(ctx, blob, SEED, stream).tolist()
    assert got == want, [(kinds[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    # controls: under another seed, the next stream or a seed of the library's own every forgery fails, whatever it was built for
    plain = [0 if t == "H" else 1 for _, t in kinds]
    for seed, strm in ((OTHER_SEED, stream), (SEED, stream + 1)):
        assert verdicts(seed, strm) == plain
        assert wire.verify_batchable_wire(ctx, blob, seed, strm).tolist() == plain, (seed, strm)
    assert wire.verify_batchable_wire(ctx, blob, None, stream).tolist() == plain
    # ... and with the call's stream one less, group 1 draws under the stream its G items were built for: they pass, and only they
    w2 = verdicts(SEED, stream - 1)
    assert w2 == [0 if t == "H" or (t == "G" and group_of[plan[s][0]] == 1) else 1 for s, t in kinds]
    assert wire.verify_batchable_wire(ctx, blob, SEED, stream - 1).tolist() == w2
    ctx.close()
