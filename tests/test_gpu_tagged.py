"""Tagged presentations on the device (include/aeonflux_gpu.h "Presentation tags"; aeonflux_amd/csrc/tags.cuh k_sc_invert,
statements_tags.cpp) against the yardstick tests/tag_ref.py and the engine's own untagged calls:

  * the presentation rows of show_tagged are batch.show's from the same draws, for every surviving item;
  * T, the challenge and the responses are the yardstick's on a sample of items (pure Python is too slow for all 300);
  * EVERY item's tag opens: (m + n) * T == H, by the engine's multiscalar multiplication on s from Python integers;
  * verify_presentations_tagged accepts every surviving item and verify_tag_proofs agrees;
  * every output byte is the same in secret modes 0 and 2, under the plan self-check, in one pass and in two, and from the _dev forms;
  * a second show of the same credentials with fresh z_wide and seeds gives the same T and different everything else.

One case of 300 items per layout (tests/tagged_case.py) serves the counts 1 (one lane), 70 (more than a wave, no multiple of 64) and
300 (past the 256-item plan switch, two blocks of the inversion kernel).  Item 2 has m + n == 0: it fails, all zeros."""
import numpy as np
import pytest

from tests import tag_ref as TR
from tests.tagged_case import COUNTS, FAILING, LAYOUTS, SAMPLE, STRICT_LAYOUTS, L, Case, flatten, item_of

pytestmark = pytest.mark.gpu

ALL = [(k, p, False) for k, p in LAYOUTS] + [(k, p, True) for k, p in STRICT_LAYOUTS]
IDS = ["%s-p%d%s" % ("".join(map(str, k)), p, "-strict" if s else "") for k, p, s in ALL]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(kinds, p, strict):
        key = (tuple(kinds), p, strict)
        if key not in made:
            made[key] = Case(kinds, p, strict)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def survivors(cnt):
    return [i for i in range(cnt) if i != FAILING]


def expected_status(cnt):
    return [1 if i == FAILING else 0 for i in range(cnt)]


def assert_same_outputs(a, b, what):
    fa, fb = flatten(*a), flatten(*b)
    assert fa.keys() == fb.keys()
    for f in fa:
        assert np.array_equal(fa[f], fb[f]), (what, f)


def test_the_scope_generator_is_the_yardsticks(cases):
    from aeonflux_amd import batch
    c = cases(*ALL[0])
    for scope in (b"", b"a", b"x" * 111, b"y" * 112, bytes(range(256)) * 4):      # (112 bytes: the SHA-512 padding takes a second block)
        assert batch.tag_scope_generator(c.user, scope) == TR.scope_generator(scope), len(scope)
    assert c.H == TR.scope_generator(b"tests/tagged_case: scope one")


@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_presentation_bytes_statuses_and_the_failed_item(cases, kinds, p, strict, cnt):
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.shown_once(cnt)
    assert st.tolist() == expected_status(cnt)
    a = c.show_args(cnt)
    plain, pshape, pst = batch.show(c.user, a["kinds"], a["values"], a["t"], a["U"], a["V"], a["keypairs"], a["z_wide"], a["rng_seed"], a["enc_seeds"], a["M2"], a["m3"])
    assert not pst.any() and bytes(pshape) == bytes(shape)
    got, want = flatten(pres, tags, st), flatten(plain, {}, pst)
    keep = survivors(cnt)
    for f, w in want.items():
        if f == "status":
            continue
        for i in keep:
            assert np.array_equal(item_of(got[f], i), item_of(w, i)), (f, i)
    if cnt > FAILING:
        for f, g in got.items():
            if f != "status":
                assert not item_of(g, FAILING).any(), f          # every output row of the failed item is zeros


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_tag_bytes_equal_the_yardstick(cases, kinds, p, strict):
    from tests.pyref import ristretto as R
    from tests.pyref import statements as S
    c = cases(kinds, p, strict)
    sp = S.Params(c.params)
    for cnt in COUNTS:
        pres, tags, shape, st = c.shown_once(cnt)
        for i in [i for i in SAMPLE if i < cnt]:
            z = R.sc_from_wide(bytes(c.draws["z_wide"][i]))
            rst, ref = TR.tag_show(sp, p, c.H, bytes(c.nonce[i]), c.m[i], z, bytes(pres["C_y"][p][i]), bytes(c.draws["tag_seed"][i]))
            assert rst == S.OK
            assert bytes(tags["T"][i]) == ref["T"], (cnt, i)
            assert bytes(tags["challenge"][i]) == ref["challenge"], (cnt, i)
            assert [bytes(tags["responses"][k][i]) for k in range(2)] == ref["responses"], (cnt, i)
        if cnt > FAILING:
            z = R.sc_from_wide(bytes(c.draws["z_wide"][FAILING]))
            assert TR.tag_show(sp, p, c.H, bytes(c.nonce[FAILING]), c.m[FAILING], z, bytes(32), bytes(32))[0] == S.VERIFICATION_FAILURE
        if cnt > 1:
            assert bytes(tags["T"][0]) == c.H                                     # s == 1
            assert bytes(tags["T"][1]) == R.encode(R.neg(R.decode(c.H)))          # s == l - 1


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_every_tag_opens_to_H(cases, kinds, p, strict):
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.shown_once(300)
    keep = survivors(300)
    s = np.stack([np.frombuffer(((c.m[i] + c.nn[i]) % L).to_bytes(32, "little"), np.uint8) for i in keep])
    out, ok = batch.multiscalar_mul(c.user, s[None], tags["T"][keep][None])
    assert ok.all()
    assert all(bytes(row) == c.H for row in out)
    assert len({bytes(t) for t in tags["T"][keep]}) == len(keep)      # distinct (m, n): distinct tags


@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_the_verifiers_accept_what_the_prover_made(cases, kinds, p, strict, cnt):
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.shown_once(cnt)
    nonce = c.cut(c.nonce, cnt)
    want = expected_status(cnt)                                              # the failed item's rows are zeros: rejected
    assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, nonce, tags).tolist() == want
    assert batch.verify_tag_proofs(c.user, p, c.H, pres["C_y"][p], nonce, tags).tolist() == want
    plain = batch.verify_presentations(c.issuer, shape, pres).tolist()
    assert plain == want


def _dev_show(c, cnt):
    from aeonflux_amd import batch
    from tests.helpers import DevMem
    a = c.show_args(cnt)
    n, hs, nsp = c.n, c.hs, c.nsp
    dev = lambda x: DevMem(x)
    out = lambda *shape: DevMem(np.full(shape, 0xEE, np.uint8))
    creds = dict(values=dev(a["values"]), t=dev(a["t"]), U=dev(a["U"]), V=dev(a["V"]))
    if nsp:
        creds.update(M2=dev(a["M2"]), m3=dev(a["m3"]))
    kp = {f: dev(v) for f, v in a["keypairs"].items()} if a["keypairs"] else None
    rnd = dict(z_wide=dev(a["z_wide"]), rng_seed=dev(a["rng_seed"]), enc_seeds=dev(a["enc_seeds"]) if nsp else None)
    po = {f: out(cnt, 32) for f in ("challenge", "C_x_0", "C_x_1", "C_V")}
    po.update(responses=out(3 + hs, cnt, 32), C_y=out(n, cnt, 32), attr_values=DevMem(np.zeros((n, cnt, 32), np.uint8)))
    po["enc"] = [{f: out(*((6, cnt, 32) if f == "responses" else (cnt, 32))) for f in batch.ENC_FIELDS} for _ in range(nsp)]
    to = dict(T=out(cnt, 32), challenge=out(cnt, 32), responses=out(2, cnt, 32))
    d_nonce, d_seed, d_st = dev(c.cut(c.nonce, cnt)), dev(c.cut(c.draws["tag_seed"], cnt)), out(cnt)
    shape = batch.show_tagged_dev(c.user, c.kinds, creds, kp, rnd, c.p, c.H, d_nonce, d_seed, cnt, po, to, d_st)
    # the verifiers on the device rows the prover wrote (another context: wait for the user's stream first)
    c.user.synchronize()
    v_st, t_st = out(cnt), out(cnt)
    batch.verify_presentations_tagged_dev(c.issuer, shape, po, c.p, c.H, d_nonce, to, cnt, v_st)
    batch.verify_tag_proofs_dev(c.issuer, c.p, c.H, po["C_y"].ptr + c.p * cnt * 32, d_nonce, to, cnt, t_st)
    c.issuer.synchronize()
    pres = {f: po[f].numpy() for f in batch.PRES_FIELDS}
    pres["enc"] = [{f: d[f].numpy() for f in batch.ENC_FIELDS} for d in po["enc"]]
    return (pres, {f: to[f].numpy() for f in to}, d_st.numpy()), shape, v_st.numpy(), t_st.numpy()


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_outputs_do_not_depend_on_how_the_plan_is_built(cases, kinds, p, strict):
    import aeonflux_amd as afx
    c = cases(kinds, p, strict)
    for cnt in (70, 300):
        pres, tags, shape, st = c.shown_once(cnt)
        base = (pres, tags, st)
        for mode in (0, 2):
            c.user.set_secret_independent_addressing(mode)
            got = c.show_tagged(cnt)
            assert_same_outputs(base, (got[0], got[1], got[3]), ("secret mode", mode, cnt))
        c.user.set_plan_variants(afx.VARIANT_SELFCHECK)
        got = c.show_tagged(cnt)
        c.user.set_plan_variants(0)
        assert_same_outputs(base, (got[0], got[1], got[3]), ("self-check", cnt))
        dev, dshape, v_st, t_st = _dev_show(c, cnt)
        assert bytes(dshape) == bytes(shape)
        assert_same_outputs(base, dev, ("_dev", cnt))
        assert v_st.tolist() == expected_status(cnt) and t_st.tolist() == expected_status(cnt)
    # one pass against two: 300 items at 256 items per pass
    pres, tags, shape, st = c.shown_once(300)
    for ctx in (c.user, c.issuer):
        ctx.set_chunk_items(256)
    try:
        from aeonflux_amd import batch
        got = c.show_tagged(300)
        assert_same_outputs((pres, tags, st), (got[0], got[1], got[3]), "two passes")
        assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, c.nonce, tags).tolist() == expected_status(300)
        assert batch.verify_tag_proofs(c.issuer, p, c.H, pres["C_y"][p], c.nonce, tags).tolist() == expected_status(300)
    finally:
        for ctx in (c.user, c.issuer):
            ctx.set_chunk_items(0)


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_a_second_show_gives_the_same_tag_and_nothing_else(cases, kinds, p, strict):
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    cnt = 70
    pres, tags, shape, st = c.shown_once(cnt)
    pres2, tags2, shape2, st2 = c.show_tagged(cnt, draws=c.fresh_draws())
    assert st2.tolist() == st.tolist()
    assert np.array_equal(tags["T"], tags2["T"])
    other = c.show_tagged(cnt, H=batch.tag_scope_generator(c.user, b"another scope"))[1]
    for i in survivors(cnt):
        assert not np.array_equal(tags["challenge"][i], tags2["challenge"][i]) and not np.array_equal(tags["responses"][:, i], tags2["responses"][:, i]), i
        assert not np.array_equal(pres["C_y"][p][i], pres2["C_y"][p][i]) and not np.array_equal(pres["challenge"][i], pres2["challenge"][i]), i
        assert not np.array_equal(tags["T"][i], other["T"][i]), i           # another scope: another tag


def test_bad_calls_are_refused_before_anything_is_written(cases):
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    kinds, p, strict = ALL[1]
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.shown_once(70)
    nonce = c.cut(c.nonce, 70)
    for H in (bytes(32), b"\xff" * 32):
        for call in (lambda: c.show_tagged(70, H=H), lambda: batch.verify_presentations_tagged(c.issuer, shape, pres, p, H, nonce, tags),
                     lambda: batch.verify_tag_proofs(c.user, p, H, pres["C_y"][p], nonce, tags)):
            with pytest.raises(afx.AfxError) as e:
                call()
            assert e.value.rc == afx.E_BAD_ARGS
    # a position that is no hidden scalar: the prover refuses, the verifier fails every item
    for bad_p in (1, 2, 3, 4, 99):
        with pytest.raises(afx.AfxError) as e:
            batch.show_tagged(c.user, **{k: v for k, v in c.show_args(70).items()}, position=bad_p, H=c.H, nonce=nonce, tag_seed=c.cut(c.draws["tag_seed"], 70))
        assert e.value.rc == afx.E_BAD_ARGS
        assert batch.verify_presentations_tagged(c.issuer, shape, pres, bad_p, c.H, nonce, tags).tolist() == [1] * 70
    assert batch.verify_tag_proofs(c.user, 99, c.H, pres["C_y"][p], nonce, tags).tolist() == [1] * 70
    # and a good call still works afterwards
    assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, nonce, tags).tolist() == expected_status(70)


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_small_host_calls_keep_their_plans_and_the_kept_plan_gives_the_same_bytes(cases, kinds, p, strict):
    """the host-pointer forms stage the cells of H and the inverse rows in their own scratch, so their plans are kept (a key of their own):
    the second call of a size reuses the first's plan, on other staging addresses, and must write the same bytes"""
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    for cnt in (1, 70):
        first = c.show_tagged(cnt)
        u0, i0 = c.user.plan_cache_stats(), c.issuer.plan_cache_stats()
        again = c.show_tagged(cnt)
        other = c.show_tagged(cnt, draws=c.fresh_draws())          # the same plan on other data
        assert c.user.plan_cache_stats()["hits"] >= u0["hits"] + 2
        assert_same_outputs((first[0], first[1], first[3]), (again[0], again[1], again[3]), ("kept plan", cnt))
        assert np.array_equal(first[1]["T"], other[1]["T"]) and other[3].tolist() == expected_status(cnt)
        nonce = c.cut(c.nonce, cnt)
        for pres, tags in ((first[0], first[1]), (other[0], other[1]), (again[0], again[1])):
            assert batch.verify_presentations_tagged(c.issuer, first[2], pres, p, c.H, nonce, tags).tolist() == expected_status(cnt)
            assert batch.verify_tag_proofs(c.issuer, p, c.H, pres["C_y"][p], nonce, tags).tolist() == expected_status(cnt)
        assert c.issuer.plan_cache_stats()["hits"] >= i0["hits"] + 4
    # another position of the same layout is another plan: the layout with two hidden scalars, tagged at the first
    if kinds.count(1) > 1:
        q = kinds.index(1)
        assert q != p
        a = c.show_args(70)
        nonce = c.cut(c.nonce, 70).copy()
        nonce[:, 4:] = 0
        nonce[:3, :4] = 9                                           # (the chosen sums belong to position p)
        pres, tags, shape, st = batch.show_tagged(c.user, **a, position=q, H=c.H, nonce=nonce, tag_seed=c.cut(c.draws["tag_seed"], 70))
        assert not st.any()
        assert batch.verify_presentations_tagged(c.issuer, shape, pres, q, c.H, nonce, tags).tolist() == [0] * 70
        assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, nonce, tags).tolist() == [1] * 70


def test_without_the_symmetric_key_every_item_fails_with_zeros(cases):
    """hidden group elements and no keypairs: AFX_ST_NO_SYMMETRIC_KEY for every item, as afx_show answers, and every output row zeros"""
    from aeonflux_amd import batch
    kinds, p, strict = ALL[1]
    c = cases(kinds, p, strict)
    for cnt in (70, 300):
        a = dict(c.show_args(cnt), keypairs=None)
        pres, tags, shape, st = batch.show_tagged(c.user, **a, position=p, H=c.H, nonce=c.cut(c.nonce, cnt), tag_seed=c.cut(c.draws["tag_seed"], cnt))
        assert st.tolist() == [3] * cnt
        for f, g in flatten(pres, tags, st).items():
            if f != "status":
                assert not g.any(), f
    good = c.show_tagged(70)
    assert good[3].tolist() == expected_status(70)


def test_a_dev_call_that_outgrows_the_lanes_tag_buffer_still_reads_the_right_scope(cases):
    """the lane remembers which H its buffer holds, and a larger call replaces that buffer: the new one must receive H again.  300 items
    (the buffer's first megabyte), then 21 000 (the same tags, tiled: 64 bytes an item) under the same scope, then 300 again; a stale or
    zero H would reject every honest item"""
    from aeonflux_amd import batch
    from tests.helpers import DevMem
    kinds, p, strict = ALL[0]
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.shown_once(300)
    ctx = c.issuer                                   # (a context whose lane buffer has only served host-pointer calls so far)
    for reps in (1, 70, 1):
        cnt = 300 * reps
        tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1)) if a.ndim == 2 else np.tile(a, (1, reps, 1)))
        d_cy, d_n = DevMem(tile(pres["C_y"][p])), DevMem(tile(c.nonce))
        d_tags = {f: DevMem(tile(tags[f])) for f in tags}
        d_st = DevMem(np.full(cnt, 0xEE, np.uint8))
        batch.verify_tag_proofs_dev(ctx, p, c.H, d_cy, d_n, d_tags, cnt, d_st)
        ctx.synchronize()
        assert d_st.numpy().tolist() == expected_status(300) * reps, reps
