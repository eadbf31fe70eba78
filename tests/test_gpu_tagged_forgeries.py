"""Damaged tags on the device: the single damages of tests/test_tag_ref.py, one kind per item round-robin over the 300 items of a case
(tests/tagged_case.py), every item damaged except a stride of honest controls.  The expected status is known by construction -
damaged => 1, control => 0 (item 2, whose m + n is 0, has failed at the prover and stays 1) - and the yardstick's verdict is checked
on the reference sample as well.  The whole-batch transplant (every tag row moved on by one item) fails every item while the batch as
shown passes.  Statuses are the same in secret modes 0, 1 and 2, and afx_verify_tag_proofs agrees with the combined call."""
import numpy as np
import pytest

from tests import tag_ref as TR
from tests.tagged_case import FAILING, LAYOUTS, SAMPLE, STRICT_LAYOUTS, TOTAL, L, Case

pytestmark = pytest.mark.gpu

ALL = [(k, p, False) for k, p in LAYOUTS] + [(k, p, True) for k, p in STRICT_LAYOUTS]
IDS = ["%s-p%d%s" % ("".join(map(str, k)), p, "-strict" if s else "") for k, p, s in ALL]
DAMAGES = ("a bit of T", "n + 1", "n + l", "response z", "response s", "the challenge", "T = identity encoding", "another item's tag")
STRIDE = len(DAMAGES) + 1          # item i carries damage i % STRIDE; the last residue is an honest control


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(kinds, p, strict):
        key = (tuple(kinds), p, strict)
        if key not in made:
            c = Case(kinds, p, strict)
            c.honest = c.show_tagged(TOTAL)
            made[key] = c
        return made[key]
    yield get
    for c in made.values():
        c.close()


def damaged_batch(c):
    """(nonce, tags, expected status) with item i damaged by DAMAGES[i % STRIDE]"""
    pres, tags, shape, st = c.honest
    nonce = c.nonce.copy()
    tg = {f: v.copy() for f, v in tags.items()}
    want = np.zeros(TOTAL, np.uint8)
    for i in range(TOTAL):
        k = i % STRIDE
        if k < len(DAMAGES):
            want[i] = 1
        bit = 1 << (i % 8)
        byte = (7 * i) % 31
        if k == 0:
            tg["T"][i, byte] ^= bit
        elif k == 1:
            nonce[i] = np.frombuffer((c.nn[i] + 1).to_bytes(32, "little"), np.uint8)
        elif k == 2:
            nonce[i] = np.frombuffer((c.nn[i] + L).to_bytes(32, "little"), np.uint8)
        elif k == 3:
            tg["responses"][0, i, byte] ^= bit
        elif k == 4:
            tg["responses"][1, i, byte] ^= bit
        elif k == 5:
            tg["challenge"][i, byte] ^= bit
        elif k == 6:
            tg["T"][i] = 0
        elif k == 7:
            j = (i + STRIDE) % TOTAL if (i + STRIDE) % TOTAL != FAILING else (i + 2 * STRIDE) % TOTAL
            for f in tg:
                tg[f][..., i, :] = tags[f][..., j, :]
    want[FAILING] = 1
    return nonce, tg, want


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_single_damages_fail_and_controls_pass(cases, kinds, p, strict):
    from aeonflux_amd import batch
    from tests.pyref import statements as S
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.honest
    assert st.tolist() == [1 if i == FAILING else 0 for i in range(TOTAL)]
    nonce, tg, want = damaged_batch(c)
    assert 0 < int((want == 0).sum()) < TOTAL // 8 + 2          # a stride of controls, everything else damaged
    by_mode = {}
    for mode in (0, 1, 2):
        c.issuer.set_secret_independent_addressing(mode)
        by_mode[mode] = batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, nonce, tg)
    c.issuer.set_secret_independent_addressing(2)
    for mode, got in by_mode.items():
        assert got.tolist() == want.tolist(), (mode, [(i, DAMAGES[i % STRIDE] if i % STRIDE < len(DAMAGES) else "control") for i in np.nonzero(got != want)[0]])
    assert batch.verify_tag_proofs(c.user, p, c.H, pres["C_y"][p], nonce, tg).tolist() == want.tolist()
    # the yardstick's verdict on the reference sample
    sp = S.Params(c.params)
    for i in SAMPLE:
        ref = TR.tag_verify(sp, p, c.H, bytes(nonce[i]), bytes(pres["C_y"][p][i]),
                            dict(T=bytes(tg["T"][i]), challenge=bytes(tg["challenge"][i]), responses=[bytes(tg["responses"][k][i]) for k in range(2)]))
        assert ref == int(want[i]), (i, DAMAGES[i % STRIDE] if i % STRIDE < len(DAMAGES) else "control")


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_a_damaged_presentation_fails_whatever_its_tag(cases, kinds, p, strict):
    """one status for both: the tag proof of item i is intact, its presentation is not"""
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.honest
    bad = dict(pres, C_V=pres["C_V"].copy(), responses=pres["responses"].copy())
    bad["C_V"][5] = pres["C_V"][6]
    bad["responses"][0, 9, 3] ^= 4            # the presentation's z: the tag proof has a response z of its own
    got = batch.verify_presentations_tagged(c.issuer, shape, bad, p, c.H, c.nonce, tags)
    assert got.tolist() == [1 if i in (FAILING, 5, 9) else 0 for i in range(TOTAL)]
    assert batch.verify_tag_proofs(c.user, p, c.H, pres["C_y"][p], c.nonce, tags).tolist() == [1 if i == FAILING else 0 for i in range(TOTAL)]


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_the_whole_batch_transplant_fails_every_item(cases, kinds, p, strict):
    from aeonflux_amd import batch
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.honest
    assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, c.nonce, tags).tolist() == [1 if i == FAILING else 0 for i in range(TOTAL)]
    rotated = {f: np.roll(v, 1, axis=v.ndim - 2) for f, v in tags.items()}
    assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, c.H, c.nonce, rotated).tolist() == [1] * TOTAL
    assert batch.verify_tag_proofs(c.user, p, c.H, pres["C_y"][p], c.nonce, rotated).tolist() == [1] * TOTAL
    # tags that verify under one scope do not under another
    other = batch.tag_scope_generator(c.user, b"another scope")
    assert batch.verify_presentations_tagged(c.issuer, shape, pres, p, other, c.nonce, tags).tolist() == [1] * TOTAL
