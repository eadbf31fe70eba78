"""Damaged tags on the device: the single damages of tests/test_tag_ref.py, one kind per item round-robin over the 300 items of a case
(tests/tagged_case.py), every item damaged except a stride of honest controls.  The expected status is known by construction -
damaged => 1, control => 0 (item 2, whose m + n is 0, has failed at the prover and stays 1); five of the damages leave every value
intact and break only its encoding (a response or the challenge + l, T with bit 255 set, T as p - s) - and the yardstick's verdict is checked
on the reference sample as well.  The whole-batch transplant (every tag row moved on by one item) fails every item while the batch as
shown passes.  Statuses are the same in secret modes 0, 1 and 2, and afx_verify_tag_proofs agrees with the combined call."""
import numpy as np
import pytest

from tests import tag_ref as TR
from tests.tagged_case import FAILING, LAYOUTS, SAMPLE, STRICT_LAYOUTS, TOTAL, L, Case

pytestmark = pytest.mark.gpu

ALL = [(k, p, False) for k, p in LAYOUTS] + [(k, p, True) for k, p in STRICT_LAYOUTS]
IDS = ["%s-p%d%s" % ("".join(map(str, k)), p, "-strict" if s else "") for k, p, s in ALL]
DAMAGES = ("a bit of T", "n + 1", "n + l", "response z", "response s", "the challenge", "T = identity encoding", "another item's tag",
           "response z + l", "response s + l", "challenge + l", "T with bit 255", "T as p - s")
STRIDE = len(DAMAGES) + 1          # item i carries damage i % STRIDE; the last residue is an honest control
P = 2 ** 255 - 19
# ... and of the received C_y[p] row afx_verify_tag_proofs is given, every tag row honest
CY_DAMAGES = ("C_y[p] + l", "C_y[p] with bit 255", "C_y[p] as p - s")
CY_STRIDE = len(CY_DAMAGES) + 1


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


def alias(row, add):
    """the row's integer + add as 32 bytes: the same value mod l (add = l) or to a decoder that drops bit 255 (add = 2^255)"""
    return np.frombuffer((int.from_bytes(bytes(row), "little") + add).to_bytes(32, "little"), np.uint8)


def negated(row):
    """p - s: the field element -s, which a decoder without the sign test on s takes for the same point (s = 0 gives p itself)"""
    return np.frombuffer((P - int.from_bytes(bytes(row), "little")).to_bytes(32, "little"), np.uint8)


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
        elif k == 8:
            tg["responses"][0, i] = alias(tags["responses"][0, i], L)
        elif k == 9:
            tg["responses"][1, i] = alias(tags["responses"][1, i], L)
        elif k == 10:
            tg["challenge"][i] = alias(tags["challenge"][i], L)
        elif k == 11:
            tg["T"][i] = alias(tags["T"][i], 2 ** 255)
        elif k == 12:
            tg["T"][i] = negated(tags["T"][i])
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
    for i in sorted(set(SAMPLE) | set(range(3, 3 + STRIDE))):          # (every damage at least once)
        ref = TR.tag_verify(sp, p, c.H, bytes(nonce[i]), bytes(pres["C_y"][p][i]),
                            dict(T=bytes(tg["T"][i]), challenge=bytes(tg["challenge"][i]), responses=[bytes(tg["responses"][k][i]) for k in range(2)]))
        assert ref == int(want[i]), (i, DAMAGES[i % STRIDE] if i % STRIDE < len(DAMAGES) else "control")


@pytest.mark.parametrize("kinds,p,strict", ALL, ids=IDS)
def test_aliases_of_the_received_commitment_fail_the_tag_proof(cases, kinds, p, strict):
    """afx_verify_tag_proofs on a C_y[p] row whose item i carries CY_DAMAGES[i % CY_STRIDE]: the value is the same point to a decoder
    that drops bit 255 or skips the sign test, so only the decode of that row refuses it.  The yardstick states the verdict first."""
    from aeonflux_amd import batch
    from tests.pyref import statements as S
    c = cases(kinds, p, strict)
    pres, tags, shape, st = c.honest
    Cy = pres["C_y"][p].copy()
    want = np.zeros(TOTAL, np.uint8)
    for i in range(TOTAL):
        k = i % CY_STRIDE
        if k < len(CY_DAMAGES):
            want[i] = 1
            Cy[i] = (alias(Cy[i], L), alias(Cy[i], 2 ** 255), negated(Cy[i]))[k]
    want[FAILING] = 1
    sp = S.Params(c.params)
    for i in sorted(set(SAMPLE) | set(range(3, 3 + CY_STRIDE))):
        ref = TR.tag_verify(sp, p, c.H, bytes(c.nonce[i]), bytes(Cy[i]),
                            dict(T=bytes(tags["T"][i]), challenge=bytes(tags["challenge"][i]), responses=[bytes(tags["responses"][k][i]) for k in range(2)]))
        assert ref == int(want[i]), (i, CY_DAMAGES[i % CY_STRIDE] if i % CY_STRIDE < len(CY_DAMAGES) else "control")
    got = batch.verify_tag_proofs(c.user, p, c.H, Cy, c.nonce, tags)
    assert got.tolist() == want.tolist(), [(i, CY_DAMAGES[i % CY_STRIDE] if i % CY_STRIDE < len(CY_DAMAGES) else "control") for i in np.nonzero(got != want)[0]]


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
