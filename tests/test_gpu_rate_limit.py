"""The rate limit end to end on the device: "at most N shows per credential and scope" is afx_verify_presentations_tagged_dev followed by
afx_tagset_spend_dev on the T and status rows the verification has just written (include/aeonflux_gpu.h "Presentation tags", "The
spent-tag set") - one stream, no synchronisation between the two, the status rows as status_in, the [count] point rows of T as
[count][32] tags, zero rows for items the prover could not make.  What rests on it:

  * a presentation that fails verification burns nobody's tag (AFX_TAG_SKIPPED), not even the tag it carries;
  * a second show under the same (credential, counter, scope) is refused whatever its fresh proof bytes are;
  * another counter or another scope is another tag.

The reference uses no engine output: it is the sequential loop of tests/tagset_model.Model over the items whose expected status is 0,
keyed by ((m + n) mod l, scope) from the case's Python integers.  Expected statuses come from construction: honest 0, damaged 1,
m + n == 0 1.  Every comparison is exact.

Batches gather the arrays of tests/tagged_case.Case through an index list, so one credential appears several times in a call under
counters chosen here; z_wide, rng_seed, enc_seeds and tag_seed are fresh per item, so repeats differ in every byte but T.  Everything
runs on the issuer's context with pipelining off (with it on, independence of successive _dev calls is the caller's duty); every call of
a test is queued before anything is read back, then one synchronize.  Afterwards the host-pointer forms (verify_presentations_tagged,
then TagSet.spend on its numpy outputs) must give the model's answers too, into a second set with the same salt."""
import hashlib

import numpy as np
import pytest

from tests import tag_ref as TR
from tests import tagset_model as M
from tests.tagged_case import FAILING, L, Case, sc

pytestmark = pytest.mark.gpu

LAYOUTS = [([1], 0), ([1, 0, 2, 4], 0)]
IDS = ["%s-p%d" % ("".join(map(str, k)), p) for k, p in LAYOUTS]
SCOPES = (b"tests/tagged_case: scope one", b"tests/test_gpu_rate_limit: scope two")
SALT = hashlib.shake_256(b"tests/test_gpu_rate_limit salt").digest(32)
CAPACITY = 1024


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(kinds, p):
        key = (tuple(kinds), p)
        if key not in made:
            made[key] = Case(kinds, p)
            made[key].issuer.set_pipelining(0)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def generator(c, scope):
    from aeonflux_amd import batch
    H = batch.tag_scope_generator(c.user, scope)
    assert H == TR.scope_generator(scope)
    return H


class Shown:
    """one tagged show of the credentials idx[k] under the counters counters[k] (None: the case's own) and the scope's generator"""

    def __init__(self, c, idx, counters, scope):
        from aeonflux_amd import batch
        self.c, self.idx, self.cnt, self.scope = c, list(idx), len(idx), scope
        self.H = generator(c, scope)
        cnt = self.cnt
        self.n = [c.nn[i] if n is None else n % L for i, n in zip(idx, counters)]
        self.nonce = np.stack([sc(n) for n in self.n])
        self.draws = c.fresh_draws()
        g = lambda a: None if a is None else np.ascontiguousarray(a[..., self.idx, :])
        cut = lambda a: np.ascontiguousarray(a[..., :cnt, :])
        kp = {f: g(v) for f, v in c.keypairs.items()} if c.keypairs else None
        self.pres, self.tags, self.shape, st = batch.show_tagged(c.user, c.kinds, g(c.values), g(c.t), g(c.U), g(c.V), kp, cut(self.draws["z_wide"]), cut(self.draws["rng_seed"]),
                                                                 c.p, self.H, self.nonce, cut(self.draws["tag_seed"]), cut(self.draws["enc_seeds"]), g(c.M2), g(c.m3))
        # The tag is T = (m + n)^-1 * H: two credentials with m1 + n1 == m2 + n2 share a tag by the protocol, so the model's key is the sum
        # (and the scope), not the credential's index
        sums = [(c.m[i] + n) % L for i, n in zip(idx, self.n)]
        self.keys = [(s, scope) for s in sums]
        self.status = [1 if s == 0 else 0 for s in sums]                   # s == 0 has no inverse: the prover fails, every row zeros
        assert st.tolist() == self.status
        for k in range(cnt):
            if self.status[k]:
                assert not self.tags["T"][k].any()

    def damaged(self, damage):
        """copies of the host rows with the damage done, and the statuses a verifier must give"""
        pres = dict(self.pres)
        tags = {f: v.copy() for f, v in self.tags.items()}
        status = list(self.status)
        for d in damage:
            if d[0] == "response":
                tags["responses"][1, d[1], 0] ^= 1
            else:
                tags["T"][d[1]] = self.tags["T"][d[2]]
                assert self.status[d[2]] == 0 and not np.array_equal(self.tags["T"][d[1]], self.tags["T"][d[2]])
            status[d[1]] = 1
        return pres, tags, status


class Flow:
    """verify_presentations_tagged_dev, then TagSet.spend_dev on the rows it wrote, step after step on one stream; nothing read until finish()"""

    def __init__(self, c):
        from aeonflux_amd import batch
        self.c = c
        self.ts = batch.TagSet(c.issuer, CAPACITY, SALT)
        self.host_ts = batch.TagSet(c.issuer, CAPACITY, SALT)
        self.steps = []

    def close(self):
        self.ts.close()
        self.host_ts.close()

    def step(self, sh, damage=()):
        from aeonflux_amd import batch
        from tests.helpers import DevMem
        c, cnt = self.c, sh.cnt
        po = {f: DevMem(sh.pres[f]) for f in batch.PRES_FIELDS}
        po["enc"] = [{f: DevMem(d[f]) for f in batch.ENC_FIELDS} for d in sh.pres["enc"]]
        to = {f: DevMem(sh.tags[f]) for f in sh.tags}
        hip = DevMem.hip()
        for d in damage:                                                    # on the device rows, between show and verify
            if d[0] == "response":                                          # (a) one byte of the tag's second response
                byte = np.array([sh.tags["responses"][1, d[1], 0] ^ 1], np.uint8)
                assert hip.hipMemcpy(to["responses"].ptr + 32 * (cnt + d[1]), byte.ctypes.data, 1, 1) == 0
            else:                                                           # (b) T replaced by another accepted item's
                assert hip.hipMemcpy(to["T"].ptr + 32 * d[1], to["T"].ptr + 32 * d[2], 32, 3) == 0
        d_nonce, d_st = DevMem(sh.nonce), DevMem(np.full(cnt, 0xEE, np.uint8))
        d_seen, d_zero, d_has = DevMem(np.full(cnt, 0xEE, np.uint8)), DevMem(np.zeros((1, 32), np.uint8)), DevMem(np.full(1, 0xEE, np.uint8))
        batch.verify_presentations_tagged_dev(c.issuer, sh.shape, po, c.p, sh.H, d_nonce, to, cnt, d_st)
        self.ts.spend_dev(to["T"], d_st, cnt, d_seen)
        self.ts.contains_dev(d_zero, 1, d_has)
        self.steps.append(dict(sh=sh, damage=damage, st=d_st, seen=d_seen, has=d_has, keep=(po, to, d_nonce, d_zero)))

    def finish(self):
        """-> the model's answers per step, after comparing everything the device and the host forms wrote with them"""
        from aeonflux_amd import batch
        c = self.c
        c.issuer.synchronize()
        model, answers, accepted = M.Model(), [], []
        for k, s in enumerate(self.steps):
            sh = s["sh"]
            pres, tags, status = sh.damaged(s["damage"])
            want = model.spend(sh.keys, status)
            answers.append(want)
            assert s["st"].numpy().tolist() == status, k
            assert s["seen"].numpy().tolist() == want, k
            assert s["has"].numpy().tolist() == [0], k                      # 32 zero bytes - a failed item's T row - are never in the set
            assert np.array_equal(s["keep"][1]["T"].numpy(), tags["T"]), k  # the rows the set read
            accepted += [bytes(tags["T"][i]) for i in range(sh.cnt) if status[i] == 0]
            # the host-pointer forms, into a set of their own
            h_st = batch.verify_presentations_tagged(c.issuer, sh.shape, pres, c.p, sh.H, sh.nonce, tags)
            assert h_st.tolist() == status, k
            assert self.host_ts.spend(tags["T"], h_st).tolist() == want, k
        assert len(set(accepted)) == len(model.tags)                        # equal keys, equal bytes; other keys, other bytes
        rows = np.frombuffer(b"".join(sorted(set(accepted))), np.uint8).reshape(-1, 32)
        for ts in (self.ts, self.host_ts):
            assert ts.size() == (len(model.tags), CAPACITY)
            assert ts.contains(rows).tolist() == [1] * len(rows)
            assert ts.contains(np.zeros((1, 32), np.uint8)).tolist() == [0]
        return answers


# ---- the first call: 300 items ------------------------------------------------------------------------------------------------------
GROUPS = [(3, 17), (10, 100), (63, 64), (255, 256), (5, 70, 260)]          # positions that show one (credential, counter): within a wave, across
                                                                           # waves, over a wave edge, over the block edge, one in each of three
FOUR = (20, 21, 22, 23)                                                    # one credential under the counters 0 .. 3
SHARED = (30, 31)                                                          # two credentials whose sums are equal


def first_call(c):
    idx, counters = list(range(300)), [None] * 300                        # position i: credential i under the case's counter - position 2 has m + n == 0
    for g in GROUPS:
        for pos in g[1:]:
            idx[pos] = g[0]
    for n, pos in enumerate(FOUR):
        idx[pos], counters[pos] = 50, n
    counters[SHARED[0]] = (c.m[31] + c.nn[31] - c.m[30]) % L
    return idx, counters


def expected_first():
    want = [M.FRESH] * 300
    want[FAILING] = M.SKIPPED
    for g in GROUPS:
        for pos in g[1:]:
            want[pos] = M.SPENT
    want[SHARED[1]] = M.SPENT
    return want


@pytest.mark.parametrize("kinds,p", LAYOUTS, ids=IDS)
def test_repeats_in_one_call_and_replays_in_the_next(cases, kinds, p):
    from tests.pyref import ristretto as R
    from tests.pyref import statements as S
    c = cases(kinds, p)
    idx, counters = first_call(c)
    one = Shown(c, idx, counters, SCOPES[0])
    assert one.status == [1 if k == FAILING else 0 for k in range(300)]
    # the second call: 40 of the first again under fresh draws, and 30 (credential, counter) pairs nobody has shown
    again = list(range(40, 80))
    two = Shown(c, [idx[k] for k in again] + list(range(100, 130)), [one.n[k] for k in again] + [c.nn[i] + 7 for i in range(100, 130)], SCOPES[0])
    for k, pos in enumerate(again):                                         # the same tag, nothing else the same
        assert np.array_equal(two.tags["T"][k], one.tags["T"][pos])
        assert not np.array_equal(two.tags["challenge"][k], one.tags["challenge"][pos]) and not np.array_equal(two.pres["challenge"][k], one.pres["challenge"][pos])
    for g in GROUPS:
        for pos in g[1:]:
            assert np.array_equal(one.tags["T"][pos], one.tags["T"][g[0]]) and not np.array_equal(one.tags["responses"][:, pos], one.tags["responses"][:, g[0]])
    flow = Flow(c)
    try:
        flow.step(one)
        flow.step(two)
        answers = flow.finish()
    finally:
        flow.close()
    # what the model said is what the issue of a rate limit needs: the lowest index of each group fresh, the others spent; the four
    # counters four fresh tags; the replays spent, the new items fresh
    assert answers[0] == expected_first()
    assert len({bytes(one.tags["T"][pos]) for pos in FOUR + (50,)}) == 5
    assert answers[1] == [M.SPENT] * 40 + [M.FRESH] * 30
    # the bytes that were spent are the yardstick's tags
    sp = S.Params(c.params)
    for pos in (0, 1, 3, 17, 20, 23, 30, 299):
        z = R.sc_from_wide(bytes(one.draws["z_wide"][pos]))
        rst, ref = TR.tag_show(sp, p, one.H, bytes(one.nonce[pos]), c.m[idx[pos]], z, bytes(one.pres["C_y"][p][pos]), bytes(one.draws["tag_seed"][pos]))
        assert rst == S.OK and bytes(one.tags["T"][pos]) == ref["T"], pos


@pytest.mark.parametrize("kinds,p", LAYOUTS, ids=IDS)
def test_a_second_scope_is_another_limit_in_the_same_set(cases, kinds, p):
    c = cases(kinds, p)
    idx, counters = first_call(c)
    idx, counters = idx[:70], counters[:70]
    one = Shown(c, idx, counters, SCOPES[0])
    other = Shown(c, idx, counters, SCOPES[1])
    replay = Shown(c, idx[40:60], [other.n[k] for k in range(40, 60)], SCOPES[1])
    for k in range(70):
        if k != FAILING:
            assert not np.array_equal(one.tags["T"][k], other.tags["T"][k])
    flow = Flow(c)
    try:
        for sh in (one, other, replay):
            flow.step(sh)
        answers = flow.finish()
    finally:
        flow.close()
    assert answers[0] == expected_first()[:70]
    assert answers[1] == answers[0]                                         # every pair is fresh again under the second scope
    assert answers[2] == [M.SPENT] * 20


@pytest.mark.parametrize("kinds,p", LAYOUTS, ids=IDS)
def test_a_presentation_that_fails_burns_nobodys_tag(cases, kinds, p):
    c = cases(kinds, p)
    idx, counters = first_call(c)
    idx, counters = idx[:70], counters[:70]
    one = Shown(c, idx, counters, SCOPES[0])
    # (a) a byte of the tag's response at 12; (b) at 33 the T of 40 - an honest item BEHIND it, which an unskipped 33 would make spent - and
    # at 45 the T of 7, in front of it
    damage = (("response", 12), ("T", 33, 40), ("T", 45, 7))
    later = [12, 33, 45, 40, 7]
    two = Shown(c, [idx[k] for k in later], [one.n[k] for k in later], SCOPES[0])
    flow = Flow(c)
    try:
        flow.step(one, damage)
        flow.step(two)
        answers = flow.finish()
    finally:
        flow.close()
    want = expected_first()[:70]
    for pos in (12, 33, 45):
        want[pos] = M.SKIPPED
    assert answers[0] == want                                               # 40 and 7 fresh: the honest owners are answered as if nothing had happened
    assert answers[1] == [M.FRESH, M.FRESH, M.FRESH, M.SPENT, M.SPENT]      # a later honest show of what the damaged items stood for is fresh
