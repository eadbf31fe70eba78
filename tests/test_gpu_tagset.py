"""The spent-tag set on the device (include/aeonflux_gpu.h "The spent-tag set"; aeonflux_amd/csrc/tagset.cuh k_tagset_claim,
k_tagset_resolve, k_tagset_contains; tagset.cpp) against the sequential loop it is specified to equal, run on a Python set
(tests/tagset_model.py).  Tags are arbitrary 32-byte strings chosen with hashlib, so the cases aim at slots: no group arithmetic.

The cases (tests/tagset_model.py CASES; tests/test_tagset_on_host.py runs the same ones on the lane bodies): counts 1, 63, 64, 65, 257
and 300 - a wave edge and a block edge (AFX_BLOCK = 256) inside; repeated tags within a wave, across waves and across blocks, with
lane 255 - the last lane of the first block - the lowest index of two groups; 40 distinct tags that share one start slot,
interleaved with repeats; a chain from slot 126 over the wrap to slot 0; items skipped by status_in on both sides of a participating
repeat; second and third calls that replay parts of the first; lookups before and after; a fill to exactly the capacity.
Capacity 64 (128 slots) wherever the calls fit it: a call is refused unless size + count <= capacity, so the counts above 64 run on
the smallest set that takes them (capacity = count).

Where 300 items do not reach: 2304 items, nine workgroups - more than the device has XCDs, whose L2s are private, so lanes of one key
meet only in `owner` and `lowest` across dies - with one tag for all, with a key in every workgroup, with the lowest index of every
key skipped, with descending pairs, and with a 24-slot chain whose items lie in all nine; pairs of tags that differ in one word and
share a start slot.  Beside the cases: _dev rows at an address that is 16 mod 32 with status and answers at odd addresses (ts_load is
two 16-byte loads), and the bytes on both sides of the answers."""
import numpy as np
import pytest

from tests import tagset_model as M

pytestmark = pytest.mark.gpu


def rows(tags):
    return np.frombuffer(b"".join(tags), np.uint8).reshape(len(tags), 32)


@pytest.fixture(scope="module")
def ctx():
    import aeonflux_amd as afx
    import bench
    params, key, ip = bench.load_fixture("readme_4attrs_sSPe")
    c = afx.Context(params, None, ip, device=0)          # any context: the set needs no key
    yield c
    c.close()


def run_ops(ts, ops):
    out = []
    for op in ops:
        if op[0] == "spend":
            out.append(ts.spend(rows(op[1]), None if op[2] is None else np.array(op[2], np.uint8)).tolist())
        else:
            out.append(ts.contains(rows(op[1])).tolist())
    return out


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_set_answers_as_the_sequential_loop(ctx, name):
    from aeonflux_amd import batch
    capacity, ops = M.CASES[name]()
    want, tags = M.expected(ops)
    ts = batch.TagSet(ctx, capacity, M.SALT)
    try:
        assert ts.size() == (0, capacity)
        assert run_ops(ts, ops) == want
        assert ts.size() == (len(tags), capacity)
        everything = sorted(tags)
        assert ts.contains(rows(everything)).tolist() == [1] * len(everything)
    finally:
        ts.close()


def test_the_answers_do_not_depend_on_the_salt(ctx):
    from aeonflux_amd import batch
    for name in ("one start slot", "duplicates", "skipped"):
        capacity, ops = M.CASES[name]()
        want, tags = M.expected(ops)
        ts = batch.TagSet(ctx, capacity)                 # salt=None: getrandom
        try:
            assert run_ops(ts, ops) == want, name
            assert ts.size() == (len(tags), capacity)
        finally:
            ts.close()


def test_a_call_that_may_not_fit_is_refused_with_nothing_touched(ctx):
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    tags = [M.tag("full %d" % i) for i in range(66)]
    ts = batch.TagSet(ctx, 64, M.SALT)
    try:
        seen = np.full(65, 0xEE, np.uint8)
        with pytest.raises(afx.AfxError) as e:           # capacity + 1 in one call
            ts.spend(rows(tags[:65]), out=seen)
        assert e.value.rc == afx.E_FULL and str(e.value)
        assert seen.tolist() == [0xEE] * 65 and ts.size() == (0, 64)
        assert ts.contains(rows(tags[:65])).tolist() == [0] * 65
        assert ts.spend(rows(tags[:64])).tolist() == [0] * 64          # exactly the capacity
        assert ts.size() == (64, 64)
        for again in (tags[64:65], tags[:1]):                          # one more, new or not: the host cannot know before the call runs
            seen = np.full(1, 0xEE, np.uint8)
            with pytest.raises(afx.AfxError) as e:
                ts.spend(rows(again), out=seen)
            assert e.value.rc == afx.E_FULL
            assert seen.tolist() == [0xEE] and ts.size() == (64, 64)
        assert ts.contains(rows(tags)).tolist() == [1] * 64 + [0, 0]
        assert ts.spend(rows([]).reshape(0, 32)).tolist() == []        # an empty call is no call
    finally:
        ts.close()


def test_bad_arguments(ctx):
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    for capacity in (0, (1 << 30) + 1):
        with pytest.raises(afx.AfxError) as e:
            batch.TagSet(ctx, capacity, M.SALT)
        assert e.value.rc == afx.E_BAD_ARGS
    lib = afx.lib()
    assert lib.afx_tagset_size(None, None, None) == afx.E_BAD_ARGS
    assert lib.afx_tagset_spend(None, None, None, 1, None) == afx.E_BAD_ARGS
    ts = batch.TagSet(ctx, 64, M.SALT)
    try:
        assert lib.afx_tagset_spend(ts.h, None, None, 1, None) == afx.E_BAD_ARGS
        assert lib.afx_tagset_contains_dev(ts.h, 24, 1, 32) == afx.E_BAD_ARGS          # rows that are not 16-byte aligned: refused, not read
        assert lib.afx_tagset_spend_dev(ts.h, 24, None, 1, 32) == afx.E_BAD_ARGS
        assert ts.size() == (0, 64)
    finally:
        ts.close()


def test_the_dev_forms_on_both_pipelining_lanes_give_the_same_bytes(ctx):
    from aeonflux_amd import batch
    from tests.helpers import DevMem
    capacity, ops = M.CASES["replays"]()
    want, tags = M.expected(ops)
    for pipelining in (0, 1):
        ctx.set_pipelining(pipelining)
        ts = batch.TagSet(ctx, capacity, M.SALT)
        try:
            # every call queued before anything is read: with pipelining the calls alternate between the two lanes, and each must still run
            # behind the one before it
            outs = []
            for op in ops:
                n = len(op[1])
                d_T, d_seen = DevMem(rows(op[1])), DevMem(np.full(n, 0xEE, np.uint8))
                if op[0] == "spend":
                    ts.spend_dev(d_T, None, n, d_seen)
                else:
                    ts.contains_dev(d_T, n, d_seen)
                outs.append((d_T, d_seen))
            ctx.synchronize()
            assert [o[1].numpy().tolist() for o in outs] == want, pipelining
            assert ts.size() == (len(tags), capacity)
            # status rows on the device (size() above made the bound exact again: the three spends had counted 20 + 20 + 21 of the 64)
            skipped_cap, skipped_ops = M.CASES["skipped"]()
            first = skipped_ops[0]
            d_T, d_st, d_seen = DevMem(rows(first[1])), DevMem(np.array(first[2], np.uint8)), DevMem(np.full(len(first[1]), 0xEE, np.uint8))
            ts.spend_dev(d_T, d_st, len(first[1]), d_seen)
            ctx.synchronize()
            assert d_seen.numpy().tolist() == M.Model().spend(first[1], first[2])
        finally:
            ts.close()
            ctx.set_pipelining(0)


class DevAt:
    """`nbytes` of device memory that start `offset` bytes into an allocation with `after` more bytes behind them, all of it 0xEE first"""

    def __init__(self, offset, nbytes, after=0, array=None):
        from tests.helpers import DevMem
        self.mem = DevMem(nbytes=offset + nbytes + after, fill=0xEE)
        self.offset, self.n, self.ptr = offset, nbytes, self.mem.ptr + offset
        if array is not None:
            a = np.ascontiguousarray(array, dtype=np.uint8)
            assert a.nbytes == nbytes
            assert self.mem.hip().hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0

    def parts(self):
        whole = self.mem.numpy()
        return whole[:self.offset], whole[self.offset:self.offset + self.n], whole[self.offset + self.n:]


def dev_ops(ctx, ts, ops, t_off, b_off):
    """the ops through the _dev forms, every call queued before anything is read: rows t_off bytes and status / answers b_off bytes into
    their (256-byte aligned) allocations.  -> the answers, with the bytes around them checked"""
    bufs = []
    for op in ops:
        n = len(op[1])
        d_T, d_seen = DevAt(t_off, 32 * n, array=rows(op[1])), DevAt(b_off, n, after=3)
        if op[0] == "spend":
            d_st = None if op[2] is None else DevAt(b_off, n, array=np.array(op[2], np.uint8))
            ts.spend_dev(d_T.ptr, None if d_st is None else d_st.ptr, n, d_seen.ptr)
            bufs.append((d_T, d_st, d_seen))
        else:
            ts.contains_dev(d_T.ptr, n, d_seen.ptr)
            bufs.append((d_T, d_seen))
    ctx.synchronize()
    out = []
    for b in bufs:
        before, seen, after = b[-1].parts()
        assert before.tolist() == [0xEE] * b_off and after.tolist() == [0xEE] * 3
        out.append(seen.tolist())
    return out


@pytest.mark.parametrize("name", ["skipped", "duplicates"])
def test_rows_at_16_mod_32_and_bytes_at_odd_addresses_give_the_aligned_calls_answers(ctx, name):
    """ts_load reads a row as two 16-byte halves: a row needs 16-byte alignment and no more.  status_in and seen_out are bytes"""
    from aeonflux_amd import batch
    capacity, ops = M.CASES[name]()
    want, tags = M.expected(ops)
    got = {}
    for t_off, b_off in ((0, 0), (16, 1), (48, 3)):
        ts = batch.TagSet(ctx, capacity, M.SALT)
        try:
            got[t_off] = dev_ops(ctx, ts, ops, t_off, b_off)
            assert ts.size() == (len(tags), capacity)
        finally:
            ts.close()
    assert got[0] == want
    assert got[16] == got[0] and got[48] == got[0]


@pytest.mark.parametrize("count", [1, 65, 257])
def test_the_bytes_around_the_answers_are_untouched(ctx, count):
    from aeonflux_amd import batch
    tags = [M.tag("around %d" % (i % max(1, count - 2))) for i in range(count)]           # (with repeats at the end when there is room)
    status = [1 if i % 5 == 4 else 0 for i in range(count)]
    ts = batch.TagSet(ctx, max(64, 2 * count), M.SALT)
    try:
        m = M.Model()
        d_T, d_st = DevAt(0, 32 * count, array=rows(tags)), DevAt(0, count, array=np.array(status, np.uint8))
        seen = [DevAt(64, count, after=64) for _ in range(3)]
        ts.spend_dev(d_T.ptr, d_st.ptr, count, seen[0].ptr)
        ts.contains_dev(d_T.ptr, count, seen[1].ptr)
        ts.spend_dev(d_T.ptr, None, count, seen[2].ptr)
        ctx.synchronize()
        want = [m.spend(tags, status), m.contains(tags), m.spend(tags)]
        for s, w in zip(seen, want):
            before, got, after = s.parts()
            assert got.tolist() == w
            assert before.tolist() == [0xEE] * 64 and after.tolist() == [0xEE] * 64
        assert ts.size() == (len(m.tags), max(64, 2 * count))
    finally:
        ts.close()


def test_dev_calls_count_towards_the_bound_until_the_size_is_read(ctx):
    import aeonflux_amd as afx
    from aeonflux_amd import batch
    from tests.helpers import DevMem
    tags = [M.tag("bound %d" % i) for i in range(40)]
    ts = batch.TagSet(ctx, 64, M.SALT)
    try:
        d_T, d_seen = DevMem(rows(tags)), DevMem(np.full(40, 0xEE, np.uint8))
        ts.spend_dev(d_T, None, 40, d_seen)
        ts.spend_dev(d_T, None, 20, d_seen)              # a replay: the set still holds 40, the bound says 60
        with pytest.raises(afx.AfxError) as e:
            ts.spend_dev(d_T, None, 5, d_seen)
        assert e.value.rc == afx.E_FULL
        assert ts.size() == (40, 64)                     # ... and the bound is exact again
        ts.spend_dev(d_T, None, 24, d_seen)
        ctx.synchronize()
        assert d_seen.numpy()[:24].tolist() == [1] * 24 and ts.size() == (40, 64)
    finally:
        ts.close()
