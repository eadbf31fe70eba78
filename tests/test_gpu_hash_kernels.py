"""GPU: each of the three transcript kernels against the ORACLE's merlin, bit for bit (kernels.hip k_hash, k_hash_coop, k_hash_coop64).

A hash launch takes one of three kernels by its size (engine.cpp, kernels.hip afxk_hash_coop): a wave per (item, program) up to 2048
of them, 32 lanes each up to AFX_HASH_COOP_GROUPS = 4096 while the pass is small (afx_ctx_set_small_batch_items), one lane per item
beyond.  The statements' own tests reach all three, but only with the byte layouts the statements have.  Here scripted transcripts
(afx_merlin_challenges) put a per-item 32-byte hole at every position of the 166-byte rate, take challenges of every length class in
mid-script and run item counts on both sides of every launch rule - and every test asserts WHICH kernel it ran from the launch
counts (afx_ctx_get_timing "k_hash_coop64", "k_hash_coop"; "k_hash" is the three together).  Every expected byte is
oracle.merlin_script's; nothing is compared with another GPU run."""
import hashlib

import numpy as np
import pytest

from tests import hash_sweep as hs

pytestmark = pytest.mark.gpu

KERNELS = ("k_hash_coop64", "k_hash_coop", "k_hash")
SWEEP_ITEMS = {"k_hash_coop64": 5,    # four waves a block: a ragged second block
               "k_hash_coop": 9,      # 32 lanes an item, odd: a dead lane group shadows the last item
               "k_hash": 70}          # a lane an item: a ragged second wave


@pytest.fixture(scope="module")
def engine():
    import oracle
    import aeonflux_amd as afx
    st = hashlib.shake_256(b"gpu-hash-kernels").digest(1 << 15)
    params, used = oracle.system_parameters_generate(4, st)
    key, ip = oracle.issuer_new(params, st[used:used + 64 * 8])
    ctx = afx.Context(params, key, ip)
    yield afx, ctx
    ctx.close()


def select(afx, ctx, kernel):
    """the settings under which a launch of at most 2048 (item, program) pairs takes `kernel`"""
    ctx.set_plan_variants(afx.VARIANT_HASH_HALF_WAVE if kernel == "k_hash_coop" else 0)
    ctx.set_small_batch_items(0 if kernel == "k_hash" else 4096)


def reset(afx, ctx):
    ctx.set_timing(False)
    ctx.set_plan_variants(afx.DEFAULT_PLAN_VARIANTS)
    ctx.set_small_batch_items(4096)


def launches(ctx):
    """{kernel: launches since set_timing(True)}; "k_hash" reports the three kernels together, so the one-lane kernel's own count is the rest"""
    n = {k: ctx.get_timing(k)[1] for k in KERNELS}
    n["k_hash"] -= n["k_hash_coop64"] + n["k_hash_coop"]
    return n


def only(kernel, n):
    return {k: (n if k == kernel else 0) for k in KERNELS}


def as_arrays(fields, count):
    return [np.frombuffer(f, np.uint8).reshape(count, 32) for f in fields]


def item_fields(fields, i):
    return [f[32 * i:32 * i + 32] for f in fields]


@pytest.fixture(scope="module")
def complex_want(kat):
    import oracle
    from tests.test_oracle_primitives import merlin_complex_ops
    v = kat["merlin_equivalence_complex"]
    return oracle.merlin_script(v["label"].encode(), merlin_complex_ops(v))


@pytest.mark.parametrize("kernel", KERNELS)
def test_merlins_conformance_vectors_through_each_kernel(engine, kat, complex_want, kernel):
    """merlin's two published vectors (tests/golden/kat.json), with the round structure of
    test_gpu_primitives.py::test_merlins_conformance_vectors_on_the_gpu: equivalence_complex chains 32 challenges, one program per
    challenge, the earlier ones fed back as fields; the last program absorbs 34 KB"""
    afx, ctx = engine
    select(afx, ctx, kernel)
    ctx.set_timing(True)
    try:
        count = 3
        s = kat["merlin_equivalence_simple"]
        out = ctx.merlin_challenges(s["label"].encode(), [("append", s["append_label"].encode(), s["append_data"].encode()), ("challenge", s["challenge_label"].encode(), 32)], [], count)
        assert [bytes(out[i, :32]).hex() for i in range(count)] == [s["challenge32"]] * count
        v = kat["merlin_equivalence_complex"]
        big = bytes([v["big_byte"]]) * v["big_len"]
        chals = []
        for r in range(v["rounds"]):
            ops = [("append", v["first_label"].encode(), v["first_data"].encode())]
            for k in range(r):
                ops += [("challenge", v["challenge_label"].encode(), 32), ("append", v["big_label"].encode(), big), ("append_field", v["feedback_label"].encode(), k)]
            ops.append(("challenge", v["challenge_label"].encode(), 32))
            out = ctx.merlin_challenges(v["label"].encode(), ops, [np.tile(np.frombuffer(c, np.uint8), (count, 1)) for c in chals], count)
            assert [bytes(out[i, :32]) for i in range(count)] == [complex_want[r]] * count, r
            chals.append(complex_want[r])
        assert chals[-1].hex() == v["last_challenge32"]
        assert launches(ctx) == only(kernel, 1 + v["rounds"])
    finally:
        reset(afx, ctx)


def test_the_sweep_reaches_every_hole_position():
    """the coverage the hole-offset sweep is there for, from the restated position arithmetic (tests/hash_sweep.py) - a later change of
    the script cannot shrink it unnoticed.  (No GPU needed, but it belongs to the test below.)"""
    c = hs.coverage()
    assert c["starts"] == set(range(hs.R))            # holes beginning at rate bytes 160 .. 165 among them
    assert c["qrs"] == hs.ALL_QR                      # afx_hash_word.q = -1 .. 3 with every r = 0 .. 7 it can carry
    assert c["cut"] == set(range(1, 32)) and c["word20"] >= 6        # cut by the boundary after 1 .. 31 bytes; in the 6-byte word 20


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_hole_at_every_offset_of_the_rate(engine, kernel):
    """a 32-byte per-item hole starting at every byte of the 166-byte rate - inside a word, across words, cut by the rate boundary, in
    the 6-byte last word - then a second hole 8 bytes behind it and the first once more: every item's 64 bytes against the oracle"""
    import oracle
    afx, ctx = engine
    count = SWEEP_ITEMS[kernel]
    fields = hs.fields_for(kernel.encode(), count)
    arrays = as_arrays(fields, count)
    select(afx, ctx, kernel)
    ctx.set_timing(True)
    try:
        bad = []
        for k in hs.K_RANGE:
            ops = hs.sweep_ops(k)
            out = ctx.merlin_challenges(hs.SWEEP_LABEL, ops, arrays, count)
            for i in range(count):
                want = oracle.merlin_script(hs.SWEEP_LABEL, ops, item_fields(fields, i))[0]
                if bytes(out[i]) != want:
                    bad.append((k, i))
        assert not bad, ("(pad length, item) pairs that differ from the oracle", bad[:20], len(bad))
        assert launches(ctx) == only(kernel, len(hs.K_RANGE))
    finally:
        reset(afx, ctx)


@pytest.mark.parametrize("kernel", KERNELS)
def test_challenges_of_every_length_in_mid_script(engine, kernel):
    """a challenge that is not the script's last zeroes the n bytes it squeezed and goes on behind them (StrobeSim::challenge_discard:
    a partial keep mask in word n / 8); the engine returns the last challenge only, and that one is compared"""
    import oracle
    afx, ctx = engine
    count = SWEEP_ITEMS[kernel]
    fields = hs.fields_for(b"mid:" + kernel.encode(), count)
    arrays = as_arrays(fields, count)
    lengths = (1, 7, 8, 9, 31, 32, 33, 63, 64)
    select(afx, ctx, kernel)
    ctx.set_timing(True)
    try:
        for n in lengths:
            ops = [("append_field", b"first", 0), ("challenge", b"mid", n), ("append_field", b"second", 1), ("challenge", b"last", 32)]
            out = ctx.merlin_challenges(b"mid-script challenges", ops, arrays, count)
            for i in range(count):
                want = oracle.merlin_script(b"mid-script challenges", ops, item_fields(fields, i))
                assert len(want[0]) == n and bytes(out[i, :32]) == want[1], (n, i)
        assert launches(ctx) == only(kernel, len(lengths))
    finally:
        reset(afx, ctx)


EDGE_OPS = [("append_field", b"a", 0), ("append", b"between", hs.PATTERN[:200]), ("append_field", b"b", 1), ("challenge", b"c", 64)]   # three rate blocks
EDGE_MAX = 4097
# (settings, count, the kernel the launch rule gives)
EDGE_CASES = [("default", c, "k_hash_coop64") for c in (1, 2, 3, 4, 5, 2048)] + [("default", 2049, "k_hash_coop"), ("default", 4096, "k_hash_coop"), ("default", 4097, "k_hash")] + \
             [("half-wave", c, "k_hash_coop") for c in (1, 2, 3, 4, 5, 8, 9)]


@pytest.fixture(scope="module")
def edge_fields():
    return hs.fields_for(b"edges", EDGE_MAX)


@pytest.mark.parametrize("settings,count,kernel", EDGE_CASES, ids=["%s-%d" % (s, c) for s, c, k in EDGE_CASES])
def test_item_counts_at_the_edges_of_the_launch_rule(engine, edge_fields, settings, count, kernel):
    """block sizes switch at 1, 2 and 4 items, last blocks are ragged, k_hash_coop's dead lane group shadows the last item of an odd
    count, the kernels switch behind 2048 and behind 4096 items: the first, the last and some 16 items between against the oracle, and
    the caller's rows behind `count` stay as they were"""
    import oracle
    afx, ctx = engine
    arrays = [a[:count] for a in as_arrays(edge_fields, EDGE_MAX)]
    ctx.set_plan_variants(afx.VARIANT_HASH_HALF_WAVE if settings == "half-wave" else 0)
    ctx.set_small_batch_items(4096)
    ctx.set_timing(True)
    try:
        out = np.full((count + 2, 64), 0xA5, np.uint8)
        assert ctx.merlin_challenges(b"edges", EDGE_OPS, arrays, count, out=out) is out
        assert launches(ctx) == only(kernel, 1)
        assert (out[count:] == 0xA5).all()
        for i in sorted(set(range(count)) if count <= 18 else {j * (count - 1) // 17 for j in range(18)}):
            want = oracle.merlin_script(b"edges", EDGE_OPS, [bytes(edge_fields[f][32 * i:32 * i + 32]) for f in range(2)])[0]
            assert bytes(out[i]) == want, i
    finally:
        reset(afx, ctx)
