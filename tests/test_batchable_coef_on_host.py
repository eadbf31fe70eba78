"""CPU-only: one coefficient of the batchable verification's weighted sum - aeonflux_amd/csrc/batchable.cuh coef_item and coef_mac, the
statements k_coef runs per lane - compiled for the host (tests/hostsim/coef_host.cpp) and compared with Python integers:

    out = (sum over the positive triples of rho_t * x_t  -  sum over the negative triples of rho_t * x_t) mod l,

rho_t the 128-bit weight the triple names, x_t the 256-bit operand it names (1 for AFX_COEF_ONE).  The operands need not be canonical:
the kernel never reduces them before it multiplies.  A product is below 2^384, a sum of at most 2^16 of them below 2^400, and the two
13-limb accumulators (416 bits) hold such a sum EXACTLY, so the reference for a non-canonical operand is the same integer expression.

Every buffer is laid out as the engine lays it out: weights[w][stride][16] with a pointer already moved to the pass's first item,
operand arrays of [count][32] at addresses that are 4-byte but not 16-byte aligned (all sc_load promises), and unrelated bytes in
every slot the job must not read."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import edge_values as EV
from tests.batchable_ref import LARGEST_COEF_JOB_16_STRICT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = EV.L
ONE = 0xffff            # plan.h AFX_COEF_ONE
MOST_TRIPLES = 65534    # BatchableSum refuses AFX_COEF_ONE weights or more in one sum: no job is longer

WEIGHTS = [0, 1, 2 ** 64 - 1, 2 ** 64, 2 ** 127, 2 ** 128 - 1]
W_ZERO, W_ONE, W_MAX = 0, 1, 5
OPERANDS = {"0": 0, "1": 1, "l-1": L - 1, "l": L, "2^252": 2 ** 252, "2^255": 2 ** 255, "2^256-1": 2 ** 256 - 1}
OPERANDS.update(("edge " + k, v) for k, v in EV.all_scalars().items())
OPERANDS.update(("non-canonical " + k, v) for k, v in EV.NON_CANONICAL.items())
OP_NAMES = list(OPERANDS)
OP_MAX = OP_NAMES.index("2^256-1")
N_TRIPLES = [1, 2, 27, LARGEST_COEF_JOB_16_STRICT, MOST_TRIPLES]
PATTERNS = ("positive", "negative", "equal", "one-short", "mixed")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("coef") / "libcoef_host.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out,
           os.path.join(ROOT, "tests", "hostsim", "coef_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    h = C.CDLL(out)
    h.coef_host_item.restype = None
    h.coef_host_item.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return h


class Table:
    """the arrays of one pass as a job sees them.  W[w][i] and X[o][i] are the values of item i < count; the weights of the whole call
    have `stride` items per row, the pass starts at item `off` of it, and the pointer a job gets is moved there (statements.cpp:
    bi->weights + off * AFX_WEIGHT_BYTES with stride `total`).  Every other byte is noise from `rnd`."""

    def __init__(self, lib, W, X, count=1, stride=None, off=0, rnd=None):
        rnd = rnd or random.Random(1)
        self.lib, self.W, self.X, self.count = lib, W, X, count
        self.stride = stride = count if stride is None else stride
        assert off + count <= stride and all(len(r) == count for r in W) and all(len(r) == count for r in X)
        img = bytearray(rnd.randbytes(16 * len(W) * stride))
        for w, row in enumerate(W):
            for i, v in enumerate(row):
                img[16 * (w * stride + off + i):16 * (w * stride + off + i) + 16] = v.to_bytes(16, "little")
        self._wbuf = C.create_string_buffer(len(img) + 16)
        base = -C.addressof(self._wbuf) % 16
        C.memmove(C.addressof(self._wbuf) + base, bytes(img), len(img))
        self.weights = C.addressof(self._wbuf) + base + 16 * off
        assert self.weights % 16 == 0
        # operand arrays: 4 bytes past a 16-byte boundary, noise between them
        span = (32 * count + 31) // 16 * 16 + 16
        self._obuf = C.create_string_buffer(span * len(X) + 32)
        self._obuf.raw = rnd.randbytes(span * len(X) + 32)
        first = C.addressof(self._obuf) + (-C.addressof(self._obuf) % 16) + 4
        self._ptrs = (C.c_void_p * max(1, len(X)))()
        for o, row in enumerate(X):
            self._ptrs[o] = first + span * o
            assert self._ptrs[o] % 16 == 4
            C.memmove(self._ptrs[o], b"".join(v.to_bytes(32, "little") for v in row), 32 * count)

    def got(self, triples, item=0):
        t = np.array([(w, o, neg, 0) for w, o, neg in triples], np.uint16)
        out = C.create_string_buffer(32)
        self.lib.coef_host_item(out, self.weights, self.stride, t.ctypes.data, len(triples), C.addressof(self._ptrs), item)
        return int.from_bytes(out.raw, "little")

    def want(self, triples, item=0):
        pos = sum(self.W[w][item] * (1 if o == ONE else self.X[o][item]) for w, o, neg in triples if not neg)
        neg = sum(self.W[w][item] * (1 if o == ONE else self.X[o][item]) for w, o, neg in triples if neg)
        assert pos < 2 ** 400 and neg < 2 ** 400          # what 13 limbs hold with room to spare
        return (pos - neg) % L

    def check(self, triples, item=0, what=None):
        g = self.got(triples, item)
        assert g < L, (what, hex(g))
        assert g == self.want(triples, item), (what, item, triples[:6], hex(g))
        return g


def pattern(name, combos, rnd):
    """the triples of a job over the given (weight index, operand index) list, one per combo: len(combos) of them"""
    n = len(combos)
    if name == "positive":          # no negative triple: the subtrahend is 0 and the kernel adds l - 0
        return [(w, o, 0) for w, o in combos]
    if name == "negative":
        return [(w, o, 1) for w, o in combos]
    if name == "mixed":
        return [(w, o, rnd.randrange(2)) for w, o in combos]
    assert n >= 2
    if name == "equal":             # every product once on each side (an odd one out gets the weight 0): 0, and not l
        t = [x for w, o in combos[:n // 2] for x in ((w, o, 0), (w, o, 1))]
        return t + [(W_ZERO, combos[-1][1], 0)] * (n % 2)
    if name == "one-short":         # the same, and 1 * 1 more on the negative side: l - 1
        k = (n - 1) // 2
        t = [x for w, o in combos[:k] for x in ((w, o, 0), (w, o, 1))] + [(W_ONE, ONE, 1)]
        return t + [(W_ZERO, combos[-1][1], 0)] * (n - len(t))
    raise ValueError(name)


def test_the_cross_product_of_edge_weights_operands_and_job_shapes(lib):
    """every (weight, operand) pair of the edge lists - the operand 1 of AFX_COEF_ONE included - in jobs of 1, 2, 27 triples, of the
    largest job the 16-attribute layout's strict statement makes (LARGEST_COEF_JOB_16_STRICT, pinned to the plan by
    tests/test_hostsim_batchable.py) and of 65534 triples, in each sign pattern; item 3 of a pass of 5 that starts at item 4 of a call
    of 11: the weight of (w, item) lies at ((w * 11) + 4 + 3) * 16 of the call's array"""
    rnd = random.Random(20261017)
    count, item = 5, 3
    noise = lambda bits: [rnd.getrandbits(bits) for _ in range(count)]
    W = [noise(128)[:item] + [v] + noise(128)[item + 1:] for v in WEIGHTS]
    X = [noise(256)[:item] + [OPERANDS[k]] + noise(256)[item + 1:] for k in OP_NAMES]
    tab = Table(lib, W, X, count=count, stride=11, off=4, rnd=rnd)
    combos = [(w, o) for w in range(len(WEIGHTS)) for o in list(range(len(OP_NAMES))) + [ONE]]
    jobs = 0
    for n in N_TRIPLES:
        for name in PATTERNS:
            if n == 1 and name in ("equal", "one-short"):
                continue
            # consecutive stretches of the pair list until every pair has been in a job of this shape (the longest job wraps around)
            for start in range(0, len(combos), min(n, len(combos))):
                job = pattern(name, [combos[(start + k) % len(combos)] for k in range(n)], rnd)
                assert len(job) == n
                g = tab.check(job, item, (n, name, start))
                if name == "equal":
                    assert g == 0
                if name == "one-short":
                    assert g == L - 1
                jobs += 1
    assert jobs > 1500


def test_the_longest_job_at_the_largest_values_reaches_the_thirteenth_limb(lib):
    """65534 triples of (2^128 - 1) * (2^256 - 1) on one side: the sum passes 2^384, so limb 12 of the accumulator is not zero - the
    case a carry loop that stops at limb 11 gets wrong"""
    tab = Table(lib, [[v] for v in WEIGHTS], [[OPERANDS[k]] for k in OP_NAMES])
    total = MOST_TRIPLES * WEIGHTS[W_MAX] * OPERANDS["2^256-1"]
    assert total >> 384 and total < 2 ** 400
    for neg in (0, 1):
        g = tab.check([(W_MAX, OP_MAX, neg)] * MOST_TRIPLES, 0, ("longest", neg))
        assert g == ((-1) ** neg * total) % L
    both = [(W_MAX, OP_MAX, 0)] * (MOST_TRIPLES // 2) + [(W_MAX, OP_MAX, 1)] * (MOST_TRIPLES // 2)
    assert tab.check(both, 0, "longest, both sides") == 0


def test_every_item_reads_its_own_weights_and_operands(lib):
    """distinct values in every (weight, item) and (operand, item) slot, passes at several offsets of calls longer than the pass"""
    rnd = random.Random(7)
    for count, stride, off in ((1, 1, 0), (5, 5, 0), (5, 9, 4), (64, 300, 236), (7, 1000, 256)):
        W = [[rnd.getrandbits(128) for _ in range(count)] for _ in range(9)]
        X = [[rnd.getrandbits(256) for _ in range(count)] for _ in range(4)]
        tab = Table(lib, W, X, count=count, stride=stride, off=off, rnd=rnd)
        job = [(w, (w * 3 + 1) % 5 if (w * 3 + 1) % 5 < 4 else ONE, w & 1) for w in range(9)]
        got = [tab.check(job, i, (count, stride, off)) for i in range(count)]
        assert len(set(got)) == count


def test_seeded_random_jobs(lib):
    rnd = random.Random(20261018)
    for k in range(2000):
        count = rnd.randrange(1, 6)
        stride = count + rnd.randrange(0, 5)
        off = rnd.randrange(0, stride - count + 1)
        bits = lambda top: rnd.choice((top, top, rnd.randrange(1, top + 1)))
        W = [[rnd.choice(WEIGHTS) if rnd.random() < 0.15 else rnd.getrandbits(bits(128)) for _ in range(count)] for _ in range(rnd.randrange(1, 13))]
        X = [[OPERANDS[rnd.choice(OP_NAMES)] if rnd.random() < 0.15 else rnd.getrandbits(bits(256)) for _ in range(count)] for _ in range(rnd.randrange(1, 9))]
        tab = Table(lib, W, X, count=count, stride=stride, off=off, rnd=rnd)
        job = [(rnd.randrange(len(W)), ONE if rnd.random() < 0.2 else rnd.randrange(len(X)), rnd.randrange(2)) for _ in range(rnd.randrange(1, 41))]
        tab.check(job, rnd.randrange(count), k)
