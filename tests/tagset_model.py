"""The spent-tag set's model (include/aeonflux_gpu.h "The spent-tag set"): the slot function on hashlib, the sequential loop that
afx_tagset_spend is specified to equal, and tags aimed at slots - arbitrary 32-byte strings, no group arithmetic.  Shared by
tests/test_tagset_on_host.py (the lane bodies on the host), tests/test_hostsim_tagset.py (tagset.cpp on the fake runtime),
tests/test_gpu_tagset.py (the kernels) and tests/test_gpu_rate_limit.py (the loop alone, on keys of its own)."""
import hashlib

FRESH, SPENT, SKIPPED = 0, 1, 2
PREFIX = b"aeonflux-amd/tagset/v1"
assert len(PREFIX) == 22


def n_slots(capacity):
    n = 2
    while n < 2 * capacity:
        n *= 2
    return n


def slot(salt, tag, slots):
    assert len(salt) == 32 and len(tag) == 32
    return int.from_bytes(hashlib.shake_256(PREFIX + salt + tag).digest(8), "little") % slots


class Model:
    """the loop of the header, on a Python set"""

    def __init__(self):
        self.tags = set()

    def spend(self, tags, status=None):
        seen = []
        for i, t in enumerate(tags):
            if status is not None and status[i] != 0:
                seen.append(SKIPPED)
            elif t in self.tags:
                seen.append(SPENT)
            else:
                seen.append(FRESH)
                self.tags.add(t)
        return seen

    def contains(self, tags):
        return [1 if t in self.tags else 0 for t in tags]


def tag(label):
    return hashlib.shake_256(b"tests/tagset_model tag " + str(label).encode()).digest(32)


def tags_at(salt, slots, want_slot, how_many, label):
    """`how_many` distinct tags whose probe sequences all start at want_slot"""
    out, k = [], 0
    while len(out) < how_many:
        t = tag("%s/%d/%d" % (label, want_slot, k))
        k += 1
        if slot(salt, t, slots) == want_slot:
            out.append(t)
    return out


# ---- the cases both suites run: name -> (capacity, [op]), op = ("spend", tags, status or None) | ("contains", tags) ----------------
# Capacity 64 gives 128 slots.  A call is refused unless size + count <= capacity, so the counts above 64 run on a set that holds them
# (the smallest such: capacity = count).
SALT = hashlib.shake_256(b"tests/tagset_model salt").digest(32)
COUNTS = (1, 63, 64, 65, 257, 300)


def case_count(n):
    """n items, a third of them repeats of earlier ones at strides that cross wave (64) and block (256) edges"""
    distinct = max(1, (2 * n + 2) // 3)
    tags = [tag("count %d/%d" % (n, (i * 7) % distinct if i >= distinct else i)) for i in range(n)]
    probe = tags[:5] + [tag("count %d/absent %d" % (n, k)) for k in range(3)]
    return max(64, n), [("contains", probe), ("spend", tags, None), ("contains", probe)]


def case_duplicates():
    """pairs and triples within a wave, across waves and across blocks; in two groups the lowest index is lane 255, the LAST lane of the
    first block"""
    n = 300
    tags = [tag("dup %d" % i) for i in range(n)]
    groups = [(3, 17), (10, 100), (255, 256, 299), (5, 70, 260), (63, 64), (191, 192, 193), (0, 298), (254, 257)]
    for g in groups:
        for i in g[1:]:
            tags[i] = tags[g[0]]
    tags[258] = tags[255]
    return n, [("spend", tags, None), ("contains", tags[250:262])]


def case_one_start_slot():
    """40 distinct tags whose probe sequences start at one slot, interleaved with repeats of them: one chain of 40 slots"""
    chain = tags_at(SALT, 128, 37, 40, "chain")
    tags = []
    for k, t in enumerate(chain):
        tags.append(t)
        if k % 2 == 1:
            tags.append(chain[(k * 5) % (k + 1)])          # a repeat of a tag at or before k
    assert len(tags) == 60
    return 64, [("spend", tags, None), ("contains", chain + [tag("chain absent")]), ("spend", chain[::-1][:4], None)]


def case_wrap():
    """a chain that starts at slot 126 and wraps past 127 to 0, then tags that start inside the wrapped part"""
    chain = tags_at(SALT, 128, 126, 5, "wrap")
    inside = tags_at(SALT, 128, 127, 2, "wrap in") + tags_at(SALT, 128, 0, 2, "wrap in")
    first = [chain[0], chain[1], chain[0], chain[2], chain[3], chain[4], chain[2]]
    return 64, [("spend", first, None), ("contains", chain + inside), ("spend", inside + chain[3:] + inside[:1], None), ("contains", chain + inside)]


def case_skipped():
    """items skipped by status_in that repeat a participating tag, on both sides of it; a tag that is only ever skipped stays out"""
    a, b, c, d = (tag("skip %s" % x) for x in "abcd")
    tags = [a, a, a, b, c, b, b, d, a]
    status = [1, 0, 4, 0, 1, 5, 0, 0, 0]
    more = [tag("skip more %d" % i) for i in range(70)]                     # the same pattern across a wave edge
    tags2 = more[:62] + [more[63], more[63], more[63]] + more[64:]
    status2 = [0] * 62 + [1, 0, 1] + [0] * (len(tags2) - 65)
    return 128, [("spend", tags, status), ("contains", [a, b, c, d]), ("spend", [c, a], None), ("spend", tags2, status2), ("contains", more[60:66])]


def case_replays():
    """a second and a third call that replay parts of the first: comparisons with kept keys"""
    one = [tag("replay %d" % i) for i in range(20)]
    two = one[::2] + [tag("replay two %d" % i) for i in range(10)]
    three = two[5:15] + one[1::2] + [tag("replay three")]
    return 64, [("contains", one[:3]), ("spend", one, None), ("contains", one[:3] + two[-2:]), ("spend", two, None), ("spend", three, None), ("contains", one + two + three)]


def case_fill():
    """exactly `capacity` distinct tags in one call"""
    tags = [tag("fill %d" % i) for i in range(64)]
    return 64, [("spend", tags, None), ("contains", tags[::9] + [tag("fill absent")])]


def case_near_tags():
    """pairs of tags that differ in ONE of their eight 32-bit words and start at one slot: the only place where a comparison that skips
    a word shows - tags that differ anywhere nearly always start apart and are never compared.  The second of a pair meets the first as
    an item of its own call, and in the next calls as a kept key"""
    first, second = [], []
    for word in range(8):
        base = tag("near %d" % word)
        k = 0
        while True:
            other = base[:4 * word] + hashlib.shake_256(b"near other %d" % k).digest(4) + base[4 * word + 4:]
            k += 1
            if other != base and slot(SALT, other, 128) == slot(SALT, base, 128):
                break
        first += [base, other]
        second += [other[:4 * word] + bytes(b ^ 0x80 for b in other[4 * word:4 * word + 4]) + other[4 * word + 4:]]      # a third of the family, wherever it starts
    return 64, [("spend", first, None), ("contains", first + second), ("spend", first[1::2] + first[::2], None), ("spend", second, None)]


# Nine workgroups of AFX_BLOCK = 256 lanes: more than the MI355X has XCDs, so some of one key's items run on dies with private L2s and
# meet only in `owner` and `lowest`.  8192 slots, the table of capacity = count.
WIDE = 2304
WIDE_KINDS = ("one tag", "every block", "every block, lowest skipped", "descending pairs")


def case_wide(kind):
    """2304 items, then the whole call again (all spent, or skipped), then a lookup"""
    n = WIDE
    status = None
    if kind == "one tag":
        tags = [tag("wide one")] * n
    elif kind in ("every block", "every block, lowest skipped"):
        tags = [tag("wide %d" % (i % 257)) for i in range(n)]           # 257: each key has an item in every workgroup, at a lane that moves
        if kind.endswith("skipped"):
            status = [3 if i < 257 else 0 for i in range(n)]            # the lowest index of every key is out: the second lowest is fresh
    else:
        tags = [tag("wide pair %d" % ((n - 1 - i) // 2)) for i in range(n)]
    probe = tags[::97] + [tag("wide absent %d" % k) for k in range(3)]
    # the replay is refused unless size + count <= capacity: the smallest capacity that takes it, still 8192 slots
    capacity = n + len(set(tags))
    assert n_slots(capacity) == n_slots(n)
    return capacity, [("spend", tags, status), ("spend", tags, status), ("contains", probe)]


_wide_chain = []


def case_wide_chain():
    """24 tags whose probe sequences start at one slot, each once in every one of nine workgroups, among tags that go anywhere"""
    slots = n_slots(WIDE)
    if not _wide_chain:
        _wide_chain.extend(tags_at(SALT, slots, 4097, 24, "wide chain"))
    tags = [tag("wide filler %d" % i) for i in range(WIDE)]
    for w in range(WIDE // 256):
        for k, t in enumerate(_wide_chain):
            tags[256 * w + (10 * k + 7 * w) % 256] = t                   # (10 * k < 256: 24 lanes of the workgroup, other ones in each)
    return WIDE, [("spend", tags, None), ("contains", _wide_chain + [tag("wide chain absent")]), ("spend", _wide_chain[::-1], None)]


CASES = dict([("count %d" % n, (lambda n=n: case_count(n))) for n in COUNTS] +
             [("duplicates", case_duplicates), ("one start slot", case_one_start_slot), ("wrap", case_wrap), ("skipped", case_skipped),
              ("replays", case_replays), ("fill", case_fill), ("near tags", case_near_tags)] +
             [("wide: %s" % k, (lambda k=k: case_wide(k))) for k in WIDE_KINDS] + [("wide: one start slot", case_wide_chain)])


def scenario_text(capacity, salt, ops):
    """a case as the text the host programs read (tests/hostsim/tagset_host.cpp, tests/hostsim/tagset_doors.cpp)"""
    lines = ["set %d %s" % (capacity, salt.hex())]
    for op in ops:
        if op[0] == "spend":
            status = op[2] if op[2] is not None else [0] * len(op[1])
            lines.append("call %d" % len(op[1]))
            lines += ["%s %d" % (t.hex(), s) for t, s in zip(op[1], status)]
        else:
            lines.append("contains %d" % len(op[1]))
            lines += [t.hex() for t in op[1]]
    return "\n".join(lines) + "\n"


def expected(ops):
    """the model's answer to every op, in order, and the final set"""
    m, out = Model(), []
    for op in ops:
        out.append(m.spend(op[1], op[2]) if op[0] == "spend" else m.contains(op[1]))
    return out, m.tags
