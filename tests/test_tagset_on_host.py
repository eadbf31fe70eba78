"""CPU-only: the lane bodies of the spent-tag set - aeonflux_amd/csrc/tagset.cuh tagset_slot, tagset_claim_item, tagset_resolve_item and
tagset_contains_item, the statements k_tagset_claim, k_tagset_resolve and k_tagset_contains run per lane - compiled for the host over
the header's atomics shim (tests/hostsim/tagset_host.cpp: a stand-alone program under ASan and UBSan, nothing preloaded) and run lane
by lane in ten lane orders (ascending, descending, eight seeded shuffles; claim and resolve shuffled apart), each one legal
interleaving at lane granularity:

    slot(T)      == u64le(SHAKE256("aeonflux-amd/tagset/v1" || salt || T)[0..8)) mod n_slots      by hashlib, on every tag of every case
    seen_out     identical across the orders (the program's own check) and equal to the sequential loop of the header
    the contents identical across the orders as a set, equal to the model's set; the size word is their number

on the cases of tests/tagset_model.py, which tests/test_gpu_tagset.py runs on the kernels.

Lane by lane, a lane that joins a slot always finds the claimer's minimum done.  So the same program is built a second time with
-DAFX_TAGSET_TEST_THREADS -fsanitize=thread: the header's atomics are then relaxed __atomic builtins, and the claim lanes of a call run
on 16 threads, are joined, and the resolve lanes run on 16 threads - 20 rounds a case, each from a fresh table, with the same checks
and ThreadSanitizer watching the lane bodies.

`tagset_host error-paths` (the first build) runs the lane bodies on tables no finished call leaves: a stale owner on a probe path, and
a table without an empty slot."""
import os
import subprocess

import pytest

from tests import tagset_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(out, flags):
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + flags + ["-I" + os.path.join(ROOT, "tests", "hostsim", "include"), "-o", out, os.path.join(ROOT, "tests", "hostsim", "tagset_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("tagset") / "tagset_host"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def threaded_program(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("tagset_threads") / "tagset_host"), ["-fsanitize=thread", "-DAFX_TAGSET_TEST_THREADS", "-pthread"])


def run(program, tmp_path, capacity, salt, ops):
    path = tmp_path / "scenario.txt"
    path.write_text(M.scenario_text(capacity, salt, ops))
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
    slots, answers, keys, size = [], [], set(), None
    for line in r.stdout.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "slot":
            slots.append((bytes.fromhex(w[1]), int(w[2])))
        elif w[0] in ("seen", "has"):
            answers.append([int(ch) for ch in (w[1] if len(w) > 1 else "")])
        elif w[0] == "key":
            keys.add(bytes.fromhex(w[1]))
        elif w[0] == "size":
            size = int(w[1])
    return slots, answers, keys, size


@pytest.mark.parametrize("name", list(M.CASES))
def test_every_lane_order_gives_the_sequential_loops_answers(program, tmp_path, name):
    capacity, ops = M.CASES[name]()
    slots, answers, keys, size = run(program, tmp_path, capacity, M.SALT, ops)
    want, tags = M.expected(ops)
    assert answers == want
    assert keys == tags and size == len(tags)
    n = M.n_slots(capacity)
    assert len(slots) == sum(len(op[1]) for op in ops if op[0] == "spend")
    for t, s in slots:
        assert s == M.slot(M.SALT, t, n), t.hex()


THREADED = ["duplicates", "one start slot", "wrap", "skipped", "near tags"] + [name for name in M.CASES if name.startswith("wide: ")]


@pytest.mark.parametrize("name", THREADED)
def test_lanes_on_threads_give_the_sequential_loops_answers_every_round(threaded_program, tmp_path, name):
    """(the program compares its 20 rounds with each other; round 0 is compared with the model here)"""
    capacity, ops = M.CASES[name]()
    slots, answers, keys, size = run(threaded_program, tmp_path, capacity, M.SALT, ops)
    want, tags = M.expected(ops)
    assert answers == want
    assert keys == tags and size == len(tags)


def test_the_lane_bodies_on_a_stale_owner_and_on_a_table_without_an_empty_slot(program):
    r = subprocess.run([program, "error-paths"], capture_output=True, text=True)
    assert r.returncode == 0 and "error paths ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])


def test_the_slot_function_is_the_headers_on_edge_bytes(program, tmp_path):
    # all-zero and all-ones salts and tags, single set bits at the byte positions where the 86-byte message crosses the sponge's lanes
    tags = [bytes(32), b"\xff" * 32] + [bytes([0] * k + [0x80] + [0] * (31 - k)) for k in (0, 1, 2, 7, 8, 9, 15, 16, 23, 24, 30, 31)] + [bytes(range(32))]
    for salt in (bytes(32), b"\xff" * 32, bytes(range(100, 132)), b"\x00" * 31 + b"\x01", b"\x01" + b"\x00" * 31):
        for capacity in (len(tags), 64, 1 << 15):
            slots, answers, keys, size = run(program, tmp_path, capacity, salt, [("spend", tags, None)])
            n = M.n_slots(capacity)
            assert [s for _, s in slots] == [M.slot(salt, t, n) for t in tags], (salt.hex(), capacity)
            assert answers == [[0] * len(tags)] and keys == set(tags) and size == len(tags)


def test_the_aimed_tags_really_share_their_chains():
    # (the cases rest on it: 40 tags at slot 37, a chain from slot 126 over the wrap)
    assert M.n_slots(64) == 128 and M.n_slots(65) == 256 and M.n_slots(1) == 2 and M.n_slots(300) == 1024
    _, ops = M.case_one_start_slot()
    assert {M.slot(M.SALT, t, 128) for t in ops[0][1]} == {37} and len(set(ops[0][1])) == 40
    _, ops = M.case_wrap()
    assert {M.slot(M.SALT, t, 128) for t in ops[0][1]} == {126} and len(set(ops[0][1])) == 5
    capacity, ops = M.case_wide_chain()
    chain = ops[1][1][:-1]
    assert M.n_slots(capacity) == 8192 and len(set(chain)) == 24 and {M.slot(M.SALT, t, 8192) for t in chain} == {4097}
    for w in range(9):                                                         # each of them once in every workgroup
        assert sorted(t for t in ops[0][1][256 * w:256 * w + 256] if t in chain) == sorted(chain)
