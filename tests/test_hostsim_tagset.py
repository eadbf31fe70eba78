"""CPU-only: the host half of the spent-tag set (aeonflux_amd/csrc/tagset.cpp) on the fake HIP runtime under ASan/UBSan, built with its
own source list as tests/test_hostsim_tagged.py builds its program: the engine's host sources plus tagset.cpp, tests/hostsim/fake_hip.cpp,
the stand-in launchers tests/hostsim/fake_tagset.cpp and the driver tests/hostsim/tagset_doors.cpp - a program of its own, so the
sanitizers' runtimes are linked in and nothing is preloaded.  The stand-ins run the real lane bodies of tagset.cuh's host branch in a
shuffled order, so the driver compares whole calls with a std::set loop:

  * the model cases `count 65`, `duplicates`, `skipped`, `replays`, `fill` and `near tags` through afx_tagset_spend, _contains, _spend_dev and
    _contains_dev under both pipelining settings - and the answers it prints are compared with tests/tagset_model.py here;
  * the bound: _dev calls count until afx_tagset_size, AFX_E_FULL leaves seen_out and the set untouched, skipped items count;
  * argument errors, count 0, capacities 0 and 2^30 + 1, counts above 2^32 - 3, misaligned _dev rows;
  * a launcher that fails and a table whose error word is set: the call fails with seen_out untouched and EVERY later call on the set
    returns the first error - a state no GPU test can reach without provoking a fault;
  * calls that outgrow a lane's scratch buffer (T | slot_of | status_in | seen_out), on one lane and on alternating lanes;
  * destroy of NULL and after a failure.

This file only makes an issuer's parameters (the oracle's) and writes the cases out as scenario text."""
import os
import subprocess

import pytest

from tests import tagset_model as M
from tests.helpers import make_credentials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
CASES = ("count 65", "duplicates", "skipped", "replays", "fill", "near tags")


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_tagset") / "tagset_doors")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "tagset.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_tagset.cpp", "tagset_doors.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_tagset_doors_model_cases_bound_arguments_and_the_broken_state(doors, tmp_path):
    d = make_credentials(4, "SSSS", 1, b"hostsim-tagset")
    for name in ("params", "ip"):
        (tmp_path / (name + ".bin")).write_bytes(bytes(d[name]))
    paths, want = [], []
    for k, name in enumerate(CASES):
        capacity, ops = M.CASES[name]()
        path = tmp_path / ("scenario%d.txt" % k)
        path.write_text(M.scenario_text(capacity, M.SALT, ops))
        paths.append(str(path))
        want.append(M.expected(ops)[0])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([doors, str(tmp_path)] + paths, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "tagset doors ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-1500:], r.stderr[-5000:])
    got = []
    for line in r.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "scenario":
            got.append([])
        elif w and w[0] in ("seen", "has"):
            got[-1].append([int(ch) for ch in (w[1] if len(w) > 1 else "")])
    assert got == want
