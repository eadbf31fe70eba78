"""CPU-only: seeded mutation fuzzing of the user side on bytes - afx_issuance_wire_section_bytes, afx_verify_issuances_mixed_wire and
afx_show_wire - on the host simulation of the engine (fake HIP runtime, tests/hostsim/fake_hip.cpp + fake_wire_issue.cpp) built with
AddressSanitizer + UBSan.  Valid, mixed, n-mismatched and empty AFXI streams are damaged in every header word, truncated at every byte
and mutated at random; afx_show_wire gets size queries of every layout, full calls with permuted, damaged and missing positions and
short buffers.  Every call must answer AFX_OK or AFX_E_BAD_ARGS, and a refused call must leave its buffers untouched - never a
sanitizer report, never a crash.  The mutation loop is C++ (tests/hostsim/user_wire_fuzz.cpp)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
MUTATIONS = int(os.environ.get("AFX_FUZZ_MUTATIONS", "4000"))


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("userfuzz") / "user_wire_fuzz")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "wire_issue.cpp", "wire_user.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_wire_issue.cpp", "user_wire_fuzz.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def issuances(kinds, count, nr, rng):
    from aeonflux_amd import wire
    iss = {k: rng.integers(0, 256, size=(count, 32), dtype=np.uint8) for k in ("t", "U", "V", "challenge")}
    iss["responses"] = rng.integers(0, 256, size=(nr, count, 32), dtype=np.uint8)
    return wire.pack_issuances(list(kinds), rng.integers(0, 256, size=(len(kinds), count, 32), dtype=np.uint8), iss)


def test_user_side_wire_entry_points_survive_mutations(fuzzer, tmp_path):
    from tests.helpers import make_credentials
    d = make_credentials(4, "SSPE", 1, b"user-wire-fuzz")
    rng = np.random.default_rng(9)
    a = issuances([1, 0, 2, 4], 3, 9, rng)
    b = issuances([2, 2, 3, 3], 2, 9, rng)
    m = issuances([1, 1, 2], 2, 8, rng)
    z = issuances([1, 0, 2, 4], 0, 9, rng)
    files = {"params.bin": d["params"], "ip.bin": d["ip"], "a.afxi": a, "b.afxi": b, "m.afxi": m, "z.afxi": z, "mixed.afxi": a + b + m + z + a}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([fuzzer, str(tmp_path), str(MUTATIONS)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "user wire fuzz ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    words = r.stdout.split("user wire fuzz ok:")[1].split()
    assert int(words[0]) >= MUTATIONS and int(words[4]) >= MUTATIONS // 4, r.stdout
