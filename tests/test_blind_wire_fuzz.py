"""CPU-only: seeded mutation fuzzing of the host-only entry points that take blind request bytes (AFXQ v1) and blind issuance bytes
(AFXJ v1) - the two parsers and the two section walkers - on the host build of the engine (fake HIP runtime) under AddressSanitizer +
UBSan, like tests/test_request_wire_fuzz.py and with as many mutated streams.  Valid sections of two layouts, of n = 0 and a stream of
both formats from the Python packers are damaged (every edge value in every header word, truncations around every 32-byte boundary,
spliced and duplicated sections, random bit flips / truncations / field copies / swapped magics); every call must answer AFX_OK or
AFX_E_BAD_ARGS - never a sanitizer report, never a crash - and every section a parser accepts must re-pack to itself.  The mutation loop
is C++ (tests/hostsim/blind_wire_fuzz.cpp)."""
import os
import subprocess

import pytest

from tests.test_blind_wire import random_issuance, random_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
MUTATIONS = int(os.environ.get("AFX_FUZZ_MUTATIONS", "110000"))


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("blindfuzz") / "blind_wire_fuzz")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "statements_blind.cpp", "wire_blind.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_blind.cpp", "fake_wire_issue.cpp", "blind_wire_fuzz.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_blind_wire_parsers_survive_a_hundred_thousand_mutations(fuzzer, tmp_path):
    from aeonflux_amd import wire
    a, b = (4, 2, 3, 1), (0, 1, 4)
    q_a = wire.pack_blind_requests(a, *random_request(a, 3, 1))
    q_b = wire.pack_blind_requests(b, *random_request(b, 2, 2))
    q_z = wire.pack_blind_requests((), *random_request((), 2, 3))
    j_a = wire.pack_blind_issuances(a, random_issuance(10, 3, 4))
    j_b = wire.pack_blind_issuances(b, random_issuance(10, 2, 5))          # (a context of n = 4 answered a request of n = 3)
    files = {"q_a.bin": q_a, "q_b.bin": q_b, "q_z.bin": q_z, "j_a.bin": j_a, "j_b.bin": j_b, "mixed.bin": q_a + j_a + q_z + q_b + j_b}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([fuzzer, str(tmp_path), str(MUTATIONS)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "blind wire fuzz ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert int(r.stdout.split("blind wire fuzz ok:")[1].split()[0]) >= min(MUTATIONS, 100000), r.stdout
