"""CPU-only: seeded mutation fuzzing of the entry points that take CredentialRequest bytes (AFXR v1) - afx_request_wire_parse,
afx_request_wire_section_bytes, afx_issue_wire (size query and full call) - on the host simulation of the engine (fake HIP runtime,
tests/hostsim/fake_hip.cpp + fake_wire_issue.cpp) built with AddressSanitizer + UBSan.  Valid single-layout, n = 0 and mixed streams
from the Python packer are damaged in >= 10^5 ways (every edge value in every header word, truncations around every 32-byte boundary,
spliced and duplicated sections, random bit flips / truncations / field copies); every call must answer AFX_OK or AFX_E_BAD_ARGS -
never a sanitizer report, never a crash, never another code.  The mutation loop is C++ (tests/hostsim/request_wire_fuzz.cpp)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
MUTATIONS = int(os.environ.get("AFX_FUZZ_MUTATIONS", "110000"))


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reqfuzz") / "request_wire_fuzz")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "wire_issue.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_wire_issue.cpp", "request_wire_fuzz.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_request_parsers_and_issue_wire_survive_a_hundred_thousand_mutations(fuzzer, tmp_path):
    from aeonflux_amd import wire
    from tests.helpers import make_credentials
    d = make_credentials(4, "SSPE", 1, b"request-wire-fuzz")
    rng = np.random.default_rng(5)
    vals = lambda n, c: rng.integers(0, 256, size=(n, c, 32), dtype=np.uint8)
    a = wire.pack_requests([1, 0, 2, 3], vals(4, 3))
    b = wire.pack_requests([4, 4], vals(2, 2))
    z = wire.pack_requests([], np.zeros((0, 2, 32), np.uint8))
    files = {"params.bin": d["params"], "key.bin": d["key"], "ip.bin": d["ip"], "a.afxr": a, "b.afxr": b, "z.afxr": z,
             "mixed.afxr": a + b + wire.pack_requests([1, 0, 2, 3], vals(4, 1)) + z}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([fuzzer, str(tmp_path), str(MUTATIONS)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "request wire fuzz ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert int(r.stdout.split("request wire fuzz ok:")[1].split()[0]) >= min(MUTATIONS, 100000), r.stdout
