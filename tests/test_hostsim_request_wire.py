"""CPU-only: the doors of issuance on bytes (aeonflux_amd/csrc/wire_issue.cpp: afx_issue_wire, afx_issue_wire_rng, afx_group_issue_wire,
afx_group_issue_wire_rng) and the verification of the AFXI streams they write (wire_user.cpp: afx_verify_issuances_mixed_wire and its
group form) on the engine's host half, built against the fake HIP runtime under ASan/UBSan with its own source list: the engine's host
sources plus wire_issue.cpp, wire_user.cpp, tests/hostsim/fake_hip.cpp, the stand-ins for the record-writing and the draw launchers
(fake_wire_issue.cpp, fake_draw.cpp) and the driver, tests/hostsim/request_wire_doors.cpp - a program of its own, so the sanitizers'
runtimes are linked in and nothing is preloaded.  AFX_PLAN_SELFCHECK for the whole run: every plan is assembled twice and must relocate
to the same bytes, a reused one must equal a fresh one.  The stream has five sections (two batches for the device, one gathered over
two sections, a MacCreation section and an empty one); the driver checks sizes, headers, what an argument error leaves untouched,
that the size query draws nothing, which request's values and status land where, and that a group of two members - one member taking
the call, or every batch split over both - answers with the one context's bytes and statuses.
This file only makes the issuer's parameters and key (the oracle's) and hands them over."""
import os
import subprocess

import pytest

from tests.helpers import make_credentials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_request_wire") / "request_wire_doors")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "wire_issue.cpp", "wire_user.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_wire_issue.cpp", "fake_draw.cpp", "request_wire_doors.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_request_wire_doors_on_one_context_and_on_a_group(doors, tmp_path):
    d = make_credentials(4, "SSSS", 1, b"hostsim-request-wire")
    for name in ("params", "key", "ip"):
        (tmp_path / (name + ".bin")).write_bytes(bytes(d[name]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([doors, str(tmp_path)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "request wire doors ok" in r.stdout, (r.stdout[-1500:], r.stderr[-5000:])
