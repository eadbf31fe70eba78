"""CPU-only: the user's doors of blind issuance on bytes (aeonflux_amd/csrc/wire_blind_user.cpp) on the engine's host half, built
against the fake HIP runtime under ASan/UBSan with its own source list: the engine's host sources plus statements_blind.cpp,
wire_blind.cpp, wire_blind_user.cpp, tests/hostsim/fake_hip.cpp, the stand-ins for the masking, the record-writing and the draw
launchers (fake_blind.cpp, fake_wire_issue.cpp, fake_draw.cpp) and the driver, tests/hostsim/blind_user_doors.cpp - a program of its
own, so the sanitizers' runtimes are linked in and nothing is preloaded.  AFX_PLAN_SELFCHECK for the whole run: every plan is assembled
twice and must relocate to the same bytes, a reused one must equal a fresh one.  The inputs are all zeros, so every item fails: the
driver checks sizes, headers, what an argument error leaves untouched, zero records and zero t, U, V, two and three slices, the group's
two paths, and where the _rng forms' seed, d_wide rows and d rows go (and that d is copied to an output row only for a caller that asked).  This file only makes the issuer's parameters and key (the oracle's) and
hands them over."""
import os
import subprocess

import pytest

from tests.helpers import make_credentials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
# afxk_reduce_wide and afxk_soa_to_aos as the linker knows them: the driver wraps both (ld --wrap) to see where d is written, copied and
# wiped - the stand-in for k_reduce_wide in fake_hip.cpp writes nothing (the driver's WRAP_* are the same two names)
WRAP_REDUCE_WIDE = "_Z16afxk_reduce_wideP12ihipStream_tPKhPhj"
WRAP_SOA_TO_AOS = "_Z15afxk_soa_to_aosP12ihipStream_tPKhPhPKjS2_jj"


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_blind_user_wire") / "blind_user_doors")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "statements_blind.cpp", "wire_blind.cpp", "wire_blind_user.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_blind.cpp", "fake_wire_issue.cpp", "fake_draw.cpp", "blind_user_doors.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-Wl,--wrap=" + WRAP_REDUCE_WIDE, "-Wl,--wrap=" + WRAP_SOA_TO_AOS, "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_blind_user_doors_sizes_errors_zero_outputs_slices_groups_and_wipes(doors, tmp_path):
    d = make_credentials(4, "SSSS", 1, b"hostsim-blind-user-wire")
    for name in ("params", "key", "ip"):
        (tmp_path / (name + ".bin")).write_bytes(bytes(d[name]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([doors, str(tmp_path)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "blind user doors ok" in r.stdout, (r.stdout[-1500:], r.stderr[-5000:])
