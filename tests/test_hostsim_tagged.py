"""CPU-only: the calls of the presentation tags (aeonflux_amd/csrc/statements_tags.cpp; the tagged plans of statements_prove.cpp and
statements.cpp) on the engine's host half, built against the fake HIP runtime under ASan/UBSan with its own source list: the engine's
host sources plus statements_tags.cpp, tests/hostsim/fake_hip.cpp, the stand-ins for the masking and the tag launchers (fake_blind.cpp,
fake_tags.cpp) and the driver, tests/hostsim/tagged_doors.cpp - a program of its own, so the sanitizers' runtimes are linked in and
nothing is preloaded.  AFX_PLAN_SELFCHECK for the whole run: every plan is assembled twice and must relocate to the same bytes.  The
driver checks null arguments, a position of the wrong kind, a scope generator that is zero or does not decode (AFX_E_BAD_ARGS, nothing
written), count 0, a two-pass call with ONE inversion launch, what a tag adds to a verification plan (the fixed-base job and exactly two
chains) and that untagged plans count afterwards what they counted before.  This file only makes the issuer's parameters and key (the
oracle's) and hands them over."""
import os
import subprocess

import pytest

from tests.helpers import make_credentials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_tagged") / "tagged_doors")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "statements_tags.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "fake_blind.cpp", "fake_tags.cpp", "tagged_doors.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_tagged_doors_argument_errors_passes_and_plan_counts(doors, tmp_path):
    d = make_credentials(4, "SSSS", 1, b"hostsim-tagged")
    for name in ("params", "key", "ip"):
        (tmp_path / (name + ".bin")).write_bytes(bytes(d[name]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([doors, str(tmp_path)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "tagged doors ok" in r.stdout, (r.stdout[-1500:], r.stderr[-5000:])
