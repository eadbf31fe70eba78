"""CPU-only: every door that takes a presentation's column structs, swept array by array from the one table that describes them
(aeonflux_amd/csrc/batch_arrays.hpp), on the engine's host half: built against the fake HIP runtime under ASan/UBSan with its own source
list - the engine's host sources with statements_tags.cpp and wire_batchable.cpp, tests/hostsim/fake_hip_counted.cpp (the fake HIP runtime
of fake_hip.cpp with its copies and finishing launches counted), the stand-in launchers and the driver, tests/hostsim/batch_array_doors.cpp - a program of its own, so the sanitizers' runtimes are linked in and nothing is
preloaded.  AFX_PLAN_SELFCHECK for the whole run.  At three layouts of 3 items (one attribute of each kind; no hidden group element, enc
null; two hidden group elements) and every door - afx_verify_presentations[_range,_dev], afx_verify_encryption_proofs[_dev], the batchable
and tagged verifications with their _dev forms, afx_show / afx_show_batchable / afx_show_tagged, the two packers - the untouched call is
AFX_OK and a call with any one array the shape reads set to null is AFX_E_BAD_ARGS with no plan launched and the status bytes untouched;
an array the shape does not read may be null; and both packers put every cell where the format comments say.  This file only makes the
issuer's parameters and key (the oracle's) and hands them over."""
import os
import subprocess

import pytest

from tests.helpers import make_credentials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_batch_arrays") / "batch_array_doors")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp",
                                            "statements_tags.cpp", "wire_batchable.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip_counted.cpp", "fake_blind.cpp", "fake_tags.cpp", "fake_batchable.cpp", "fake_wire_issue.cpp",
                                                                 "batch_array_doors.cpp")]
    r = subprocess.run(["g++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-pthread", "-o", out] + srcs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_door_refuses_each_null_array_it_reads_and_packers_place_every_cell(doors, tmp_path):
    d = make_credentials(4, "SSSS", 1, b"hostsim-batch-arrays")
    for name in ("params", "key", "ip"):
        (tmp_path / (name + ".bin")).write_bytes(bytes(d[name]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", AFX_PLAN_SELFCHECK="1")
    r = subprocess.run([doors, str(tmp_path)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "batch array doors ok" in r.stdout, (r.stdout[-1500:], r.stderr[-5000:])
