"""CPU-only: the hole-offset sweep of tests/test_gpu_hash_kernels.py on the host simulation, against the oracle.

The engine's host half compiles a scripted transcript to the device's byte schedule (strobe_sim.hpp StrobeSim::to_device); the fake
runtime's hash launcher, with its `hash` knob on, runs that schedule word by word the way kernels.hip k_hash does
(tests/hostsim/fake_hip.cpp).  A 32-byte per-item hole at every position of the 166-byte rate - with a second hole the closest
behind it that a script can put one - must compile (a word that took bytes of two fields would be refused: "word spans two fields")
and give oracle.merlin_script's 64 bytes for every item: an error in the schedule's (q, r, fmask, keep) shows here, without a GPU.
What this cannot see is the device kernels' own lane arithmetic; tests/test_gpu_hash_kernels.py runs the same scripts there.
A plain build: no sanitizer (tests/test_hostsim.py drives the same entry point under ASan/UBSan)."""
import os
import subprocess
import sys

import pytest

from tests import hash_sweep as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")


@pytest.fixture(scope="module")
def hostsim_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostsim_hash") / "libafx_hostsim.so")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp")]
    srcs.append(os.path.join(ROOT, "tests", "hostsim", "fake_hip.cpp"))
    r = subprocess.run(["g++", "-O1", "-fPIC", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-shared", "-pthread", "-o", out] + srcs,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


DRIVER = r"""
import sys, ctypes as C
sys.path.insert(0, %(root)r)
import numpy as np
import aeonflux_amd as afx
afx.LIB_PATH = %(lib)r
import oracle
from tests import hash_sweep as hs
from tests.helpers import make_credentials
L = afx.lib()
L.afx_fake_set.argtypes = [C.c_char_p, C.c_int]
L.afx_fake_set(b"hash", 1)
d = make_credentials(1, "S", 1, b"hostsim-hash-sweep")
ctx = afx.Context(d["params"], d["key"], d["ip"])
count = 3
fields = hs.fields_for(b"hostsim", count)
arrays = [np.frombuffer(f, np.uint8).reshape(count, 32) for f in fields]
bad = []
for small in (4096, 0):            # both launchers of the fake runtime
    ctx.set_small_batch_items(small)
    for k in hs.K_RANGE:
        ops = hs.sweep_ops(k)
        out = ctx.merlin_challenges(hs.SWEEP_LABEL, ops, arrays, count)
        for i in range(count):
            if bytes(out[i]) != oracle.merlin_script(hs.SWEEP_LABEL, ops, [f[32 * i:32 * i + 32] for f in fields])[0]:
                bad.append((small, k, i))
assert not bad, ("(threshold, pad length, item) that differ from the oracle", bad[:20], len(bad))
# ... and challenges of every length class in mid-script (partial keep masks)
for n in (1, 7, 8, 9, 31, 32, 33, 63, 64):
    ops = [("append_field", b"first", 0), ("challenge", b"mid", n), ("append_field", b"second", 1), ("challenge", b"last", 32)]
    out = ctx.merlin_challenges(b"mid-script challenges", ops, arrays, count)
    for i in range(count):
        assert bytes(out[i, :32]) == oracle.merlin_script(b"mid-script challenges", ops, [f[32 * i:32 * i + 32] for f in fields])[1], (n, i)
# the knob off: the launchers are no-ops again (what every other host simulation relies on)
L.afx_fake_set(b"hash", 0)
assert not ctx.merlin_challenges(hs.SWEEP_LABEL, hs.sweep_ops(5), arrays, count).any()
# the launch accounting tells the kernels apart by the launcher's own rule (plan.h AFX_HASH_COOP_ON_WAVE); "k_hash" is the three together
def launches(variants, small, n):
    ctx.set_plan_variants(variants)
    ctx.set_small_batch_items(small)
    ctx.set_timing(True)
    f = [np.zeros((n, 32), np.uint8)] * 2
    ctx.merlin_challenges(hs.SWEEP_LABEL, hs.sweep_ops(5), f, n)
    got = tuple(ctx.get_timing(k)[1] for k in ("k_hash_coop64", "k_hash_coop", "k_hash"))
    ctx.set_timing(False)
    return got
assert launches(0, 4096, 2048) == (1, 0, 1) and launches(0, 4096, 2049) == (0, 1, 1) and launches(0, 4096, 4096) == (0, 1, 1)
assert launches(0, 4096, 4097) == (0, 0, 1) and launches(0, 0, 3) == (0, 0, 1) and launches(afx.VARIANT_HASH_HALF_WAVE, 4096, 3) == (0, 1, 1)
ctx.close()
print("ok")
"""


def test_a_hole_at_every_offset_of_the_rate_on_the_host_simulation(hostsim_lib):
    c = hs.coverage()     # what the sweep is there for, from the restated position arithmetic (tests/hash_sweep.py)
    assert c["starts"] == set(range(hs.R)) and c["qrs"] == hs.ALL_QR and c["cut"] == set(range(1, 32)) and c["word20"] >= 6
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT, "lib": hostsim_lib}], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-5000:])
