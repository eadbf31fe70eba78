"""CPU-only: the header functions of the six wire formats (*_wire_parse, *_wire_section_bytes, *_wire_header_bytes,
*_wire_cells_per_record; aeonflux_amd/csrc/wire_formats.hpp) answer every case of tests/wire_header_cases.py as the commit that recorded
tests/golden/wire_headers.json answered it: return code, every out-parameter, and the text of afx_last_error() - which is API, the
Python layer raises with it.  The fixture is never regenerated from the code under test (tests/gen_wire_headers.py says how it was made)."""
import json
import os

import pytest

import aeonflux_amd as afx
from tests import wire_header_cases as whc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "wire_headers.json")) as f:
        return json.load(f)


def test_fixture_is_small_and_names_its_cases(recorded):
    size = os.path.getsize(os.path.join(GOLDEN, "wire_headers.json"))
    others = [os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "wire_headers.json"]
    assert size <= max(others)
    assert recorded["recorded_at"]
    # the generator still makes the cases the fixture was recorded for, every format among them
    assert recorded["cases_sha256"] == whc.digest()
    assert {f.name for f, _, _ in whc.cases()} == {"AFXP", "AFXB", "AFXR", "AFXI", "AFXQ", "AFXJ"}


def test_every_case_answers_as_recorded(recorded):
    lib = afx.lib()
    strings, outcomes = recorded["strings"], recorded["outcomes"]
    want_idx = [v for v, run in recorded["case_outcomes"] for _ in range(run)]
    assert len(want_idx) == recorded["cases"]
    n = 0
    accepted = {f.name: 0 for f in whc.FORMATS}
    for (f, what, blob), wi in zip(whc.cases(), want_idx):
        want = [[o[0], None if o[1] is None else strings[o[1]]] + o[2:] for o in outcomes[wi]]
        got = [list(o) for o in whc.outcome(lib, f, blob)]
        assert got == want, what
        accepted[f.name] += got[0][0] == 0
        n += 1
    assert n == recorded["cases"]
    assert all(accepted.values()), accepted   # (every format has sections that parse: the fixture is not a list of refusals)


def test_layout_sweep_as_recorded(recorded):
    got = whc.sweep(afx.lib())
    assert len(got) == afx.MAX_ATTRIBUTES + 2
    for n, (g, w) in enumerate(zip(got, recorded["sweep"])):
        assert g == w, "n = %d" % n
