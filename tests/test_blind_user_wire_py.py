"""CPU-only: the Python mirror of the user's doors of blind issuance on bytes (include/aeonflux_gpu.h "Blind issuance on bytes: the
user's doors").  Every prototype the header's section declares is one the loaded library exports and aeonflux_amd gave argument types
to; the two structs have the header's fields; and the draw labels' lengths are the header's AFX_DRAW_BYTES."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aeonflux_gpu.h")


def user_doors_section():
    text = open(HEADER).read()
    start = text.index("/* ---- Blind issuance on bytes: the user's doors")
    return text[start:text.index("/* ---- setup helpers", start)]


def test_python_declares_every_prototype_of_the_headers_section():
    import aeonflux_amd as afx
    names = re.findall(r"^int (afx_\w+)\(", user_doors_section(), re.M)
    assert sorted(names) == sorted(["afx_blind_request_wire", "afx_group_blind_request_wire", "afx_blind_request_wire_rng", "afx_group_blind_request_wire_rng",
                                    "afx_unblind_issuances_wire", "afx_group_unblind_issuances_wire", "afx_unblind_issuances_wire_rng",
                                    "afx_group_unblind_issuances_wire_rng"])
    lib = afx.lib()
    for name in names:
        fn = getattr(lib, name)          # AttributeError: the library does not export it
        assert fn.argtypes, name         # None: aeonflux_amd never declared it
        params = re.search(r"^int %s\((.*?)\);" % name, user_doors_section(), re.M | re.S).group(1)
        assert len(fn.argtypes) == params.count(",") + 1, name
    from aeonflux_amd import wire
    for name in ("blind_request_wire", "blind_request_wire_rng", "unblind_issuances_wire", "unblind_issuances_wire_rng"):
        assert callable(getattr(wire, name))


def test_structs_have_the_headers_fields():
    import aeonflux_amd as afx
    section = user_doors_section()
    for cname, cls in (("afx_blind_request_group", afx.BlindRequestGroup), ("afx_credential_out", afx.CredentialOut)):
        body = re.search(r"^struct %s \{(.*?)^\};" % cname, section, re.M | re.S).group(1)
        fields = re.findall(r"(\w+);", body)
        assert [f for f, _ in cls._fields_] == fields, cname
    assert C.sizeof(afx.BlindRequestGroup) == C.sizeof(afx.AttributesSoA) + 4 * 8
    assert C.sizeof(afx.CredentialOut) == 3 * 8


def test_draw_label_arithmetic():
    import aeonflux_amd as afx
    assert (afx.DRAW_BLINDREQ_D_WIDE, afx.DRAW_BLINDREQ_SEED, afx.DRAW_BLINDREQ_R_WIDE(0), afx.DRAW_BLINDREQ_R_WIDE(31)) == (69, 70, 71, 102)
    assert [afx.draw_bytes(label) for label in (69, 70, 71, 102)] == [64, 32, 64, 64]
    assert afx.draw_bytes(103) == 32 and afx.draw_bytes(68) == 32          # the neighbours keep their lengths
    # ... and the header's macro says the same (evaluated from its text)
    text = open(HEADER).read()
    cond = re.search(r"#define AFX_DRAW_BYTES\(label\) \((.*?)\? 64u : 32u\)", text, re.S).group(1).replace("\\\n", " ")
    defs = dict(re.findall(r"#define (AFX_DRAW_[A-Z_]+) (\d+)u", text))
    for name in sorted(defs, key=len, reverse=True):
        cond = re.sub(r"\b%s\b(?!\()" % name, defs[name], cond)
    cond = re.sub(r"AFX_DRAW_BLINDREQ_R_WIDE\((\d+)\)", lambda m: str(71 + int(m.group(1))), cond)
    cond = re.sub(r"(\d+)u\b", r"\1", cond).replace("||", " or ").replace("&&", " and ")
    cond = " ".join(cond.split())
    for label, want in ((69, 64), (70, 32), (71, 64), (102, 64), (103, 32), (0, 64), (2, 32), (67, 64), (68, 32)):
        assert (64 if eval(cond.replace("(label)", "(%d)" % label)) else 32) == want, (label, cond)
