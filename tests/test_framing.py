"""CPU-only: the FRAMING of the three Schnorr statements - transcript and proof labels, the order of allocations, the terms of every
constraint - checked against text the reference holds, for all three implementations: oracle/ (C), tests/pyref/ (Python) and the
engine's SchnorrBuilder (aeonflux_amd/csrc/engine.cpp).

tests/golden/framing.json is extracted mechanically from the reference's src/nizk/{issuance,presentation,encryption}.rs by
tests/gen_framing.py: labels, their order, which labels sit in loops, and the constraints' terms as label names.  Where the
reference tree is present the extraction is repeated here and must equal the committed fixture.  expand() below turns the fixture
plus a concrete shape (number of attributes, their kinds, the hidden scalars) into the flat sequence a run must produce, and every
statement of every golden flow (tests/golden/flows.json), prover and verifier side, must log exactly that sequence in each
implementation.

What is mechanical and what is not: labels, order and terms come out of the fixture untouched.  How often a loop runs is NOT in
the text of the calls the extractor reads; MULTIPLICITY and LOOKUP below are a separate reading of the reference, one rule each with
its file and line.  What stays pinned only by our own restatements agreeing: the internals of zkp, merlin and dalek (how a label or
a point enters the sponge, what a compact proof's challenge is) - tests/test_pyref_cross_check.py and the third-party vectors.

Out of scope: blind issuance and batchable presentation proofs have no counterpart in the reference - the crate leaves blind
issuance as stubs and does not contain batchable proofs - so there is no text to extract their framing from."""
import copy
import json
import os
import subprocess

import pytest

from tests import gen_framing
from tests.helpers import pres_from_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aeonflux_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = gen_framing.DEFAULT_REFERENCE
H = bytes.fromhex

# amacs::Attribute as the user holds it (AFX_ATTR_*) and amacs::EncryptedAttribute as a presentation carries it (AFX_ENC_*)
ATTR_KINDS = ("PublicScalar", "SecretScalar", "PublicPoint", "EitherPoint", "SecretPoint")
ENC_KINDS = ("PublicScalar", "SecretScalar", "PublicPoint", "SecretPoint")


@pytest.fixture(scope="module")
def framing():
    with open(os.path.join(GOLDEN, "framing.json")) as f:
        return json.load(f)["statements"]


@pytest.fixture(scope="module")
def golden_flows():
    with open(os.path.join(GOLDEN, "flows.json")) as f:
        return json.load(f)["flows"]


# ---- the fixture against the reference's text ---------------------------------------------------------------------------------

needs_reference = pytest.mark.skipif(not all(os.path.exists(os.path.join(REF, p)) for p in gen_framing.SOURCES.values()),
                                     reason="the reference's sources are not on this machine")


@needs_reference
def test_the_fixture_is_what_the_extractor_reads_from_the_reference():
    with open(os.path.join(GOLDEN, "framing.json")) as f:
        committed = f.read()
    assert gen_framing.dumps(gen_framing.extract(REF)) == committed


@needs_reference
def test_the_extractor_fails_loudly():
    """no silent skip: a label that differs between prove and verify, an allocation in a form it does not know (the sources keep
    such calls, with computed labels, in comments: one is brought back) and a constraint it cannot read all stop the extraction"""
    import re
    texts = {}
    for name, rel in gen_framing.SOURCES.items():
        with open(os.path.join(REF, rel)) as f:
            texts[name] = f.read()
    assert gen_framing.extract_texts(texts) == gen_framing.extract(REF)
    for name in texts:
        # the verifier's first scalar label changed: the two sides disagree
        at = texts[name].index("allocate_scalar(b\"", texts[name].index("Verifier::new")) + len("allocate_scalar(b\"")
        with pytest.raises(gen_framing.FramingError, match="disagree"):
            gen_framing.extract_texts(dict(texts, **{name: texts[name][:at] + "q" + texts[name][at:]}))
        # the last constraint's call renamed to a constraint-like call of another shape
        at = texts[name].rindex(".constrain(")
        with pytest.raises(gen_framing.FramingError):
            gen_framing.extract_texts(dict(texts, **{name: texts[name][:at] + ".constrain(&mut " + texts[name][at + len(".constrain("):]}))
    commented = [(name, m) for name in texts for m in re.finditer(r"^(\s*)//\s*(.*allocate_\w+\(format!.*)$", texts[name], re.M)]
    assert len(commented) >= 8       # the commented-out calls the extractor must not pick up ...
    for name, m in commented:        # ... and must refuse once they are code
        with pytest.raises(gen_framing.FramingError):
            gen_framing.extract_texts(dict(texts, **{name: texts[name][:m.start()] + m.group(1) + m.group(2) + texts[name][m.end():]}))


def test_the_fixture_holds_labels_only(framing):
    """three statements, two sides each, the sides equal; nothing in it but labels, label names and attribute kind names"""
    assert sorted(framing) == ["encryption", "issuance", "presentation"]
    for name, sides in framing.items():
        assert sorted(sides) == ["prove", "verify"] and sides["prove"] == sides["verify"], name
        assert set(MULTIPLICITY[name](dict(n=4, g=4, kinds=["PublicScalar"] * 4, hidden=[]))) == {a["loop"] for a in sides["prove"]["allocations"] if a["loop"]}, name
    assert os.path.getsize(os.path.join(GOLDEN, "framing.json")) < 16384
    assert [a.get("skip_kinds") for a in framing["presentation"]["prove"]["allocations"] if a["label"] == "C_y"] == [["SecretPoint"]]


# ---- fixture + shape -> the flat expected sequence -----------------------------------------------------------------------------

class ReferencePanics(Exception):
    """the reference indexes out of range on this shape (it would panic): there is no sequence to expect"""


# How often each loop of a statement runs, by the label it allocates.  A separate reading of the reference (the extractor does not
# see it).  shape: n = NUMBER_OF_ATTRIBUTES, g = len(G_y), kinds = the attributes' kinds in position order, hidden = the attribute
# positions of the hidden scalars in allocation order.
MULTIPLICITY = {
    "issuance": lambda s: {
        "y": s["n"],       # issuance.rs:59 walks amacs_key.y, one per attribute (amacs.rs:98-100); :153 counts 0..NUMBER_OF_ATTRIBUTES
        "-G_y": s["g"],    # issuance.rs:79 and :170 walk system_parameters.G_y: "always at least three elements" (parameters.rs:235-243)
        "M": s["n"],       # issuance.rs:97 and :186 walk Messages::from_attributes: one message per attribute (amacs.rs:230-241)
    },
    "presentation": lambda s: {
        "m": len(s["hidden"]),     # presentation.rs:199 walks H_s_, filled for SecretScalar attributes only (:175-178); :366 walks hidden_scalar_indices
        "C_y": sum(1 for k in s["kinds"] if k != "SecretPoint"),   # presentation.rs:219-229 and :385-393: every commitment but those of hidden group elements
        "G_y": s["g"],             # presentation.rs:232 and :396 walk system_parameters.G_y (parameters.rs:235-243)
        "G_m": len(s["hidden"]),   # presentation.rs:242 walks H_s_ again; :404 walks H_s.0
    },
    "encryption": lambda s: {},    # encryption.rs:85-106 and :164-185: no loop
}
# `x[i]` in a term: H_s and G_m are the "hashmap-like" wrappers whose Index looks for the entry stored WITH attribute position i and
# panics without one (presentation.rs:72-82, :91-101); every other repeated label is a plain Vec indexed by position (G_y: :214, :380)
LOOKUP = {"m", "G_m"}


def expand(side, multiplicity, shape):
    """the flat sequence: transcript, proof, allocs [[kind, label]], constraints [[lhs point, [[scalar, point], ...]]] with variables as
    allocation indices, scalars and points counted apart (the form all three logs have)"""
    allocs, n_of, single, repeated = [], {"scalar": 0, "point": 0}, {}, {}
    for a in side["allocations"]:
        key = (a["kind"], a["label"])
        if a["loop"] is None:
            assert key not in single and key not in repeated
            single[key] = n_of[a["kind"]]
        else:
            assert key not in single
            repeated.setdefault(key, [])
        for _ in range(1 if a["loop"] is None else multiplicity[a["loop"]]):
            allocs.append([a["kind"], a["label"]])
            if a["loop"] is not None:
                repeated[key].append(n_of[a["kind"]])
            n_of[a["kind"]] += 1

    def element(kind, label, j):
        row = repeated[(kind, label)]
        if label in LOOKUP:
            if j not in shape["hidden"]:
                raise ReferencePanics("no hidden scalar stored with position %d" % j)
            j = shape["hidden"].index(j)
        if j >= len(row):
            raise ReferencePanics("%s[%d]" % (label, j))
        return row[j]

    def one(term_side, kind, j):
        return single[(kind, term_side)] if isinstance(term_side, str) else element(kind, term_side["at"], j)

    constraints = []
    for c in side["constraints"]:
        if "lhs" in c:
            terms = []
            for t in c["terms"]:
                if isinstance(t, dict):       # Iterator::zip stops with the shorter of the two
                    terms += [[s, p] for s, p in zip(repeated[("scalar", t["zip"][0])], repeated[("point", t["zip"][1])])]
                else:
                    terms.append([single[("scalar", t[0])], single[("point", t[1])]])
            constraints.append([single[("point", c["lhs"])], terms])
            continue
        # one constraint per element of the repeated label; the match looks at the attribute AT THE ELEMENT'S INDEX in that list
        # (presentation.rs:267-268 and :427-428: `i` counts the kept commitments, and indexes the attributes)
        for j, lhs in enumerate(repeated[("point", c["each"])]):
            if j >= len(shape["kinds"]):
                raise ReferencePanics("attributes[%d]" % j)
            arm = next((a for a in c["arms"] if shape["kinds"][j] in a["kinds"]), None) or next(a for a in c["arms"] if a["kinds"] == ["_"])
            if arm.get("skip"):
                continue
            constraints.append([lhs, [[one(t[0], "scalar", j), one(t[1], "point", j)] for t in arm["terms"]]])
    return dict(transcript=side["transcript"], proof=side["proof"], allocs=allocs, constraints=constraints)


def shape_of(n, kinds, hidden=None):
    return dict(n=n, g=max(n, 3), kinds=list(kinds), hidden=[i for i, k in enumerate(kinds) if k == "SecretScalar"] if hidden is None else list(hidden))


def expected_calls(framing, flow):
    """{call: list of expected statements | ReferencePanics} for issue, issuance_verify, show, verify of one golden flow, and
    "engine_verify": the same for the presentation the engine's own show describes (the fixture's may have been altered after show)"""
    n = flow["n"]
    ex = lambda name, side, shape: expand(framing[name][side], MULTIPLICITY[name](shape), shape)
    out = {"issue": [ex("issuance", "prove", shape_of(n, [ATTR_KINDS[k] for k in flow["issue"]["kinds"]]))],
           "issuance_verify": [ex("issuance", "verify", shape_of(n, [ATTR_KINDS[k] for k in flow["issue"]["kinds"]]))]}
    enc = lambda side: ex("encryption", side, shape_of(n, []))

    def guarded(make):
        try:
            return make()
        except ReferencePanics as e:
            return e
    sh = flow.get("show")
    if sh:
        kinds = [ATTR_KINDS[k] for k in sh["kinds"]]
        nsp = kinds.count("SecretPoint")
        if nsp and not sh.get("keypair"):
            out["show"] = []      # presentation.rs:150-157: no keypair for a hidden group element - the function returns before any transcript exists
        else:
            out["show"] = guarded(lambda: [ex("presentation", "prove", shape_of(n, kinds))] + [enc("prove")] * nsp)
        shown = ["PublicPoint" if k == "EitherPoint" else k for k in kinds]     # presentation.rs:295-307: what the verifier is sent
        out["engine_verify"] = guarded(lambda: [ex("presentation", "verify", shape_of(n, shown))] + [enc("verify")] * nsp)
    p = flow.get("presentation")
    if p:
        kinds = [ENC_KINDS[k] for k in p["kinds"]]
        out["verify"] = guarded(lambda: [ex("presentation", "verify", shape_of(n, kinds, p["hidden_scalar_indices"]))] + [enc("verify")] * len(p["enc"]))
    return out


def differs(log, expected):
    """None if the logged statements are exactly the expected ones, else where they part"""
    if len(log) != len(expected):
        return "%d statements, expected %d" % (len(log), len(expected))
    for k, (got, want) in enumerate(zip(log, expected)):
        for f in ("transcript", "proof", "allocs", "constraints"):
            if got[f] != want[f]:
                return "statement %d (%s): %s differs:\n got %r\nwant %r" % (k, want["proof"], f, got[f], want[f])
    return None


def check_calls(name, logs, expected, failed):
    """logs: {call: [statements]} of one implementation for one flow; failed: {call: True} where the implementation rejected.
    A verifier that rejects may have left where the reference returns its error - at an allocate_point that is handed the identity
    (the `?` of issuance.rs:162-189 and the like), or behind a main proof that does not verify, before the proofs of encryption
    are looked at (presentation.rs:435-440): what a rejecting call logged must be the beginning of the expected sequence."""
    n = 0
    for call, log in logs.items():
        want = expected[call]
        if isinstance(want, ReferencePanics):
            assert failed.get(call), (name, call, "the reference panics on this shape (%s): the call must fail" % want)
            continue
        if failed.get(call) and differs(log, want) is not None:
            assert 0 < len(log) <= len(want), (name, call)
            last, full = log[-1], want[len(log) - 1]
            assert differs(log[:-1], want[:len(log) - 1]) is None, (name, call)
            assert (last["transcript"], last["proof"]) == (full["transcript"], full["proof"]), (name, call)
            assert last["allocs"] == full["allocs"][:len(last["allocs"])] and last["constraints"] == full["constraints"][:len(last["constraints"])], (name, call)
            continue
        d = differs(log, want)
        assert d is None, (name, call, d)
        n += len(want)
    return n


def mutations(expected):
    """the three ways a shared misreading could look, applied to a copy of an expected sequence"""
    renamed = copy.deepcopy(expected)
    renamed[0]["allocs"][0][1] += "?"
    swapped = copy.deepcopy(expected)
    a = swapped[0]["allocs"]
    i = next(i for i in range(len(a) - 1) if a[i] != a[i + 1])
    a[i], a[i + 1] = a[i + 1], a[i]
    dropped = copy.deepcopy(expected)
    next(c for c in dropped[-1]["constraints"] if len(c[1]) > 1)[1].pop()
    return dict(renamed=renamed, swapped=swapped, dropped=dropped)


def check_negatives(logs, expected):
    """a renamed label, two neighbouring allocations swapped, a term dropped: each must make the comparison fail"""
    n = 0
    for call, log in logs.items():
        if isinstance(expected[call], ReferencePanics) or not expected[call] or differs(log, expected[call]) is not None:
            continue
        for what, wrong in mutations(expected[call]).items():
            assert differs(log, wrong) is not None, (call, what)
            n += 1
    return n


def test_expand_on_a_shape_worked_by_hand(framing):
    """n = 4, attributes (hidden scalar, revealed scalar, revealed point, hidden point): 4 scalars z z_0 t m; points I C_x_1 C_x_0
    G_x_0 G_x_1, three C_y (positions 0 1 2), four G_y, one G_m, Z = 15; constraint #3 runs over the three kept commitments and
    looks at attributes 0, 1, 2"""
    s = expand(framing["presentation"]["prove"], MULTIPLICITY["presentation"](shape_of(4, ["SecretScalar", "PublicScalar", "PublicPoint", "SecretPoint"])),
               shape_of(4, ["SecretScalar", "PublicScalar", "PublicPoint", "SecretPoint"]))
    assert [l for k, l in s["allocs"]] == ["z", "z_0", "t", "m", "I", "C_x_1", "C_x_0", "G_x_0", "G_x_1", "C_y", "C_y", "C_y", "G_y", "G_y", "G_y", "G_y", "G_m", "Z"]
    assert s["constraints"] == [[13, [[0, 0]]], [1, [[2, 2], [1, 3], [0, 4]]], [5, [[0, 8], [3, 12]]], [6, [[0, 9]]], [7, [[0, 10]]]]
    # fewer than three attributes: three G_y all the same (parameters.rs:235-243), and the zip of n scalars with them stops at n
    s = expand(framing["issuance"]["verify"], MULTIPLICITY["issuance"](shape_of(1, ["PublicScalar"])), shape_of(1, ["PublicScalar"]))
    assert [l for k, l in s["allocs"]].count("-G_y") == 3 and [l for k, l in s["allocs"]].count("y") == 1
    assert s["constraints"][1] == [9, [[5, 0], [2, 3], [3, 4], [4, 5]]]
    # a hidden scalar behind a hidden group element: the kept commitment of position 1 sits at index 0, where the attribute is the
    # hidden point (skipped); index 1 looks at attribute 1, the hidden scalar - stored with position 1: found
    sh = shape_of(2, ["SecretPoint", "SecretScalar"])
    assert len(expand(framing["presentation"]["verify"], MULTIPLICITY["presentation"](sh), sh)["constraints"]) == 2
    sh = shape_of(3, ["SecretPoint", "PublicScalar", "SecretScalar"])   # index 1: a revealed scalar; the hidden one (position 2) is never looked up
    assert len(expand(framing["presentation"]["verify"], MULTIPLICITY["presentation"](sh), sh)["constraints"]) == 2 + 1
    sh = shape_of(3, ["PublicScalar", "SecretScalar", "PublicScalar"], hidden=[2])   # a presentation that names the wrong position: H_s[1] panics
    with pytest.raises(ReferencePanics):
        expand(framing["presentation"]["verify"], MULTIPLICITY["presentation"](sh), sh)


# ---- the three implementations ---------------------------------------------------------------------------------------------------

def test_the_oracle_frames_every_flow_as_the_reference_does(framing, golden_flows):
    import oracle
    checked = negatives = 0
    for f in golden_flows:
        expected = expected_calls(framing, f)
        issuer = oracle.Ctx(H(f["params"]), H(f["key"]), H(f["issuer_params"]))
        user = oracle.Ctx(H(f["params"]), None, H(f["issuer_params"]))
        logs, failed = {}, {}

        def logged(call, fn):
            oracle.framing_log(True)
            try:
                r = fn()
                logs[call] = oracle.framing_log_read()
            finally:
                oracle.framing_log(False)
            return r
        i = f["issue"]
        vals = [H(v) for v in i["values"]]
        st, t, U, V, ch, resp = logged("issue", lambda: issuer.issue(i["kinds"], vals, H(i["t_wide"]), H(i["U_wide"]), H(i["rng_seed"])))
        assert st == 0
        failed["issuance_verify"] = logged("issuance_verify", lambda: user.issuance_verify(i["kinds"], vals, t, U, V, ch, resp)) != 0
        s = f["show"]
        st, p = logged("show", lambda: user.show(s["kinds"], [H(v) for v in s["values"]], t, U, V, H(s["keypair"]) if s["keypair"] else None,
                                                 H(s["z_wide"]), H(s["rng_seed"]), H(s["enc_seeds"])))
        failed["show"] = st != 0
        if "presentation" in f:
            failed["verify"] = logged("verify", lambda: issuer.verify_presentation(pres_from_json(f))) != 0
        checked += check_calls(f["name"], logs, expected, failed)
        negatives += check_negatives(logs, expected)
    assert checked >= 4 * 15 and negatives >= 3 * 4 * 15, (checked, negatives)
    assert oracle.framing_log_read() == []       # off: nothing is recorded


def test_pyref_frames_every_flow_as_the_reference_does(framing, golden_flows):
    from tests.pyref import statements as S, zkp
    checked = negatives = 0
    for f in golden_flows:
        expected = expected_calls(framing, f)
        params, key, ip = H(f["params"]), H(f["key"]), H(f["issuer_params"])
        logs, failed = {}, {}

        def logged(call, fn):
            zkp.LOG = []
            try:
                r = fn()
                logs[call] = zkp.LOG
            finally:
                zkp.LOG = None
            return r
        i = f["issue"]
        vals = [H(v) for v in i["values"]]
        st, o = logged("issue", lambda: S.issue(params, key, ip, i["kinds"], vals, H(i["t_wide"]), H(i["U_wide"]), H(i["rng_seed"])))
        assert st == 0
        failed["issuance_verify"] = logged("issuance_verify", lambda: S.issuance_verify(params, ip, i["kinds"], vals, o["t"], o["U"], o["V"], o["challenge"], o["responses"]))[0] != 0
        s = f["show"]
        st, p = logged("show", lambda: S.show(params, ip, s["kinds"], [H(v) for v in s["values"]], o["t"], o["U"], o["V"], H(s["keypair"]) if s.get("keypair") else None,
                                              H(s["z_wide"]), H(s["rng_seed"]), H(s["enc_seeds"])))
        failed["show"] = st != 0
        if "presentation" in f:
            w = f["presentation"]
            pres = dict(kinds=w["kinds"], attr_values=[H(v) for v in w["attr_values"]], hidden_scalar_indices=w["hidden_scalar_indices"], challenge=H(w["challenge"]),
                        responses=[H(r) for r in w["responses"]], C_x_0=H(w["C_x_0"]), C_x_1=H(w["C_x_1"]), C_V=H(w["C_V"]), C_y=[H(c) for c in w["C_y"]],
                        enc=[dict(index=e["index"], challenge=H(e["challenge"]), responses=[H(r) for r in e["responses"]],
                                  **{k: H(e[k]) for k in ("pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p")}) for e in w["enc"]])
            failed["verify"] = logged("verify", lambda: S.verify_presentation(params, key, ip, pres))[0] != 0
        checked += check_calls(f["name"], logs, expected, failed)
        negatives += check_negatives(logs, expected)
    assert checked >= 4 * 15 and negatives >= 3 * 4 * 15, (checked, negatives)


@pytest.fixture(scope="module")
def framing_log_program(tmp_path_factory):
    """tests/hostsim/framing_log.cpp with the engine's host sources (SchnorrBuilder logging: -DAFX_FRAMING_LOG) on the fake HIP runtime; no sanitizer"""
    out = str(tmp_path_factory.mktemp("framing_log") / "framing_log")
    srcs = [os.path.join(CSRC, f) for f in ("engine.cpp", "plans.cpp", "statements.cpp", "statements_prove.cpp", "statements_setup.cpp", "group.cpp", "mixed.cpp", "wire.cpp")]
    srcs += [os.path.join(ROOT, "tests", "hostsim", f) for f in ("fake_hip.cpp", "framing_log.cpp")]
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-DAFX_FRAMING_LOG", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-pthread", "-o", out] + srcs,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_the_engine_frames_every_flow_as_the_reference_does(framing, golden_flows, framing_log_program, tmp_path):
    args = []
    for k, f in enumerate(golden_flows):
        for field in ("params", "key", "issuer_params"):
            path = tmp_path / ("%d.%s" % (k, field))
            path.write_bytes(H(f[field]))
            args.append(str(path))
        no_keypair = 4 in f["show"]["kinds"] and not f["show"].get("keypair")
        args += ["".join(str(x) for x in f["issue"]["kinds"]), ("!" if no_keypair else "") + "".join(str(x) for x in f["show"]["kinds"])]
    r = subprocess.run([framing_log_program] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    per_flow = [dict(issue=[], issuance_verify=[], show=[], engine_verify=[]) for _ in golden_flows]
    for line in r.stdout.splitlines():
        d = json.loads(line)
        shape, call = d.pop("shape"), d.pop("call")
        per_flow[shape]["engine_verify" if call == "verify" else call].append(d)
    checked = negatives = 0
    for f, logs in zip(golden_flows, per_flow):
        expected = expected_calls(framing, f)
        if expected["show"] == []:
            assert logs.pop("engine_verify") == []      # (no keypair, no presentation: the program does not go on to verify)
        # the program runs zeros through no-op kernels, so no status says whether a statement was built to its end: every sequence
        # must be complete - except where the reference would panic, where the engine must not have built the statement at all
        for call in [c for c in logs if isinstance(expected[c], ReferencePanics)]:
            assert logs.pop(call) == [], (f["name"], call)
        checked += check_calls(f["name"], logs, expected, {})
        negatives += check_negatives(logs, expected)
    assert checked >= 4 * 15 and negatives >= 3 * 4 * 15, (checked, negatives)


def test_the_shipped_library_carries_no_framing_log():
    """the switch is for the test program only: neither the build recipe nor the built library knows the log"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "AFX_FRAMING_LOG" not in f.read()
    lib = os.path.join(ROOT, "aeonflux_amd", "lib", "libaeonflux_gpu.so")
    if os.path.exists(lib):
        import ctypes
        assert not hasattr(ctypes.CDLL(lib), "afx_framing_log_text")
