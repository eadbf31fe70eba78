"""Extracts the FRAMING of the reference's three Schnorr statements from its source text into tests/golden/framing.json.

Framing = what a statement feeds its transcript before any value: the merlin label, the proof label, the allocations in order
(scalar | point, label) and the constraints (left-hand side and (scalar, point) terms).  oracle/, tests/pyref/ and the engine's
SchnorrBuilder each restate it from one reading of the crate; a label or an order wrong in all three would pass every other test
here and reject every proof the crate makes.  This script reads that framing out of the crate's own text instead, mechanically:
    src/nizk/issuance.rs, src/nizk/presentation.rs, src/nizk/encryption.rs - the bodies of `prove` and `verify`.
It runs on the build machine only (the reference tree is not part of this repository); tests/test_framing.py re-runs it where the
tree is present and compares with the committed fixture.

    python tests/gen_framing.py [reference root]      # writes tests/golden/framing.json

What it understands - and it FAILS on anything else that mentions an allocation or a constraint, so that nothing is skipped
silently - are the call forms the three files use (the search patterns are ours; no source text is copied anywhere):
    the transcript and the prover / verifier being made, each with a byte-string label;
    a variable bound to one allocation, directly or as the first of a pair; an allocation pushed onto a vector, alone or beside an
        index; a variable allocated inside a loop and then pushed onto a vector (the vector then stands for the repeated label);
    a constraint whose terms are listed in place, or collected in a vector by pushes of single terms and by one extension with two
        repeated labels zipped; a constraint per element of a repeated label, chosen by a match on the attribute's kind.
Lines that are commented out are dropped first (the sources keep older allocation calls in comments).

The fixture holds label strings, lists of label names and attribute kind names - nothing else.  For each statement and each side:
    transcript, proof          the two labels
    allocations                [{kind, label, loop}]: loop = null, or the name of the loop the call sits in (a loop is named by the
                               first label allocated in it); skip_kinds = the attribute kinds whose arm of an enclosing match allocates nothing
    constraints                [{lhs, terms}] with terms [scalar label, point label] or {"zip": [scalar label, point label]} (two
                               repeated labels, element by element), or
                               {each, arms}: one constraint per element of the repeated label `each`; arms [{kinds, skip}] or
                               [{kinds, terms}], a term's side being a label or {"at": repeated label} (its element for this position)
How often a loop runs is not in the text of these calls and not in the fixture (tests/test_framing.py states it separately).
The two sides of a statement must agree on all of it, or the extraction fails."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_REFERENCE = os.environ.get("AFX_REFERENCE_DIR", "/root/reference")   # (as tests/test_integration_patch.py finds it)
FIXTURE = os.path.join(ROOT, "tests", "golden", "framing.json")
SOURCES = {"issuance": "src/nizk/issuance.rs", "presentation": "src/nizk/presentation.rs", "encryption": "src/nizk/encryption.rs"}
SIDES = ("prove", "verify")


class FramingError(Exception):
    pass


def strip_comments(text):
    """drop // comments (to the end of the line) and /* */ comments, leaving string literals alone"""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == '"':
            j = i + 1
            while j < n and text[j] != '"':
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
        else:
            out.append(c)
            i += 1
    return "".join(out)


def matching(text, i):
    """index of the bracket that closes the one at text[i] (string literals skipped)"""
    pairs = {"{": "}", "(": ")", "[": "]"}
    stack, j, n = [], i, len(text)
    while j < n:
        c = text[j]
        if c == '"':
            j += 1
            while text[j] != '"':
                j += 2 if text[j] == "\\" else 1
        elif c in pairs:
            stack.append(pairs[c])
        elif c in ")]}":
            if not stack or stack.pop() != c:
                raise FramingError("unbalanced brackets")
            if not stack:
                return j
        j += 1
    raise FramingError("unbalanced brackets")


def function_body(text, name):
    m = re.search(r"\bfn\s+%s\b" % name, text)
    if not m:
        raise FramingError("no function %s" % name)
    paren = text.index("(", m.end())
    brace = text.index("{", matching(text, paren))
    return text[brace + 1:matching(text, brace)]


BLOCK_HEADS = ("for ", "match ", "if ", "else", "while ", "loop")


def parse_block(text):
    """[("stmt", text) | ("block", header, inner)]: statements end at a `;` outside every bracket; a `{` outside parentheses opens a
    block when what stands before it is a loop / match / if header, and is part of the statement otherwise (a struct literal)"""
    items, start, i, n = [], 0, 0, len(text)
    while i < n:
        c = text[i]
        if c == '"':
            i += 1
            while text[i] != '"':
                i += 2 if text[i] == "\\" else 1
        elif c in "([":
            i = matching(text, i)
        elif c == "{":
            head = " ".join(text[start:i].split())
            end = matching(text, i)
            if head.startswith(BLOCK_HEADS):
                items.append(("block", head, text[i + 1:end]))
                start = end + 1
            i = end
        elif c == ";":
            s = " ".join(text[start:i].split())
            if s:
                items.append(("stmt", s))
            start = i + 1
        i += 1
    s = " ".join(text[start:].split())
    if s:
        items.append(("stmt", s))     # a block's closing expression
    return items


def parse_arms(inner):
    """[(pattern, body text)] of a match block"""
    arms, i, n = [], 0, len(inner)
    while i < n:
        if inner[i].isspace() or inner[i] == ",":
            i += 1
            continue
        j = i
        while not inner.startswith("=>", j):       # the pattern: up to `=>` outside brackets
            j = matching(inner, j) + 1 if inner[j] in "([{" else j + 1
            if j >= n:
                raise FramingError("a match arm without `=>`")
        pattern = " ".join(inner[i:j].split())
        j += 2
        while inner[j].isspace():
            j += 1
        if inner[j] == "{":
            end = matching(inner, j)
            arms.append((pattern, inner[j + 1:end]))
            i = end + 1
        else:
            k = j
            while k < n and inner[k] != ",":
                k = matching(inner, k) + 1 if inner[k] in "([{" else k + 1
            arms.append((pattern, inner[j:k]))
            i = k + 1
    return arms


def kind_of(pattern):
    """the attribute kind a match pattern names: the last path segment before any payload; `_` for the catch-all"""
    if pattern == "_":
        return "_"
    m = re.fullmatch(r"(?:\w+::)*(\w+)\s*(\(.*\)|\{.*\})?", pattern)
    if not m:
        raise FramingError("match pattern not understood: %r" % pattern)
    return m.group(1)


ID = r"[A-Za-z_]\w*"
LABEL = r'b"([^"\\]*)"'
RE_TRANSCRIPT = re.compile(r"let mut (%s) = Transcript::new\(%s\)" % (ID, LABEL))
RE_BUILDER = re.compile(r"let mut (%s) = (Prover|Verifier)::new\(%s, &mut (%s)\)" % (ID, LABEL, ID))
RE_ALLOC = r"(%s)\.allocate_(scalar|point)\(%s\s*(?:,.*)?\)\??" % (ID, LABEL)
RE_LET_ALLOC = re.compile(r"let (?:(%s)|\((%s), _\)) = %s" % (ID, ID, RE_ALLOC))
RE_PUSH_ALLOC = re.compile(r"(%s)\.push\((?:\(\*?%s(?: as \w+)?, )?%s\)?\)" % (ID, ID, RE_ALLOC))
RE_PUSH_NAME = re.compile(r"(%s)\.push\((?:\(\*?%s(?: as \w+)?, (%s)\)|(%s))\)" % (ID, ID, ID, ID))
RE_TERMLIST = re.compile(r"let mut (%s): Vec<\(ScalarVar, PointVar\)> = Vec::with_capacity\(.*\)" % ID)
RE_PUSH_TERM = re.compile(r"(%s)\.push\(\((%s), (%s)\)\)" % (ID, ID, ID))
RE_EXTEND_ZIP = re.compile(r"(%s)\.extend\((%s)\.iter\(\)\.copied\(\)\.zip\((%s)\.iter\(\)\.copied\(\)\)\)" % (ID, ID, ID))
RE_CONSTRAIN = re.compile(r"(%s)\.constrain\((\*?%s), (.*)\)" % (ID, ID))
RE_FOR_EACH = re.compile(r"for \((%s), (%s)\) in (%s)\.iter\(\)\.enumerate\(\)" % (ID, ID, ID))
RE_TERM = re.compile(r"\((%s)(\[%s\])?, (%s)(\[%s\])?\)" % (ID, ID, ID, ID))


class Side:
    """one function body, walked once"""

    def __init__(self, body, where):
        self.where = where
        self.transcript_var = self.builder = None
        self.out = dict(transcript=None, proof=None, allocations=[], constraints=[])
        self.names = {}        # variable -> (kind, label, repeated)
        self.termlists = {}    # variable -> terms so far
        self.handled = 0
        self.walk(parse_block(body), [], None)
        calls = len(re.findall(r"\.allocate_\w+|\.constrain\b", body))
        if calls != self.handled:
            raise FramingError("%s: %d allocation / constraint calls in the text, %d understood" % (where, calls, self.handled))
        if not self.out["transcript"] or not self.out["proof"]:
            raise FramingError("%s: transcript or proof label not found" % where)

    def fail(self, what, s):
        raise FramingError("%s: %s: %r" % (self.where, what, s))

    # loops: [dict(name=None | first label allocated in it, each=(element variable, repeated variable) | None)]
    def walk(self, items, loops, arm):
        for it in items:
            if it[0] == "stmt":
                self.statement(it[1], loops, arm)
                continue
            head, inner = it[1], it[2]
            if head.startswith("for "):
                m = RE_FOR_EACH.fullmatch(head)
                loop = dict(name=None, each=(m.group(2), m.group(3)) if m else None, index=m.group(1) if m else None)
                self.walk(parse_block(inner), loops + [loop], arm)
            elif head.startswith("match "):
                arms = [(kind_of(p), " ".join(b.split()).rstrip(";").strip(), b) for p, b in parse_arms(inner)]
                calls = sum(len(re.findall(r"\.allocate_\w+|\.constrain\b", b)) for _, _, b in arms)
                if not calls:
                    continue
                if not loops:
                    self.fail("a match with allocations or constraints outside a loop", head)
                skip = [k for k, flat, _ in arms if flat == "continue"]
                if any(".constrain" in b for _, _, b in arms):
                    self.constraint_arms(arms, loops)
                else:
                    for k, flat, b in arms:
                        if flat != "continue":
                            self.walk(parse_block(b), loops, dict(skip=skip))
            else:
                if re.search(r"\.allocate_\w+|\.constrain\b", inner):
                    self.fail("an allocation or a constraint under a condition", head)

    def statement(self, s, loops, arm):
        m = RE_TRANSCRIPT.fullmatch(s)
        if m:
            self.transcript_var, self.out["transcript"] = m.group(1), m.group(2)
            return
        m = RE_BUILDER.fullmatch(s)
        if m:
            if m.group(4) != self.transcript_var:
                self.fail("a prover / verifier over another transcript", s)
            self.builder, self.out["proof"] = m.group(1), m.group(3)
            return
        if ".allocate_" in s:
            if s.count(".allocate_") != 1:
                self.fail("several allocations in one statement", s)
            m = RE_LET_ALLOC.fullmatch(s)
            if m:
                var, recv, kind, label = m.group(1) or m.group(2), m.group(3), m.group(4), m.group(5)
                if (m.group(2) is not None) and kind != "point":
                    self.fail("a pair bound to a scalar allocation", s)
                pushed = None
            else:
                m = RE_PUSH_ALLOC.fullmatch(s)
                if not m:
                    self.fail("allocation form not understood", s)
                pushed, recv, kind, label = m.group(1), m.group(2), m.group(3), m.group(4)
                var = None
                if not loops:
                    self.fail("an allocation pushed onto a vector outside a loop", s)
            if recv != self.builder:
                self.fail("an allocation on something that is not the prover / verifier", s)
            self.allocation(kind, label, loops, arm)
            if var:
                self.names[var] = (kind, label, False)
                if loops:
                    loops[-1].setdefault("locals", {})[var] = (kind, label)
            if pushed:
                self.names[pushed] = (kind, label, True)
            return
        if ".constrain" in s:
            m = RE_CONSTRAIN.fullmatch(s)
            if not m or m.group(1) != self.builder or loops:
                self.fail("constraint form not understood", s)
            self.handled += 1
            self.out["constraints"].append(dict(lhs=self.single(m.group(2), "point", s), terms=self.terms(m.group(3), s, None)))
            return
        m = RE_TERMLIST.fullmatch(s)
        if m:
            self.termlists[m.group(1)] = []
            return
        m = RE_PUSH_TERM.fullmatch(s)
        if m and m.group(1) in self.termlists:
            self.termlists[m.group(1)].append([self.single(m.group(2), "scalar", s), self.single(m.group(3), "point", s)])
            return
        m = RE_EXTEND_ZIP.fullmatch(s)
        if m and m.group(1) in self.termlists:
            self.termlists[m.group(1)].append(dict(zip=[self.repeated(m.group(2), "scalar", s), self.repeated(m.group(3), "point", s)]))
            return
        m = RE_PUSH_NAME.fullmatch(s)
        if m and loops and (m.group(2) or m.group(3)) in loops[-1].get("locals", {}):
            kind, label = loops[-1]["locals"][m.group(2) or m.group(3)]
            self.names[m.group(1)] = (kind, label, True)
            return
        if any(v in self.termlists for v in re.findall(ID, s)[:1]) and (".push" in s or ".extend" in s):
            self.fail("a term list built in a way that is not understood", s)

    def allocation(self, kind, label, loops, arm):
        self.handled += 1
        if len(loops) > 1:
            raise FramingError("%s: an allocation in nested loops (%r)" % (self.where, label))
        a = dict(kind=kind, label=label, loop=None)
        if loops:
            if loops[-1]["name"] is None:
                loops[-1]["name"] = label
            a["loop"] = loops[-1]["name"]
            if arm:
                a["skip_kinds"] = arm["skip"]
        self.out["allocations"].append(a)

    def single(self, var, kind, s):
        v = self.names.get(var.lstrip("*"))
        if not v or v[0] != kind or v[2]:
            self.fail("%r is not a single allocated %s" % (var, kind), s)
        return v[1]

    def repeated(self, var, kind, s):
        v = self.names.get(var)
        if not v or v[0] != kind or not v[2]:
            self.fail("%r is not a repeated allocated %s" % (var, kind), s)
        return v[1]

    def terms(self, expr, s, index):
        """`vec![(a, b), ...]` in place, or a term list variable; index: the loop's position variable (then `x[index]` is allowed)"""
        if expr in self.termlists:
            return self.termlists[expr]
        m = re.fullmatch(r"vec!\[(.*)\]", expr)
        if not m:
            self.fail("terms not understood", s)
        out, rest = [], m.group(1).strip()
        while rest:
            t = RE_TERM.match(rest)
            if not t:
                self.fail("term not understood", s)
            side = []
            for var, idx, kind in ((t.group(1), t.group(2), "scalar"), (t.group(3), t.group(4), "point")):
                if idx is None:
                    side.append(self.single(var, kind, s))
                elif index is not None and idx == "[%s]" % index:
                    side.append(dict(at=self.repeated(var, kind, s)))
                else:
                    self.fail("an index that is not the loop's position", s)
            out.append(side)
            rest = rest[t.end():].lstrip()
            if rest.startswith(","):
                rest = rest[1:].lstrip()
            elif rest:
                self.fail("terms not understood", s)
        return out

    def constraint_arms(self, arms, loops):
        if len(loops) != 1 or not loops[-1]["each"]:
            raise FramingError("%s: constraints in a loop that does not walk a repeated label" % self.where)
        elem, vec = loops[-1]["each"]
        entry = dict(each=self.repeated(vec, "point", vec), arms=[])
        for kind, flat, body in arms:
            if flat == "continue":
                entry["arms"].append(dict(kinds=[kind], skip=True))
                continue
            m = RE_CONSTRAIN.fullmatch(flat)
            if not m or m.group(1) != self.builder or m.group(2) != "*" + elem:
                self.fail("constraint arm not understood", flat)
            self.handled += 1
            entry["arms"].append(dict(kinds=[kind], terms=self.terms(m.group(3), flat, loops[-1]["index"])))
        self.out["constraints"].append(entry)


def extract(reference_root=DEFAULT_REFERENCE):
    texts = {}
    for name, rel in SOURCES.items():
        with open(os.path.join(reference_root, rel)) as f:
            texts[name] = f.read()
    return extract_texts(texts)


def extract_texts(texts):
    """texts: {statement: the whole text of its source file}"""
    statements = {}
    for name in SOURCES:
        text = strip_comments(texts[name])
        sides = {side: Side(function_body(text, side), "%s %s" % (name, side)).out for side in SIDES}
        if sides["prove"] != sides["verify"]:
            raise FramingError("%s: prove and verify disagree:\n%s\n%s" % (name, json.dumps(sides["prove"]), json.dumps(sides["verify"])))
        statements[name] = sides
    return dict(_source="tests/gen_framing.py over the reference's src/nizk/{issuance,presentation,encryption}.rs: labels and label names only",
                statements=statements)


def dumps(fixture):
    """JSON with every container that fits a line kept on one line (an allocation, a term list)"""
    def go(v, ind):
        flat = json.dumps(v)
        if not isinstance(v, (dict, list)) or len(flat) + ind <= 120:
            return flat
        pad = " " * (ind + 1)
        if isinstance(v, dict):
            return "{\n" + ",\n".join(pad + json.dumps(k) + ": " + go(x, ind + 1) for k, x in v.items()) + "\n" + " " * ind + "}"
        return "[\n" + ",\n".join(pad + go(x, ind + 1) for x in v) + "\n" + " " * ind + "]"
    return go(fixture, 0) + "\n"


if __name__ == "__main__":
    fx = extract(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_REFERENCE)
    with open(FIXTURE, "w") as f:
        f.write(dumps(fx))
    print("wrote %s: %s" % (FIXTURE, ", ".join("%s %d allocations %d constraints" % (k, len(v["prove"]["allocations"]), len(v["prove"]["constraints"]))
                                              for k, v in fx["statements"].items())))
