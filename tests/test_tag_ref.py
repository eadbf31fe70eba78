"""CPU-only: the presentation-tag yardstick (tests/tag_ref.py) against itself.  Honest tags verify; (m + n)*T == H; T depends on (m, n, H)
alone - not on z, C_y's blinding or the proof's seed; another counter or scope gives another T; and every single damage of a tag is
rejected: a bit of T, n + 1, the non-canonical n + l, each response, the challenge, T = the identity encoding, another item's tag, and the
aliases that leave every value intact: a response or the challenge + l, T or C_y[p] with bit 255 set or as p - s.
m + n == 0 (mod l) is refused by the prover."""
import hashlib

import pytest

from tests import tag_ref as TR
from tests.pyref import ristretto as R
from tests.pyref import statements as S

L = R.L


@pytest.fixture(scope="module")
def world():
    import oracle
    n = 3
    params, _ = oracle.system_parameters_generate(n, hashlib.shake_256(b"tag-ref params").digest(1 << 16))
    sp = S.Params(params)
    xof = hashlib.shake_256(b"tag-ref draws").digest(4096)
    pos = [0]

    def take(k):
        b = xof[pos[0]:pos[0] + k]
        pos[0] += k
        return b
    return dict(sp=sp, take=take, H=TR.scope_generator(b"scope A"), H2=TR.scope_generator(b"scope B"))


def commit(sp, p, m, z):
    return R.encode(R.add(R.mul(z, sp.G_y[p]), R.mul(m, sp.G_m[p])))


def make_item(w, p, m, n, H=None):
    sp, take = w["sp"], w["take"]
    z = R.sc_from_wide(take(64))
    Cy = commit(sp, p, m, z)
    seed = take(32)
    nb = n.to_bytes(32, "little")
    st, tag = TR.tag_show(sp, p, H or w["H"], nb, m, z, Cy, seed)
    return dict(p=p, m=m, n=n, nb=nb, z=z, Cy=Cy, st=st, tag=tag, H=H or w["H"])


def verify(w, it, **over):
    tag = dict(it["tag"])
    nb = over.pop("nb", it["nb"])
    Cy = over.pop("Cy", it["Cy"])
    H = over.pop("H", it["H"])
    tag.update(over)
    return TR.tag_verify(w["sp"], it["p"], H, nb, Cy, tag)


def test_scope_generator_is_hash_from_bytes():
    H = TR.scope_generator(b"")
    assert H == R.encode(R.from_uniform_bytes(hashlib.sha512(b"").digest())) and R.decode(H) is not None and H != bytes(32)
    assert TR.scope_generator(b"a") != TR.scope_generator(b"b")


@pytest.mark.parametrize("p", [0, 1, 2])
def test_honest_tags_verify_and_open_to_H(world, p):
    m = R.sc_from_wide(world["take"](64))
    for n in (0, 1, 7, 2 ** 32 - 1, (1 - m) % L, (L - 1 - m) % L):
        it = make_item(world, p, m, n)
        assert it["st"] == S.OK
        assert verify(world, it) == S.OK
        assert R.encode(R.mul((m + n) % L, R.decode(it["tag"]["T"]))) == world["H"]
    it = make_item(world, p, m, (L - 1 - m) % L)          # s = l - 1: T = -H
    assert it["tag"]["T"] == R.encode(R.neg(R.decode(world["H"])))
    it = make_item(world, p, m, (1 - m) % L)              # s = 1: T = H
    assert it["tag"]["T"] == world["H"]


def test_T_is_a_function_of_attribute_counter_and_scope_alone(world):
    m = R.sc_from_wide(world["take"](64))
    a, b = make_item(world, 1, m, 5), make_item(world, 1, m, 5)      # fresh z and seed
    assert a["z"] != b["z"] and a["Cy"] != b["Cy"]
    assert a["tag"]["T"] == b["tag"]["T"]
    assert a["tag"]["challenge"] != b["tag"]["challenge"] and a["tag"]["responses"] != b["tag"]["responses"]
    assert make_item(world, 1, m, 6)["tag"]["T"] != a["tag"]["T"]
    assert make_item(world, 1, m, 5, H=world["H2"])["tag"]["T"] != a["tag"]["T"]
    assert make_item(world, 1, (m + 1) % L, 5)["tag"]["T"] != a["tag"]["T"]


def test_every_single_damage_fails(world):
    m = R.sc_from_wide(world["take"](64))
    it, other = make_item(world, 2, m, 9), make_item(world, 2, R.sc_from_wide(world["take"](64)), 9)
    assert verify(world, it) == S.OK and verify(world, other) == S.OK
    flip = lambda b, bit=0: bytes([b[0] ^ (1 << bit)]) + b[1:]
    plus = lambda b, k: (int.from_bytes(b, "little") + k).to_bytes(32, "little")
    P = 2 ** 255 - 19
    T = it["tag"]["T"]
    damages = {
        "a bit of T": dict(T=flip(T, 1)),
        "n + 1": dict(nb=(it["n"] + 1).to_bytes(32, "little")),
        "n + l": dict(nb=(it["n"] + L).to_bytes(32, "little")),
        "response z": dict(responses=[flip(it["tag"]["responses"][0]), it["tag"]["responses"][1]]),
        "response s": dict(responses=[it["tag"]["responses"][0], flip(it["tag"]["responses"][1])]),
        "response s + l": dict(responses=[it["tag"]["responses"][0], (int.from_bytes(it["tag"]["responses"][1], "little") + L).to_bytes(32, "little")]),
        "challenge": dict(challenge=flip(it["tag"]["challenge"])),
        "T = identity encoding": dict(T=bytes(32)),
        "T that does not decode": dict(T=b"\xff" * 32),
        "another scope": dict(H=world["H2"]),
        "another item's C_y": dict(Cy=other["Cy"]),
        "another item's tag": dict(other["tag"]),
        # the same values in another encoding: only a canonicity check (scalars) or the decoder's own checks (points) refuse these
        "response z + l": dict(responses=[plus(it["tag"]["responses"][0], L), it["tag"]["responses"][1]]),
        "challenge + l": dict(challenge=plus(it["tag"]["challenge"], L)),
        "T with bit 255": dict(T=plus(T, 2 ** 255)),
        "T as p - s": dict(T=(P - int.from_bytes(T, "little")).to_bytes(32, "little")),
        "C_y[p] + l": dict(Cy=plus(it["Cy"], L)),
        "C_y[p] with bit 255": dict(Cy=plus(it["Cy"], 2 ** 255)),
        "C_y[p] as p - s": dict(Cy=(P - int.from_bytes(it["Cy"], "little")).to_bytes(32, "little")),
    }
    for name, over in damages.items():
        over.pop("commitments", None)
        assert verify(world, it, **over) == S.VERIFICATION_FAILURE, name


def test_the_prover_refuses_a_zero_sum_and_a_non_canonical_counter(world):
    sp = world["sp"]
    m = R.sc_from_wide(world["take"](64))
    z = R.sc_from_wide(world["take"](64))
    Cy = commit(sp, 0, m, z)
    st, tag = TR.tag_show(sp, 0, world["H"], ((L - m) % L).to_bytes(32, "little"), m, z, Cy, bytes(32))
    assert st == S.VERIFICATION_FAILURE and tag is None
    st, tag = TR.tag_show(sp, 0, world["H"], (L + 3).to_bytes(32, "little"), m, z, Cy, bytes(32))
    assert st == S.VERIFICATION_FAILURE and tag is None
    st, tag = TR.tag_show(sp, 0, world["H"], (L - 1).to_bytes(32, "little"), 1, z, commit(sp, 0, 1, z), bytes(32))     # m = 1, n = l - 1
    assert st == S.VERIFICATION_FAILURE


def test_a_bad_scope_generator_is_refused(world):
    sp = world["sp"]
    for H in (bytes(32), b"\xff" * 32):
        with pytest.raises(TR.BadScope):
            TR.tag_show(sp, 0, H, bytes(32), 1, 1, commit(sp, 0, 1, 1), bytes(32))
        with pytest.raises(TR.BadScope):
            TR.tag_verify(sp, 0, H, bytes(32), commit(sp, 0, 1, 1), dict(T=world["H"], challenge=bytes(32), responses=[bytes(32), bytes(32)]))
