"""Presentation tags (include/aeonflux_gpu.h, "Presentation tags"), restated on tests/pyref: the yardstick of tests/test_tag_ref.py,
tests/test_gpu_tagged.py and tests/test_gpu_tagged_forgeries.py.  Every draw is an argument; scalars travel as 32 bytes or ints, points
as their 32-byte encodings.

  scope_generator  H = RistrettoPoint::hash_from_bytes::<Sha512>(scope)
  tag_show         user:   s = m + n, T = s^-1 * H, C' = C_y[p] + n*G_m[p], the tag proof on the presentation's z
  tag_verify       anyone: the tag proof as a zkp Verifier checks it, on the received C_y[p]
"""
import hashlib

from tests.pyref import ristretto as R
from tests.pyref.keccak import Transcript
from tests.pyref.statements import OK, VERIFICATION_FAILURE
from tests.pyref.zkp import ProofError, Prover, Verifier

TRANSCRIPT = b"2019/1416 anonymous credential"
TAG_LABEL = b"2019/1416 presentation tag proof"


class BadScope(ValueError):
    """an H that does not decode or is the identity encoding: the library's AFX_E_BAD_ARGS"""


def scope_generator(scope):
    return R.encode(R.from_uniform_bytes(hashlib.sha512(bytes(scope)).digest()))


def _scope_point(H):
    H = bytes(H)
    P = R.decode(H) if len(H) == 32 else None
    if P is None or H == bytes(32):
        raise BadScope("scope generator")
    return P


def _statement(cs, sp, p, scalar, point, H, T, Cp):
    z = scalar(b"z", "z")
    s = scalar(b"s", "s")
    vGy = point(b"G_y", sp.G_y[p])
    vGm = point(b"G_m", sp.G_m[p])
    vH = point(b"H", H)
    vT = point(b"T", T)
    vCp = point(b"C_y+nG_m", Cp)
    cs.constrain(vCp, [(z, vGy), (s, vGm)])
    cs.constrain(vH, [(s, vT)])


def tag_show(sp, p, H, n, m, z, C_y_p, seed):
    """sp: pyref Params; H, n, C_y_p, seed: 32 bytes each; m, z: ints (the hidden attribute and the presentation's nonce).
    -> (status, dict(T, challenge, responses [z, s], commitments) or None)"""
    Hp = _scope_point(H)
    nn = R.sc_canonical(bytes(n))
    if nn is None:
        return VERIFICATION_FAILURE, None
    s = (m + nn) % R.L
    if s == 0:
        return VERIFICATION_FAILURE, None
    T = R.mul(pow(s, R.L - 2, R.L), Hp)
    Cy = R.decode(bytes(C_y_p))
    assert Cy is not None
    Cp = R.add(Cy, R.mul(nn, sp.G_m[p]))
    if R.encode(T) == bytes(32) or R.encode(Cp) == bytes(32):
        return VERIFICATION_FAILURE, None
    pr = Prover(TAG_LABEL, Transcript(TRANSCRIPT))
    wit = {"z": z % R.L, "s": s}
    _statement(pr, sp, p, lambda label, what: pr.allocate_scalar(label, wit[what]), pr.allocate_point, Hp, T, Cp)
    ch, resp, coms = pr.prove_compact(bytes(seed))
    return OK, dict(T=R.encode(T), challenge=R.sc_bytes(ch), responses=[R.sc_bytes(x) for x in resp], commitments=coms)


def tag_verify(sp, p, H, n, C_y_p, tag):
    """tag: dict(T, challenge, responses [2]) of 32-byte strings -> status"""
    _scope_point(H)
    if p >= sp.n:
        return VERIFICATION_FAILURE
    nn = R.sc_canonical(bytes(n))
    ch = R.sc_canonical(bytes(tag["challenge"]))
    rs = [R.sc_canonical(bytes(x)) for x in tag["responses"]]
    if nn is None or ch is None or len(rs) != 2 or None in rs:
        return VERIFICATION_FAILURE
    Cy = R.decode(bytes(C_y_p))
    if Cy is None:
        return VERIFICATION_FAILURE
    Cp = R.encode(R.add(Cy, R.mul(nn, sp.G_m[p])))
    try:
        ve = Verifier(TAG_LABEL, Transcript(TRANSCRIPT))
        _statement(ve, sp, p, lambda label, what: ve.allocate_scalar(label), lambda label, v: ve.allocate_point(label, v if isinstance(v, bytes) else R.encode(v)),
                   bytes(H), bytes(tag["T"]), Cp)
        ve.verify_compact(ch, rs)
        return OK
    except ProofError:
        return VERIFICATION_FAILURE
