"""Blind issuance (include/aeonflux_gpu.h, "Blind issuance"), restated on tests/pyref: the yardstick of tests/test_blind_ref.py,
tests/test_gpu_blind.py.  Every draw is an argument; scalars travel as 32 bytes, points as their 32-byte encodings.

  blind_request   user:   D = d*G, (A_j, B_j) = (r_j*G, r_j*D + M_i) for every hidden position i, the request proof
  verify_request  anyone: the request proof as a zkp Verifier checks it
  blind_issue     issuer: t, U, S1, S2 and the blind issuance proof - the hidden positions' values are never read
  unblind         user:   the issuance proof, then V = S2 - d*S1
"""
from tests.pyref import ristretto as R
from tests.pyref.keccak import Transcript
from tests.pyref.statements import (OK, VERIFICATION_FAILURE, MAC_CREATION, PUBLIC_SCALAR, SECRET_SCALAR, SECRET_POINT, Params, Key,
                                    _issuer_params)
from tests.pyref.zkp import ProofError, Prover, Verifier

TRANSCRIPT = b"2019/1416 anonymous credential"
REQUEST_LABEL = b"2019/1416 blind request proof"
ISSUANCE_LABEL = b"2019/1416 blind issuance proof"


def hidden_positions(kinds):
    return [i for i, k in enumerate(kinds) if k in (SECRET_SCALAR, SECRET_POINT)]


def n_request_responses(kinds):
    return 1 + len(hidden_positions(kinds)) + sum(1 for k in kinds if k == SECRET_SCALAR)


def _is_scalar(k):
    return k in (PUBLIC_SCALAR, SECRET_SCALAR)


def _request_statement(cs, sp, kinds, scalar, point, D, A, B):
    """allocation order and constraints of the request proof; scalar(label, j, what) / point(label, value) allocate"""
    H = hidden_positions(kinds)
    d = scalar(b"d", None, "d")
    r, m = [], {}
    for j, i in enumerate(H):
        r.append(scalar(b"r", j, "r"))
        if kinds[i] == SECRET_SCALAR:
            m[j] = scalar(b"m", j, "m")
    vG = point(b"G", sp.G)
    vD = point(b"D", D)
    vA, vB, vGm = [], [], {}
    for j, i in enumerate(H):
        vA.append(point(b"A", A[j]))
        vB.append(point(b"B", B[j]))
        if kinds[i] == SECRET_SCALAR:
            vGm[j] = point(b"G_m", sp.G_m[i])
    cs.constrain(vD, [(d, vG)])
    for j, i in enumerate(H):
        cs.constrain(vA[j], [(r[j], vG)])
        if kinds[i] == SECRET_SCALAR:
            cs.constrain(vB[j], [(r[j], vD), (m[j], vGm[j])])


def blind_request(params, kinds, values, d, r_wide, seed):
    """values: 32 bytes per position (all n of them are checked); r_wide: 64 bytes per hidden position.  (status, request)"""
    sp = Params(params)
    if len(kinds) != sp.n or any(k > SECRET_POINT for k in kinds):
        return MAC_CREATION, None
    dd = R.sc_canonical(d)
    if dd is None:
        return MAC_CREATION, None
    M, ms = [], []
    for i, k in enumerate(kinds):
        if _is_scalar(k):
            m = R.sc_canonical(values[i][:32])
            if m is None:
                return MAC_CREATION, None
            ms.append(m)
            M.append(R.mul(m, sp.G_m[i]))
        else:
            p = R.decode(values[i][:32])
            if p is None:
                return MAC_CREATION, None
            ms.append(None)
            M.append(p)
    H = hidden_positions(kinds)
    rs = [R.sc_from_wide(w) for w in r_wide]
    assert len(rs) == len(H)
    D = R.mul(dd, sp.G)
    A = [R.mul(r, sp.G) for r in rs]
    B = [R.add(R.mul(r, D), M[i]) for r, i in zip(rs, H)]
    if any(R.encode(P) == bytes(32) for P in [D] + A + B):
        return MAC_CREATION, None
    pr = Prover(REQUEST_LABEL, Transcript(TRANSCRIPT))
    wit = {"d": lambda j: dd, "r": lambda j: rs[j], "m": lambda j: ms[H[j]]}
    _request_statement(pr, sp, kinds, lambda label, j, what: pr.allocate_scalar(label, wit[what](j)), pr.allocate_point, D, A, B)
    ch, resp, coms = pr.prove_compact(seed)
    return OK, dict(D=R.encode(D), A=[R.encode(P) for P in A], B=[R.encode(P) for P in B], challenge=R.sc_bytes(ch),
                    responses=[R.sc_bytes(x) for x in resp], commitments=coms)


def _verify_request(sp, kinds, req):
    """raises ProofError; returns the decoded (D, A, B)"""
    H = hidden_positions(kinds)
    if len(req["A"]) != len(H) or len(req["B"]) != len(H) or len(req["responses"]) != n_request_responses(kinds):
        raise ProofError("wrong shape")
    ch = R.sc_canonical(req["challenge"])
    rs = [R.sc_canonical(x) for x in req["responses"]]
    if ch is None or None in rs:
        raise ProofError("malformed")
    ve = Verifier(REQUEST_LABEL, Transcript(TRANSCRIPT))
    _request_statement(ve, sp, kinds, lambda label, j, what: ve.allocate_scalar(label),
                       lambda label, v: ve.allocate_point(label, v if isinstance(v, bytes) else R.encode(v)), req["D"], req["A"], req["B"])
    ve.verify_compact(ch, rs)
    return R.decode(req["D"]), [R.decode(x) for x in req["A"]], [R.decode(x) for x in req["B"]]


def verify_request(params, kinds, req):
    sp = Params(params)
    if len(kinds) != sp.n or any(k > SECRET_POINT for k in kinds):
        return VERIFICATION_FAILURE
    try:
        _verify_request(sp, kinds, req)
        return OK
    except ProofError:
        return VERIFICATION_FAILURE


def _issuance_statement(cs, sp, kinds, C_W, I, scalar, point, U, tU, D, S1, S2, AB, M):
    """the blind issuance proof: the issuance proof's own allocations without V, then G, D, S1, S2 and per position A, B or M"""
    n = sp.n
    H = hidden_positions(kinds)
    w = scalar(b"w", "w")
    w_prime = scalar(b"w'", "w'")
    x_0 = scalar(b"x_0", "x_0")
    x_1 = scalar(b"x_1", "x_1")
    y = [scalar(b"y", i) for i in range(n)]
    one = scalar(b"1", "1")
    rp = scalar(b"r'", "r'")
    G_V = point(b"G_V", sp.G_V)
    G_w = point(b"G_w", sp.G_w)
    G_w_prime = point(b"G_w_prime", sp.G_w_prime)
    nGx0 = point(b"-G_x_0", R.neg(sp.G_x_0))
    nGx1 = point(b"-G_x_1", R.neg(sp.G_x_1))
    nGy = [point(b"-G_y", R.neg(g)) for g in sp.G_y]
    vC_W = point(b"C_W", C_W)
    vI = point(b"I", I)
    vU = point(b"U", U)
    vtU = point(b"tU", tU)
    vG = point(b"G", sp.G)
    vD = point(b"D", D)
    vS1 = point(b"S1", S1)
    vS2 = point(b"S2", S2)
    vA, last = {}, {}
    for i in range(n):
        if i in H:
            j = H.index(i)
            vA[i] = point(b"A", AB[0][j])
            last[i] = point(b"B", AB[1][j])
        else:
            last[i] = point(b"M", M[i])
    cs.constrain(vC_W, [(w, G_w), (w_prime, G_w_prime)])
    cs.constrain(vI, [(one, G_V), (x_0, nGx0), (x_1, nGx1)] + list(zip(y, nGy)))
    cs.constrain(vS1, [(rp, vG)] + [(y[i], vA[i]) for i in H])
    cs.constrain(vS2, [(w, G_w), (x_0, vU), (x_1, vtU), (rp, vD)] + [(y[i], last[i]) for i in range(n)])


def _revealed_messages(sp, kinds, values):
    """M_i of the revealed positions (None at hidden ones, whose values are never read); None for a malformed value"""
    H = hidden_positions(kinds)
    out = []
    for i, k in enumerate(kinds):
        if i in H:
            out.append(None)
        elif _is_scalar(k):
            m = R.sc_canonical(values[i][:32])
            if m is None:
                return None
            out.append(R.mul(m, sp.G_m[i]))
        else:
            p = R.decode(values[i][:32])
            if p is None:
                return None
            out.append(p)
    return out


def blind_issue(params, key, ip, kinds, values, req, t_wide, U_wide, rprime_wide, seed):
    """values[i] of a hidden position is never read (pass None).  (status, issuance)"""
    sp, sk = Params(params), Key(key)
    C_W, I = _issuer_params(ip)
    if len(kinds) != sp.n or any(k > SECRET_POINT for k in kinds):
        return MAC_CREATION, None
    try:
        D, A, B = _verify_request(sp, kinds, req)
    except ProofError:
        return VERIFICATION_FAILURE, None
    M = _revealed_messages(sp, kinds, values)
    if M is None:
        return VERIFICATION_FAILURE, None
    H = hidden_positions(kinds)
    t = R.sc_from_wide(t_wide)
    U = R.from_uniform_bytes(U_wide)
    rp = R.sc_from_wide(rprime_wide)
    Vp = R.add(R.add(sk.W, R.mul(sk.x_0, U)), R.mul(sk.x_1 * t, U))
    for i in range(sp.n):
        if i not in H:
            Vp = R.add(Vp, R.mul(sk.y[i], M[i]))
    S1 = R.mul(rp, sp.G)
    S2 = R.add(R.mul(rp, D), Vp)
    for j, i in enumerate(H):
        S1 = R.add(S1, R.mul(sk.y[i], A[j]))
        S2 = R.add(S2, R.mul(sk.y[i], B[j]))
    tU = R.mul(t, U)
    pr = Prover(ISSUANCE_LABEL, Transcript(TRANSCRIPT))
    wit = {"w": sk.w, "w'": sk.w_prime, "x_0": sk.x_0, "x_1": sk.x_1, "1": 1, "r'": rp}
    _issuance_statement(pr, sp, kinds, C_W, I, lambda label, what: pr.allocate_scalar(label, sk.y[what] if isinstance(what, int) else wit[what]),
                        pr.allocate_point, U, tU, D, S1, S2, (A, B), M)
    ch, resp, coms = pr.prove_compact(seed)
    return OK, dict(t=R.sc_bytes(t), U=R.encode(U), S1=R.encode(S1), S2=R.encode(S2), challenge=R.sc_bytes(ch),
                    responses=[R.sc_bytes(x) for x in resp], commitments=coms)


def unblind(params, ip, kinds, values, req, d, iss):
    """the user's side of the issuance: (status, V).  req: the user's own request (D, A, B are read)"""
    sp = Params(params)
    C_W, I = _issuer_params(ip)
    if len(kinds) != sp.n or any(k > SECRET_POINT for k in kinds) or len(iss["responses"]) != sp.n + 6:
        return VERIFICATION_FAILURE, None
    H = hidden_positions(kinds)
    try:
        dd, t, ch = R.sc_canonical(d), R.sc_canonical(iss["t"]), R.sc_canonical(iss["challenge"])
        rs = [R.sc_canonical(x) for x in iss["responses"]]
        U, S1, S2 = R.decode(iss["U"]), R.decode(iss["S1"]), R.decode(iss["S2"])
        D, A, B = R.decode(req["D"]), [R.decode(x) for x in req["A"]], [R.decode(x) for x in req["B"]]
        M = _revealed_messages(sp, kinds, values)
        if None in (dd, t, ch, U, S1, S2, D, M) or None in rs or None in A or None in B or len(A) != len(H) or len(B) != len(H):
            raise ProofError("malformed")
        ve = Verifier(ISSUANCE_LABEL, Transcript(TRANSCRIPT))
        _issuance_statement(ve, sp, kinds, C_W, I, lambda label, what: ve.allocate_scalar(label),
                            lambda label, P: ve.allocate_point(label, R.encode(P)), U, R.mul(t, U), D, S1, S2, (A, B), M)
        ve.verify_compact(ch, rs)
        return OK, R.encode(R.sub(S2, R.mul(dd, S1)))
    except ProofError:
        return VERIFICATION_FAILURE, None
