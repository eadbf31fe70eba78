"""CPU yardsticks for the batchable form of a presentation (include/aeonflux_gpu.h "Batchable presentation proofs"): every
`challenge` replaced by the proof's commitments.

  to_batchable(issuer, p)        the ORACLE's commitments of an honest compact presentation (oracle.debug_last: what its verifier
                                 recomputed and hashed), main proof and each proof of encryption apart;
  ref_verify_batchable(...)      rules 1-3 of the header in pure Python on tests/pyref, PER CONSTRAINT and WITHOUT weights: the received
                                 commitments go into the transcript, the challenge comes out, and every constraint is compared as a
                                 group element.  The statements are not copied: pyref's own verify_presentation runs with its Verifier
                                 swapped for one whose verify_compact takes commitments;
  weights(seed, stream, i, m)    the engine's weight draw restated with hashlib.

A batchable presentation here is a pair (p, cm): p a pyref presentation dict (its challenge fields are ignored), cm =
dict(main=[32-byte R_j ...], enc=[[5 x R_j] per proof of encryption]).
"""
import contextlib
import hashlib

from tests.pyref import ristretto as R
from tests.pyref import statements as S
from tests.pyref import zkp

DRAW_BATCH_WEIGHTS = 64


def pyref_presentation(p):
    """oracle.Presentation -> the dict tests/pyref/statements.verify_presentation takes"""
    b = bytes
    return dict(kinds=[p.kinds[i] for i in range(p.n_attributes)], attr_values=[b(p.attr_values[i]) for i in range(p.n_attributes)],
                hidden_scalar_indices=[p.hidden_scalar_indices[i] for i in range(p.n_hidden_scalars)], challenge=b(p.challenge),
                responses=[b(p.responses[k]) for k in range(p.n_responses)], C_x_0=b(p.C_x_0), C_x_1=b(p.C_x_1), C_V=b(p.C_V),
                C_y=[b(p.C_y[i]) for i in range(p.n_attributes)],
                enc=[dict(index=p.enc[e].index, challenge=b(p.enc[e].challenge), responses=[b(p.enc[e].responses[k]) for k in range(6)],
                          **{f: b(getattr(p.enc[e], f)) for f in ("pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p")}) for e in range(p.n_enc_proofs)])


def to_batchable(issuer, p):
    """the oracle's commitments for a compact presentation p (oracle.Presentation): dict(main, enc), or None when its main proof or
    one of its proofs of encryption does not reach the transcript (nothing to take the commitments from)"""
    import oracle
    q = oracle.Presentation.from_buffer_copy(bytes(p))
    q.n_enc_proofs = 0                                   # the main proof alone
    oracle.debug_reset()
    issuer.verify_presentation(q)
    main, _ = oracle.debug_last()
    if not main:
        return None
    enc = []
    for e in range(p.n_enc_proofs):
        oracle.debug_reset()
        issuer.verify_encryption_proof(p.enc[e])
        c, _ = oracle.debug_last()
        if not c:
            return None
        enc.append(c)
    return dict(main=main, enc=enc)


class _BatchableVerifier(zkp.Verifier):
    """zkp's Verifier::verify_batchable, constraint by constraint: `queue` holds the received commitment lists in the order the
    statement verifies its proofs; `trace` receives each proof's challenge (as 32 bytes)"""
    queue, trace = None, None

    def verify_compact(self, challenge_ignored, responses):
        coms = type(self).queue.pop(0)
        if len(responses) != self.n_scalars:
            raise zkp.ProofError("wrong number of responses")
        if len(coms) != len(self.constraints):
            raise zkp.ProofError("wrong number of commitments")
        pts = []
        for enc in self.points:
            p = R.decode(enc)
            if p is None:
                raise zkp.ProofError("point does not decompress")
            pts.append(p)
        for (lhs, _), enc in zip(self.constraints, coms):
            if enc == bytes(32) or R.decode(enc) is None:
                raise zkp.ProofError("identity or undecodable commitment")       # validate_and_append_blinding_commitment
            zkp._append_point(self.t, b"blindcom", self.labels[lhs], enc)
        c = zkp._challenge(self.t)
        type(self).trace.append(R.sc_bytes(c))
        for (lhs, terms), enc in zip(self.constraints, coms):
            want = R.msm([responses[s] for s, _ in terms] + [(-c) % R.L], [pts[p] for _, p in terms] + [pts[lhs]])
            if R.encode(want) != enc:
                raise zkp.ProofError("constraint does not hold")
        return list(coms)


@contextlib.contextmanager
def _batchable_statements(queue, trace):
    saved = S.Verifier
    _BatchableVerifier.queue, _BatchableVerifier.trace = queue, trace
    S.Verifier = _BatchableVerifier
    try:
        yield
    finally:
        S.Verifier = saved


def ref_verify_batchable(params, key, ip, p, cm, strict=False, trace=None):
    """status (0 accepted, 1 rejected) of the batchable presentation (p, cm); `trace` (a list) receives the challenges of the proofs
    that reach their transcript's end, main proof first"""
    q = dict(p, challenge=bytes(32), enc=[dict(e, challenge=bytes(32)) for e in p["enc"]])
    queue = [list(cm["main"])] + [list(c) for c in cm["enc"]]
    if len(cm["enc"]) != len(p["enc"]):
        return S.VERIFICATION_FAILURE
    with _batchable_statements(queue, trace if trace is not None else []):
        st, _ = S.verify_presentation(params, key, ip, q, strict=strict)
    return st


def weights(seed, stream, index, m, label=DRAW_BATCH_WEIGHTS):
    """the m 128-bit weights of item `index`: draw(seed, stream, index, label) squeezed to 16 m bytes, little-endian integers"""
    d = hashlib.shake_256(b"aeonflux-amd/device-rng/v1" + bytes(seed) + stream.to_bytes(8, "little") + index.to_bytes(8, "little") + bytes([label])).digest(16 * m)
    return [int.from_bytes(d[16 * w:16 * w + 16], "little") for w in range(m)]


def arrays_of(cms):
    """a list of per-item commitment dicts -> the column arrays the engine takes: dict(main [n_main,count,32], enc [[5,count,32]...])"""
    import numpy as np
    col = lambda rows: np.stack([np.stack([np.frombuffer(r, np.uint8) for r in item]) for item in rows], axis=1).copy()
    return dict(main=col([c["main"] for c in cms]), enc=[col([c["enc"][e] for c in cms]) for e in range(len(cms[0]["enc"]))])
