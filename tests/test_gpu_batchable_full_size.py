"""GPU, the headline's full size once: 2^20 C3 presentations shown in batchable form on the GPU, resident in HBM, one item in 2^6
damaged afterwards; the batchable verification must reject exactly the damaged ones, and on a strided sample of 2^12 items the
commitments the GPU's show wrote are the ones the ORACLE recomputes from the compact proof (tests/batchable_ref.py to_batchable)."""
import ctypes as C

import numpy as np
import pytest

from tests import batchable_ref as B
from tests.helpers import DevMem

pytestmark = pytest.mark.gpu


def _oracle_presentation(oracle, shape, pres, i):
    p = oracle.Presentation()
    p.n_attributes, p.n_responses, p.n_hidden_scalars, p.n_enc_proofs = shape.n_attributes, shape.n_responses, shape.n_hidden_scalars, shape.n_enc_proofs
    for k in range(shape.n_attributes):
        p.kinds[k] = shape.kinds[k]
        C.memmove(p.C_y[k], pres["C_y"][k, i].tobytes(), 32)
        C.memmove(p.attr_values[k], pres["attr_values"][k, i].tobytes(), 32)
    for k in range(shape.n_hidden_scalars):
        p.hidden_scalar_indices[k] = shape.hidden_scalar_indices[k]
    C.memmove(p.challenge, pres["challenge"][i].tobytes(), 32)
    for k in range(shape.n_responses):
        C.memmove(p.responses[k], pres["responses"][k, i].tobytes(), 32)
    for f in ("C_x_0", "C_x_1", "C_V"):
        C.memmove(getattr(p, f), pres[f][i].tobytes(), 32)
    for e in range(shape.n_enc_proofs):
        q, d = p.enc[e], pres["enc"][e]
        q.index = shape.enc_indices[e]
        C.memmove(q.challenge, d["challenge"][i].tobytes(), 32)
        for k in range(6):
            C.memmove(q.responses[k], d["responses"][k, i].tobytes(), 32)
        for f in ("pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p"):
            C.memmove(getattr(q, f), d[f][i].tobytes(), 32)
    return p


def test_2_20_c3_presentations_in_batchable_form():
    import oracle
    import aeonflux_amd as afx
    import bench
    from aeonflux_amd import batch
    n, layout, hide, count = 8, "SSPPEEEE", [4, 5, 6, 7], 1 << 20
    params, key, ip = bench.load_fixture("c3_8attrs_SSPPeeee")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    # bench.generate (what tests/test_gpu_full_size.py generates with), its show in batchable form
    stash, orig = [], batch.show

    def show2(ctx, *a, **k):
        pres, cm, shape, st = batch.show_batchable(ctx, *a, **k)
        assert cm["main"].shape[1] == chunk      # (one show per generated chunk: anything else would stack the wrong arrays below)
        stash.append(cm)
        return pres, shape, st
    batch.show = show2
    chunk = 1 << 16
    try:
        parts = [bench.generate(afx, batch, issuer, user, params, n, layout, hide, chunk, 9000 + o) for o in range(0, count, chunk)]
    finally:
        batch.show = orig
    user.close()
    assert len(stash) == len(parts)
    shape = parts[0][1]
    pres = {f: np.concatenate([p[0][f] for p in parts], axis=-2) for f in batch.PRES_FIELDS}
    pres["enc"] = [{f: np.concatenate([p[0]["enc"][e][f] for p in parts], axis=-2) for f in batch.ENC_FIELDS} for e in range(shape.n_enc_proofs)]
    cm = {"main": np.concatenate([c["main"] for c in stash], axis=-2), "enc": [np.concatenate([c["enc"][e] for c in stash], axis=-2) for e in range(shape.n_enc_proofs)]}
    del parts, stash
    assert cm["main"].shape == (6, count, 32)
    # the oracle half on a strided sample of 2^12 honest items: the commitments are the ones its verifier recomputes and hashes
    octx = oracle.Ctx(params, key, ip)
    sample = (np.arange(1 << 12, dtype=np.int64) * (count >> 12) + 3) % count
    for i in sample:
        p = _oracle_presentation(oracle, shape, pres, int(i))
        ref = B.to_batchable(octx, p)
        assert ref is not None and ref["main"] == [cm["main"][j, i].tobytes() for j in range(6)], int(i)
        assert ref["enc"] == [[cm["enc"][e][j, i].tobytes() for j in range(5)] for e in range(shape.n_enc_proofs)], int(i)
    # one item in 2^6 damaged, the kind by turns
    want = np.zeros(count, np.uint8)
    for t, i in enumerate(range(17, count, 64)):
        kind = t % 6
        if kind == 0:
            cm["main"][t % 6, i, 5] ^= 0x08
        elif kind == 1:
            cm["enc"][t % 4][t % 5, i, 9] ^= 0x01
        elif kind == 2:
            cm["main"][1, i, :] = 0
        elif kind == 3:
            pres["responses"][1, i, 2] ^= 0x20
        elif kind == 4:
            pres["C_V"][i, 7] ^= 0x01
        else:
            pres["enc"][2]["responses"][4, i, 0] ^= 0x02
        want[i] = 1
    # device-resident
    dev, keep = {}, []

    def up(a):
        m = DevMem(a)
        keep.append(m)
        return m.ptr
    dpres = {f: up(pres[f]) for f in batch.PRES_FIELDS if f != "challenge"}
    dpres["challenge"] = 0
    dpres["enc"] = [{f: (up(d[f]) if f != "challenge" else 0) for f in batch.ENC_FIELDS} for d in pres["enc"]]
    dcm = {"main": up(cm["main"]), "enc": [up(a) for a in cm["enc"]]}
    soa, k1 = batch.presentation_soa(dpres, ptr=lambda x: x)
    csoa, k2 = batch.commitments_soa(dcm, ptr=lambda x: x)
    status = DevMem(nbytes=count, fill=255)
    rng = batch.device_rng(bytes(range(32)), 1)
    afx.check(afx.lib().afx_verify_presentations_batchable_dev(issuer.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), count, status.ptr))
    issuer.synchronize()
    got = status.numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert want.sum() == count // 64
    # the compact form of the same arrays rejects the damaged items that are damaged in a field it reads, and no other
    compact = batch.verify_presentations(issuer, shape, pres)
    reads = np.array([t % 6 >= 3 for t in range(count // 64)])
    assert np.array_equal(compact[17::64].astype(bool), reads) and compact.sum() == reads.sum()
    issuer.close()
