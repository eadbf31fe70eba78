"""Batch front end over the C ABI with numpy arrays (host pointers) — the Python mirror of the reference's
`Issuer::issue`, `CredentialIssuance::verify`, `AnonymousCredential::show`, `Issuer::verify` for whole batches.

Layout convention everywhere: a field of a batch is a uint8 array of shape [count, 32]; a repeated field is
[k, count, 32] (k-major), exactly the struct-of-arrays layout of include/aeonflux_gpu.h.
"""
import ctypes as C

import numpy as np

from . import (AttributesSoA, BlindIssuanceSoA, BlindIssueRandomness, BlindRequestRandomness, BlindRequestSoA, CommitmentsSoA, CredentialsSoA, DeviceRng, EncProofOut, EncProofSoA, IssuanceGroup, IssuanceSoA, IssueGroup, IssueRandomness, KeypairsSoA,
               PresentationOut, PresentationSoA, Shape, ShowGroup, ShowRandomness, TagsOut, TagsSoA, TagStatement, check, lib)

ENC_FIELDS = ("challenge", "responses", "pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p")
PRES_FIELDS = ("challenge", "responses", "C_x_0", "C_x_1", "C_V", "C_y", "attr_values")


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


def _attrs(kinds, values):
    s = AttributesSoA()
    s.n_attributes = len(kinds)
    for i, k in enumerate(kinds):
        s.kinds[i] = k
    s.values = values.ctypes.data
    return s


def _issue_args(n_ctx, kinds, values, t_wide, U_wide, rng_seed):
    """(AttributesSoA, IssueRandomness, IssuanceSoA, output dict, count, keepalive) of one layout's requests"""
    values, t_wide, U_wide, rng_seed = map(_u8, (values, t_wide, U_wide, rng_seed))
    cnt = t_wide.shape[0]
    req = _attrs(kinds, values)
    rnd = IssueRandomness(t_wide.ctypes.data, U_wide.ctypes.data, rng_seed.ctypes.data)
    o = {k: np.zeros((cnt, 32), np.uint8) for k in ("t", "U", "V", "challenge")}
    o["responses"] = np.zeros((n_ctx + 5, cnt, 32), np.uint8)
    out = IssuanceSoA(*(o[k].ctypes.data for k in ("t", "U", "V", "challenge", "responses")))
    return req, rnd, out, o, cnt, (values, t_wide, U_wide, rng_seed)


def issue(ctx, kinds, values, t_wide, U_wide, rng_seed, first=None, n=None):
    """Issuer::issue over a batch.  values [n,count,32], t_wide/U_wide [count,64], rng_seed [count,32].
    Returns (dict(t,U,V,challenge,responses[n+5,count,32]), status[count]).  ctx may be a Group (all its GPUs); with
    first/n only that range of the batch is issued (afx_issue_range; the other output rows stay zero / status 255)."""
    req, rnd, out, o, cnt, keep = _issue_args(ctx.n, kinds, values, t_wide, U_wide, rng_seed)
    status = np.full(cnt, 255, np.uint8)
    if first is not None:
        check(lib().afx_issue_range(ctx.h, C.byref(req), C.byref(rnd), cnt, first, n, C.byref(out), status.ctypes.data))
    elif hasattr(ctx, "member"):
        check(lib().afx_group_issue(ctx.h, C.byref(req), C.byref(rnd), cnt, C.byref(out), status.ctypes.data))
    else:
        check(lib().afx_issue(ctx.h, C.byref(req), C.byref(rnd), cnt, C.byref(out), status.ctypes.data))
    return o, status


def _positions(items, total=None):
    """per group: its items' places in the caller's order.  An item may carry "positions"; otherwise the groups are contiguous."""
    out, nxt = [], 0
    for it, cnt in items:
        pos = np.ascontiguousarray(it["positions"], dtype=np.uint64) if it.get("positions") is not None else np.arange(nxt, nxt + cnt, dtype=np.uint64)
        assert pos.size == cnt
        out.append(pos)
        nxt += cnt
    return out, nxt


def issue_mixed(ctx, items):
    """Issuer::issue over requests of DIFFERENT attribute layouts in one call (afx_issue_mixed / afx_group_issue_mixed).
    items = [dict(kinds, values [n,count,32], t_wide, U_wide, rng_seed, positions=None)], one per layout group (layouts may
    repeat).  Returns ([output dict per group], status in the caller's order)."""
    arr = (IssueGroup * max(1, len(items)))()
    keep, outs, counts = [], [], []
    for g, it in enumerate(items):
        req, rnd, out, o, cnt, k = _issue_args(ctx.n, it["kinds"], it["values"], it["t_wide"], it["U_wide"], it["rng_seed"])
        arr[g].requests, arr[g].rnd, arr[g].out, arr[g].count = req, rnd, out, cnt
        keep.append(k)
        outs.append(o)
        counts.append(cnt)
    pos, total = _positions(list(zip(items, counts)))
    total = max([total] + [int(p.max()) + 1 for p in pos if p.size])
    for g, p in enumerate(pos):
        arr[g].positions = p.ctypes.data_as(C.POINTER(C.c_uint64))
    status = np.full(total, 255, np.uint8)
    fn = lib().afx_group_issue_mixed if hasattr(ctx, "member") else lib().afx_issue_mixed
    check(fn(ctx.h, arr, len(items), status.ctypes.data, total))
    return outs, status


def _issuance_args(kinds, values, issuance, n_responses=None):
    values = _u8(values)
    iss = {k: _u8(issuance[k]) for k in ("t", "U", "V", "challenge", "responses")}
    cnt = iss["t"].shape[0]
    req = _attrs(kinds, values)
    s = IssuanceSoA(*(iss[k].ctypes.data for k in ("t", "U", "V", "challenge", "responses")))
    nr = iss["responses"].shape[0] if n_responses is None else n_responses
    return req, s, nr, cnt, (values, iss)


def verify_issuances(ctx, kinds, values, issuance, n_responses=None, first=None, n=None):
    """CredentialIssuance::verify over a batch; issuance = dict as returned by issue().  ctx may be a Group; with first/n only
    that range is verified (afx_verify_issuances_range; the other status bytes stay 255)."""
    req, s, nr, cnt, keep = _issuance_args(kinds, values, issuance, n_responses)
    status = np.full(cnt, 255, np.uint8)
    if first is not None:
        check(lib().afx_verify_issuances_range(ctx.h, C.byref(req), C.byref(s), nr, cnt, first, n, status.ctypes.data))
    elif hasattr(ctx, "member"):
        check(lib().afx_group_verify_issuances(ctx.h, C.byref(req), C.byref(s), nr, cnt, status.ctypes.data))
    else:
        check(lib().afx_verify_issuances(ctx.h, C.byref(req), C.byref(s), nr, cnt, status.ctypes.data))
    return status


def verify_issuances_mixed(ctx, items):
    """CredentialIssuance::verify over issuances of DIFFERENT layouts in one call.  items = [dict(kinds, values, issuance,
    n_responses=None, positions=None)].  Returns the statuses in the caller's order."""
    arr = (IssuanceGroup * max(1, len(items)))()
    keep, counts = [], []
    for g, it in enumerate(items):
        req, s, nr, cnt, k = _issuance_args(it["kinds"], it["values"], it["issuance"], it.get("n_responses"))
        arr[g].attrs, arr[g].issuances, arr[g].n_responses, arr[g].count = req, s, nr, cnt
        keep.append(k)
        counts.append(cnt)
    pos, total = _positions(list(zip(items, counts)))
    total = max([total] + [int(p.max()) + 1 for p in pos if p.size])
    for g, p in enumerate(pos):
        arr[g].positions = p.ctypes.data_as(C.POINTER(C.c_uint64))
    status = np.full(total, 255, np.uint8)
    fn = lib().afx_group_verify_issuances_mixed if hasattr(ctx, "member") else lib().afx_verify_issuances_mixed
    check(fn(ctx.h, arr, len(items), status.ctypes.data, total))
    return status


def _show_args(kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds=None, M2=None, m3=None, outputs=True):
    """(CredentialsSoA, KeypairsSoA or None, ShowRandomness, PresentationOut, output dict, count, keepalive) of one layout's credentials
    (outputs=False: no output arrays - an empty PresentationOut and dict, for afx_show_wire, which does not read them)"""
    n = len(kinds)
    values, t, U, V, z_wide, rng_seed = map(_u8, (values, t, U, V, z_wide, rng_seed))
    cnt = t.shape[0]
    nsp = sum(1 for k in kinds if k == 4)
    hs = sum(1 for k in kinds if k == 1)
    cs = CredentialsSoA()
    cs.n_attributes = n
    for i, k in enumerate(kinds):
        cs.kinds[i] = k
    keep = [values, t, U, V, z_wide, rng_seed]
    cs.values, cs.t, cs.U, cs.V = values.ctypes.data, t.ctypes.data, U.ctypes.data, V.ctypes.data
    if nsp:
        M2, m3, enc_seeds = _u8(M2), _u8(m3), _u8(enc_seeds)
        keep += [M2, m3, enc_seeds]
        cs.M2, cs.m3 = M2.ctypes.data, m3.ctypes.data
    kp = None
    if keypairs is not None:
        ka = {f: _u8(keypairs[f]) for f in ("a", "a0", "a1", "pk")}
        keep.append(ka)
        kp = KeypairsSoA(*(ka[f].ctypes.data for f in ("a", "a0", "a1", "pk")))
    rnd = ShowRandomness(z_wide.ctypes.data, rng_seed.ctypes.data, enc_seeds.ctypes.data if nsp else None)
    if not outputs:
        return cs, kp, rnd, PresentationOut(), {}, cnt, keep
    o = {k: np.zeros((cnt, 32), np.uint8) for k in ("challenge", "C_x_0", "C_x_1", "C_V")}
    o["responses"] = np.zeros((3 + hs, cnt, 32), np.uint8)
    o["C_y"] = np.zeros((n, cnt, 32), np.uint8)
    o["attr_values"] = np.zeros((n, cnt, 32), np.uint8)
    o["enc"] = []
    eouts = (EncProofOut * max(1, nsp))()
    for e in range(nsp):
        d = {f: np.zeros(((6, cnt, 32) if f == "responses" else (cnt, 32)), np.uint8) for f in ENC_FIELDS}
        for f, v in d.items():
            setattr(eouts[e], f, v.ctypes.data)
        o["enc"].append(d)
    out = PresentationOut()
    for f in PRES_FIELDS:
        setattr(out, f, o[f].ctypes.data)
    out.enc = C.cast(eouts, C.POINTER(EncProofOut))
    keep.append(eouts)
    return cs, kp, rnd, out, o, cnt, keep


def show(ctx, kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds=None, M2=None, m3=None, first=None, n_items=None):
    """AnonymousCredential::show over a batch.  kinds: AFX_ATTR_* after hide/reveal.  values/M2/m3 [n,count,32];
    keypairs: dict(a,a0,a1,pk -> [count,32]) or None; enc_seeds [#secret points, count, 32].
    Returns (presentation dict incl. 'enc' list, Shape, status).  ctx may be a Group; with first/n_items only that range
    of the batch is shown (afx_show_range; the other output rows stay zero / status 255)."""
    cs, kp, rnd, out, o, cnt, keep = _show_args(kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds, M2, m3)
    shape = Shape()
    status = np.full(cnt, 255, np.uint8)
    kpp = C.byref(kp) if kp is not None else None
    if first is not None:
        check(lib().afx_show_range(ctx.h, C.byref(cs), kpp, C.byref(rnd), cnt, first, n_items, C.byref(out), C.byref(shape), status.ctypes.data))
    elif hasattr(ctx, "member"):
        check(lib().afx_group_show(ctx.h, C.byref(cs), kpp, C.byref(rnd), cnt, C.byref(out), C.byref(shape), status.ctypes.data))
    else:
        check(lib().afx_show(ctx.h, C.byref(cs), kpp, C.byref(rnd), cnt, C.byref(out), C.byref(shape), status.ctypes.data))
    return o, shape, status


def show_mixed(ctx, items):
    """AnonymousCredential::show over credentials of DIFFERENT layouts in one call (afx_show_mixed / afx_group_show_mixed).
    items = [dict(kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds=None, M2=None, m3=None, positions=None)].
    Returns ([(presentation dict, Shape) per group], status in the caller's order)."""
    arr = (ShowGroup * max(1, len(items)))()
    keep, outs, counts = [], [], []
    for g, it in enumerate(items):
        cs, kp, rnd, out, o, cnt, k = _show_args(it["kinds"], it["values"], it["t"], it["U"], it["V"], it.get("keypairs"), it["z_wide"], it["rng_seed"],
                                                 it.get("enc_seeds"), it.get("M2"), it.get("m3"))
        arr[g].creds, arr[g].rnd, arr[g].out, arr[g].count = cs, rnd, out, cnt
        if kp is not None:
            arr[g].keypairs = C.pointer(kp)
        keep.append((k, kp))
        outs.append(o)
        counts.append(cnt)
    pos, total = _positions(list(zip(items, counts)))
    total = max([total] + [int(p.max()) + 1 for p in pos if p.size])
    for g, p in enumerate(pos):
        arr[g].positions = p.ctypes.data_as(C.POINTER(C.c_uint64))
    status = np.full(total, 255, np.uint8)
    fn = lib().afx_group_show_mixed if hasattr(ctx, "member") else lib().afx_show_mixed
    check(fn(ctx.h, arr, len(items), status.ctypes.data, total))
    return [(o, Shape.from_buffer_copy(bytes(arr[g].shape_out))) for g, o in enumerate(outs)], status


def presentation_soa(p, ptr=lambda a: a.ctypes.data):
    """afx_presentation_soa over a presentation dict (numpy arrays by default; pass ptr=lambda t: t.data_ptr()
    for torch device tensors).  Returns (soa, keepalive)."""
    encs = (EncProofSoA * max(1, len(p["enc"])))()
    for e, d in enumerate(p["enc"]):
        for f in ENC_FIELDS:
            setattr(encs[e], f, ptr(d[f]))
    soa = PresentationSoA()
    for f in PRES_FIELDS:
        setattr(soa, f, ptr(p[f]))
    soa.enc = C.cast(encs, C.POINTER(EncProofSoA))
    return soa, encs


def verify_presentations(ctx, shape, p, first=None, n=None):
    """Issuer::verify over a batch of presentations held in host numpy arrays.  ctx may be a Group (all its GPUs); with
    first/n only that range is verified (afx_verify_presentations_range; the other status bytes stay 255)."""
    p = dict(p, **{f: _u8(p[f]) for f in PRES_FIELDS}, enc=[{f: _u8(d[f]) for f in ENC_FIELDS} for d in p["enc"]])
    cnt = p["challenge"].shape[0]
    soa, keep = presentation_soa(p)
    status = np.full(cnt, 255, np.uint8)
    if first is not None:
        check(lib().afx_verify_presentations_range(ctx.h, C.byref(shape), C.byref(soa), cnt, first, n, status.ctypes.data))
    elif hasattr(ctx, "member"):
        check(lib().afx_group_verify_presentations(ctx.h, C.byref(shape), C.byref(soa), cnt, status.ctypes.data))
    else:
        check(lib().afx_verify_presentations(ctx.h, C.byref(shape), C.byref(soa), cnt, status.ctypes.data))
    return status


def commitments_soa(cm, ptr=lambda a: a.ctypes.data):
    """afx_commitments_soa over dict(main [n_main,count,32], enc [[5,count,32] per proof of encryption]); returns (soa, keepalive)"""
    encs = (C.c_void_p * max(1, len(cm["enc"])))(*[ptr(a) for a in cm["enc"]])
    return CommitmentsSoA(ptr(cm["main"]), C.cast(encs, C.POINTER(C.c_void_p))), encs


def device_rng(seed, stream=0):
    """afx_device_rng; seed None: the library reads one from getrandom for the call"""
    return DeviceRng(bytes(seed) if seed is not None else None, stream)


def shape_of_kinds(kinds):
    """the afx_shape afx_show derives from credential kinds (AFX_ATTR_*)"""
    sh = Shape()
    sh.n_attributes = len(kinds)
    hs = ne = 0
    for i, k in enumerate(kinds):
        sh.kinds[i] = {0: 0, 1: 1, 4: 3}.get(k, 2)   # AFX_ENC_PUBLIC_SCALAR, _SECRET_SCALAR, _SECRET_POINT, else _PUBLIC_POINT
        if k == 1:
            sh.hidden_scalar_indices[hs] = i
            hs += 1
        elif k == 4:
            sh.enc_indices[ne] = i
            ne += 1
    sh.n_hidden_scalars, sh.n_responses, sh.n_enc_proofs = hs, 3 + hs, ne
    return sh


def show_batchable(ctx, kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds=None, M2=None, m3=None):
    """AnonymousCredential::show with both encodings of every proof (afx_show_batchable): what show() returns plus the commitments,
    dict(main [n_main,count,32], enc [[5,count,32] per proof of encryption]).  Returns (presentation, commitments, Shape, status)."""
    cs, kp, rnd, out, o, cnt, keep = _show_args(kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds, M2, m3)
    sh0 = shape_of_kinds(kinds)
    n_main = lib().afx_batchable_main_commitments(ctx.h, C.byref(sh0))
    cm = {"main": np.zeros((n_main, cnt, 32), np.uint8), "enc": [np.zeros((5, cnt, 32), np.uint8) for _ in range(sh0.n_enc_proofs)]}
    csoa, keep2 = commitments_soa(cm)
    shape = Shape()
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_show_batchable(ctx.h, C.byref(cs), C.byref(kp) if kp is not None else None, C.byref(rnd), cnt, C.byref(out), C.byref(csoa),
                                   C.byref(shape), status.ctypes.data))
    return o, cm, shape, status


def verify_presentations_batchable(ctx, shape, p, commitments, seed=None, stream=0):
    """Issuer::verify over batchable presentations (afx_verify_presentations_batchable): p as for verify_presentations (its challenge
    fields are not read and may be missing), commitments = dict(main, enc) as show_batchable returns them.  seed: 32 bytes for a
    reproducible run; None draws the weights from a seed the library reads from getrandom."""
    cnt = _u8(p["responses"]).shape[1]
    zero = np.zeros((cnt, 32), np.uint8)
    q = {f: _u8(p[f]) if p.get(f) is not None else zero for f in PRES_FIELDS}
    q["enc"] = [{f: _u8(d[f]) if d.get(f) is not None else zero for f in ENC_FIELDS} for d in p["enc"]]
    soa, keep = presentation_soa(q)
    cm = {"main": _u8(commitments["main"]), "enc": [_u8(a) for a in commitments["enc"]]}
    csoa, keep2 = commitments_soa(cm)
    rng = device_rng(seed, stream)
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_verify_presentations_batchable(ctx.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), cnt, status.ctypes.data))
    return status


def points_from_uniform(ctx, wide):
    wide = _u8(wide)
    out = np.zeros((wide.shape[0], 32), np.uint8)
    check(lib().afx_points_from_uniform_bytes(ctx.h, wide.ctypes.data, wide.shape[0], out.ctypes.data))
    return out


def scalars_from_wide(ctx, wide):
    wide = _u8(wide)
    out = np.zeros((wide.shape[0], 32), np.uint8)
    check(lib().afx_scalars_from_wide_bytes(ctx.h, wide.ctypes.data, wide.shape[0], out.ctypes.data))
    return out


def sha512(ctx, msgs):
    """SHA-512 of every row of msgs [count, msg_len] (msg_len 0 .. 1024) on the device (afx_sha512) -> [count, 64]"""
    msgs = _u8(msgs)
    out = np.zeros((msgs.shape[0], 64), np.uint8)
    check(lib().afx_sha512(ctx.h, msgs.ctypes.data, msgs.shape[1], msgs.shape[0], out.ctypes.data))
    return out


def plaintexts_from_bytes(ctx, msgs):
    """Plaintext::from(&[u8; 30]) over msgs [count, 30] (afx_plaintexts_from_bytes) -> M1, M2, m3 ([count, 32]), counters [count]"""
    msgs = _u8(msgs)
    cnt = msgs.shape[0]
    assert msgs.shape == (cnt, 30)
    M1, M2, m3 = (np.zeros((cnt, 32), np.uint8) for _ in range(3))
    counters = np.zeros(cnt, np.uint32)
    check(lib().afx_plaintexts_from_bytes(ctx.h, msgs.ctypes.data, cnt, M1.ctypes.data, M2.ctypes.data, m3.ctypes.data, counters.ctypes.data))
    return M1, M2, m3, counters


def keypairs_derive(ctx, master_secrets):
    """Keypair::derive over master_secrets [count, 64] (afx_keypairs_derive) -> dict(a, a0, a1, pk), [count, 32] each"""
    ms = _u8(master_secrets)
    cnt = ms.shape[0]
    assert ms.shape == (cnt, 64)
    kp = {f: np.zeros((cnt, 32), np.uint8) for f in ("a", "a0", "a1", "pk")}
    check(lib().afx_keypairs_derive(ctx.h, ms.ctypes.data, cnt, *(kp[f].ctypes.data for f in ("a", "a0", "a1", "pk"))))
    return kp


def _keypairs_soa(kp, ptr):
    return KeypairsSoA(*(ptr(kp[f]) if kp.get(f) is not None else None for f in ("a", "a0", "a1", "pk")))


def encrypt(ctx, keypairs, M1, M2, m3):
    """Keypair::encrypt over arrays (afx_encrypt): keypairs = dict(a, a0, a1[, pk]) -> E1, E2 ([count, 32]), status [count]"""
    kp = {f: _u8(v) for f, v in keypairs.items() if v is not None}
    M1, M2, m3 = _u8(M1), _u8(M2), _u8(m3)
    cnt = M1.shape[0]
    E1, E2 = np.zeros((cnt, 32), np.uint8), np.zeros((cnt, 32), np.uint8)
    status = np.full(cnt, 255, np.uint8)
    soa = _keypairs_soa(kp, lambda a: a.ctypes.data)
    check(lib().afx_encrypt(ctx.h, C.byref(soa), M1.ctypes.data, M2.ctypes.data, m3.ctypes.data, cnt, E1.ctypes.data, E2.ctypes.data, status.ctypes.data))
    return E1, E2, status


def decrypt(ctx, keypairs, E1, E2, messages=True):
    """Keypair::decrypt over arrays (afx_decrypt) -> M1, M2, m3 ([count, 32]), messages ([count, 30], or None), status [count]"""
    kp = {f: _u8(v) for f, v in keypairs.items() if v is not None}
    E1, E2 = _u8(E1), _u8(E2)
    cnt = E1.shape[0]
    M1, M2, m3 = (np.zeros((cnt, 32), np.uint8) for _ in range(3))
    msg = np.zeros((cnt, 30), np.uint8) if messages else None
    status = np.full(cnt, 255, np.uint8)
    soa = _keypairs_soa(kp, lambda a: a.ctypes.data)
    check(lib().afx_decrypt(ctx.h, C.byref(soa), E1.ctypes.data, E2.ctypes.data, cnt, M1.ctypes.data, M2.ctypes.data, m3.ctypes.data,
                            msg.ctypes.data if messages else None, status.ctypes.data))
    return M1, M2, m3, msg, status


# The *_dev forms: every array is a device pointer - an int, or anything that carries one as .data_ptr() (a torch tensor) or .ptr -
# to rows the caller allocated on the context's device; the call is asynchronous on afx_ctx_stream (ctx.synchronize() waits for it).
def _dptr(x):
    if x is None or isinstance(x, int):
        return x
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ptr


def plaintexts_from_bytes_dev(ctx, msgs, count, M1, M2, m3, counters, status):
    """afx_plaintexts_from_bytes_dev: msgs [count][30] -> M1, M2, m3 ([count][32]), counters ([count] u32, or None), status [count]"""
    check(lib().afx_plaintexts_from_bytes_dev(ctx.h, _dptr(msgs), count, _dptr(M1), _dptr(M2), _dptr(m3), _dptr(counters), _dptr(status)))


def keypairs_derive_dev(ctx, master_secrets, count, a, a0, a1, pk):
    """afx_keypairs_derive_dev: master_secrets [count][64] -> a, a0, a1, pk ([count][32] each)"""
    check(lib().afx_keypairs_derive_dev(ctx.h, _dptr(master_secrets), count, _dptr(a), _dptr(a0), _dptr(a1), _dptr(pk)))


def encrypt_dev(ctx, keypairs, M1, M2, m3, count, E1, E2, status):
    """afx_encrypt_dev: keypairs = dict(a, a0, a1[, pk]) of device rows"""
    soa = _keypairs_soa(keypairs, _dptr)
    check(lib().afx_encrypt_dev(ctx.h, C.byref(soa), _dptr(M1), _dptr(M2), _dptr(m3), count, _dptr(E1), _dptr(E2), _dptr(status)))


def decrypt_dev(ctx, keypairs, E1, E2, count, M1, M2, m3, messages, status):
    """afx_decrypt_dev: messages ([count][30]) may be None"""
    soa = _keypairs_soa(keypairs, _dptr)
    check(lib().afx_decrypt_dev(ctx.h, C.byref(soa), _dptr(E1), _dptr(E2), count, _dptr(M1), _dptr(M2), _dptr(m3), _dptr(messages), _dptr(status)))


# ---- whole messages (include/aeonflux_gpu.h "whole messages"): any length, one key per message ----
def message_chunks(length):
    """afx_message_chunks: 30-byte chunks of a message of `length` bytes"""
    return int(lib().afx_message_chunks(length))


def pack_messages(messages):
    """a list of bytes -> (blob [total] u8, offsets [count + 1] u64); a (blob, offsets) pair goes through as arrays"""
    if isinstance(messages, tuple):
        blob, offsets = messages
        return np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8) if isinstance(blob, (bytes, bytearray)) else _u8(blob).reshape(-1)), \
            np.ascontiguousarray(offsets, dtype=np.uint64)
    offsets = np.zeros(len(messages) + 1, np.uint64)
    if len(messages):
        offsets[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    return np.frombuffer(b"".join(bytes(m) for m in messages), np.uint8).copy(), offsets


def chunk_table(offsets):
    """afx_messages_chunk_table: offsets [count + 1] -> chunk_first [count + 1] u32"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cf = np.zeros(offsets.size, np.uint32)
    check(lib().afx_messages_chunk_table(offsets.ctypes.data, offsets.size - 1, cf.ctypes.data))
    return cf


def _blob_ptr(blob):
    # (a batch of only empty messages still hands the library a pointer)
    return blob.ctypes.data if blob.size else _NO_BYTES.ctypes.data


_NO_BYTES = np.zeros(16, np.uint8)


def split_messages(rows, chunk_first):
    """[n_chunks, 30] recovered rows -> a list of bytes, 30 * chunks(i) each"""
    flat = _u8(rows).reshape(-1)
    return [flat[30 * int(chunk_first[i]):30 * int(chunk_first[i + 1])].tobytes() for i in range(len(chunk_first) - 1)]


def plaintexts_from_messages(ctx, messages):
    """Plaintext::from_slice over a batch (afx_plaintexts_from_messages): messages = a list of bytes, or (blob, offsets)
    -> M1, M2, m3 ([n_chunks, 32]), counters [n_chunks], chunk_first [count + 1]"""
    blob, offsets = pack_messages(messages)
    cf = chunk_table(offsets)
    n = int(cf[-1])
    M1, M2, m3 = (np.zeros((n, 32), np.uint8) for _ in range(3))
    counters = np.zeros(n, np.uint32)
    # (n == 0: numpy may hand out a null pointer for an empty array - the library gets room it will not write)
    room = [np.zeros((1, 32), np.uint8) for _ in range(4)] if n == 0 else [M1, M2, m3, counters]
    check(lib().afx_plaintexts_from_messages(ctx.h, _blob_ptr(blob), offsets.ctypes.data, offsets.size - 1, *(a.ctypes.data for a in room)))
    return M1, M2, m3, counters, cf


def plaintexts_from_points(ctx, points):
    """impl From<&RistrettoPoint> for Plaintext (afx_plaintexts_from_points): points [count, 32] -> M2, m3 ([count, 32]), status [count]"""
    points = _u8(points)
    cnt = points.shape[0]
    M2, m3 = np.zeros((cnt, 32), np.uint8), np.zeros((cnt, 32), np.uint8)
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_plaintexts_from_points(ctx.h, points.ctypes.data, cnt, M2.ctypes.data, m3.ctypes.data, status.ctypes.data))
    return M2, m3, status


def plaintexts_from_bytes_at(ctx, msgs, counters):
    """afx_plaintexts_from_bytes_at: msgs [count, 30], counters [count] (what plaintexts_from_bytes returned) -> M1, M2, m3, status"""
    msgs = _u8(msgs)
    cnt = msgs.shape[0]
    assert msgs.shape == (cnt, 30)
    counters = np.ascontiguousarray(counters, dtype=np.uint32)
    assert counters.shape == (cnt,)
    M1, M2, m3 = (np.zeros((cnt, 32), np.uint8) for _ in range(3))
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_plaintexts_from_bytes_at(ctx.h, msgs.ctypes.data, counters.ctypes.data, cnt, M1.ctypes.data, M2.ctypes.data, m3.ctypes.data, status.ctypes.data))
    return M1, M2, m3, status


def encrypt_messages(ctx, keypairs, messages):
    """afx_encrypt_messages: keypairs = dict(a, a0, a1[, pk]) with one row per MESSAGE; messages = a list of bytes, or (blob, offsets)
    -> E1, E2 ([n_chunks, 32]), counters [n_chunks], chunk_first [count + 1], status [count] per message"""
    kp = {f: _u8(v) for f, v in keypairs.items() if v is not None}
    blob, offsets = pack_messages(messages)
    cf = chunk_table(offsets)
    cnt, n = offsets.size - 1, int(cf[-1])
    assert kp["a"].shape == (cnt, 32)
    E1, E2 = np.zeros((max(n, 1), 32), np.uint8), np.zeros((max(n, 1), 32), np.uint8)
    counters = np.zeros(max(n, 1), np.uint32)
    status = np.full(max(cnt, 1), 255, np.uint8)
    soa = _keypairs_soa(kp, lambda a: a.ctypes.data)
    check(lib().afx_encrypt_messages(ctx.h, C.byref(soa), _blob_ptr(blob), offsets.ctypes.data, cnt, E1.ctypes.data, E2.ctypes.data, counters.ctypes.data,
                                     status.ctypes.data))
    return E1[:n], E2[:n], counters[:n], cf, status[:cnt]


def decrypt_messages(ctx, keypairs, E1, E2, chunk_first, fill=0, as_rows=False):
    """afx_decrypt_messages: E1, E2 [n_chunks, 32], chunk_first [count + 1] -> (a list of bytes, 30 * chunks(i) each; status [count]).
    A message that did not decrypt comes back as zeros.  `fill`: what the output holds before the call (tests); `as_rows`: the
    [n_chunks, 30] array itself instead of the list (message i at row chunk_first[i])."""
    kp = {f: _u8(v) for f, v in keypairs.items() if v is not None}
    E1, E2 = _u8(E1), _u8(E2)
    cf = np.ascontiguousarray(chunk_first, dtype=np.uint32)
    cnt, n = cf.size - 1, int(cf[-1])
    assert E1.shape[0] == n and E2.shape[0] == n
    rows = np.full((max(n, 1), 30), fill, np.uint8)
    status = np.full(max(cnt, 1), 255, np.uint8)
    soa = _keypairs_soa(kp, lambda a: a.ctypes.data)
    check(lib().afx_decrypt_messages(ctx.h, C.byref(soa), E1.ctypes.data if n else _NO_BYTES.ctypes.data, E2.ctypes.data if n else _NO_BYTES.ctypes.data,
                                     cf.ctypes.data, cnt, rows.ctypes.data, status.ctypes.data))
    return (rows[:n] if as_rows else split_messages(rows[:n], cf)), status[:cnt]


# the *_dev forms: data pointers are device pointers; offsets / chunk_first stay host arrays (numpy), read before the call returns
def plaintexts_from_messages_dev(ctx, blob, offsets, M1, M2, m3, counters, status):
    """afx_plaintexts_from_messages_dev: blob on the device, offsets [count + 1] u64 on the host; status [n_chunks]"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    check(lib().afx_plaintexts_from_messages_dev(ctx.h, _dptr(blob), offsets.ctypes.data, offsets.size - 1, _dptr(M1), _dptr(M2), _dptr(m3), _dptr(counters),
                                                 _dptr(status)))


def plaintexts_from_points_dev(ctx, points, count, M2, m3, status):
    check(lib().afx_plaintexts_from_points_dev(ctx.h, _dptr(points), count, _dptr(M2), _dptr(m3), _dptr(status)))


def plaintexts_from_bytes_at_dev(ctx, msgs, counters, count, M1, M2, m3, status):
    check(lib().afx_plaintexts_from_bytes_at_dev(ctx.h, _dptr(msgs), _dptr(counters), count, _dptr(M1), _dptr(M2), _dptr(m3), _dptr(status)))


def encrypt_messages_dev(ctx, keypairs, blob, offsets, E1, E2, counters, status):
    """afx_encrypt_messages_dev: keypairs = dict(a, a0, a1) of device rows, one per message; status [count]"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    soa = _keypairs_soa(keypairs, _dptr)
    check(lib().afx_encrypt_messages_dev(ctx.h, C.byref(soa), _dptr(blob), offsets.ctypes.data, offsets.size - 1, _dptr(E1), _dptr(E2), _dptr(counters), _dptr(status)))


def decrypt_messages_dev(ctx, keypairs, E1, E2, chunk_first, messages, status):
    """afx_decrypt_messages_dev: chunk_first [count + 1] u32 on the host; messages [n_chunks][30] and status [count] on the device"""
    cf = np.ascontiguousarray(chunk_first, dtype=np.uint32)
    soa = _keypairs_soa(keypairs, _dptr)
    check(lib().afx_decrypt_messages_dev(ctx.h, C.byref(soa), _dptr(E1), _dptr(E2), cf.ctypes.data, cf.size - 1, _dptr(messages), _dptr(status)))


# ---- blind issuance (include/aeonflux_gpu.h "Blind issuance") ----
REQUEST_FIELDS = ("D", "A", "B", "challenge", "responses")
BLIND_ISSUANCE_FIELDS = ("t", "U", "S1", "S2", "challenge", "responses")


def blind_layout(kinds):
    """(h, hs): hidden positions of a layout and how many of them are scalars; a request has 1 + h + hs responses"""
    return sum(1 for k in kinds if k in (1, 4)), sum(1 for k in kinds if k == 1)


def _blind_attrs(kinds, values, ptr):
    s = AttributesSoA()
    s.n_attributes = len(kinds)
    for i, k in enumerate(kinds[:len(s.kinds)]):
        s.kinds[i] = k
    s.values = ptr(values) if values is not None else None
    return s


def _hptr(a):
    return a.ctypes.data if a is not None and a.size else None


def blind_request(ctx, kinds, values, d, r_wide, rng_seed):
    """afx_blind_request: values [n, count, 32], d [count, 32], r_wide [h, count, 64], rng_seed [count, 32]
    -> (dict(D, A [h], B [h], challenge, responses [1 + h + hs]), status [count])"""
    values, d, r_wide, rng_seed = map(_u8, (values, d, r_wide, rng_seed))
    cnt = d.shape[0]
    h, hs = blind_layout(kinds)
    o = dict(D=np.zeros((cnt, 32), np.uint8), A=np.zeros((h, cnt, 32), np.uint8), B=np.zeros((h, cnt, 32), np.uint8), challenge=np.zeros((cnt, 32), np.uint8),
             responses=np.zeros((1 + h + hs, cnt, 32), np.uint8))
    status = np.full(cnt, 255, np.uint8)
    a = _blind_attrs(kinds, values, _hptr)
    rnd = BlindRequestRandomness(_hptr(r_wide), _hptr(rng_seed))
    out = BlindRequestSoA(*(_hptr(o[f]) for f in REQUEST_FIELDS))
    check(lib().afx_blind_request(ctx.h, C.byref(a), _hptr(d), C.byref(rnd), cnt, C.byref(out), status.ctypes.data))
    return o, status


def verify_blind_requests(ctx, kinds, request, n_responses=None):
    """afx_verify_blind_requests -> status [count]"""
    q = {f: _u8(request[f]) for f in REQUEST_FIELDS}
    cnt = q["D"].shape[0]
    status = np.full(cnt, 255, np.uint8)
    a = _blind_attrs(kinds, None, _hptr)
    soa = BlindRequestSoA(*(_hptr(q[f]) for f in REQUEST_FIELDS))
    nr = q["responses"].shape[0] if n_responses is None else n_responses
    check(lib().afx_verify_blind_requests(ctx.h, C.byref(a), C.byref(soa), nr, cnt, status.ctypes.data))
    return status


def issue_blind(ctx, kinds, values, request, t_wide, U_wide, rprime_wide, rng_seed, request_n_responses=None):
    """afx_issue_blind: values [n, count, 32] (the rows of hidden positions are never read), request as blind_request returned it
    -> (dict(t, U, S1, S2, challenge, responses [n + 6]), status [count])"""
    values, t_wide, U_wide, rprime_wide, rng_seed = map(_u8, (values, t_wide, U_wide, rprime_wide, rng_seed))
    q = {f: _u8(request[f]) for f in REQUEST_FIELDS}
    cnt = t_wide.shape[0]
    o = {f: np.zeros((cnt, 32), np.uint8) for f in BLIND_ISSUANCE_FIELDS[:5]}
    o["responses"] = np.zeros((ctx.n + 6, cnt, 32), np.uint8)
    status = np.full(cnt, 255, np.uint8)
    a = _blind_attrs(kinds, values, _hptr)
    soa = BlindRequestSoA(*(_hptr(q[f]) for f in REQUEST_FIELDS))
    rnd = BlindIssueRandomness(*(_hptr(x) for x in (t_wide, U_wide, rprime_wide, rng_seed)))
    out = BlindIssuanceSoA(*(_hptr(o[f]) for f in BLIND_ISSUANCE_FIELDS))
    nr = q["responses"].shape[0] if request_n_responses is None else request_n_responses
    check(lib().afx_issue_blind(ctx.h, C.byref(a), C.byref(soa), nr, C.byref(rnd), cnt, C.byref(out), status.ctypes.data))
    return o, status


def unblind_issuances(ctx, kinds, values, d, request, issuance, n_responses=None):
    """afx_unblind_issuances: the user's own request (D, A, B) and d, the issuer's answer -> (V [count, 32], status [count])"""
    values, d = _u8(values), _u8(d)
    q = {f: _u8(request[f]) for f in ("D", "A", "B")}
    s = {f: _u8(issuance[f]) for f in BLIND_ISSUANCE_FIELDS}
    cnt = d.shape[0]
    V = np.zeros((cnt, 32), np.uint8)
    status = np.full(cnt, 255, np.uint8)
    a = _blind_attrs(kinds, values, _hptr)
    soa = BlindRequestSoA(_hptr(q["D"]), _hptr(q["A"]), _hptr(q["B"]), None, None)
    iss = BlindIssuanceSoA(*(_hptr(s[f]) for f in BLIND_ISSUANCE_FIELDS))
    nr = s["responses"].shape[0] if n_responses is None else n_responses
    check(lib().afx_unblind_issuances(ctx.h, C.byref(a), _hptr(d), C.byref(soa), C.byref(iss), nr, cnt, V.ctypes.data, status.ctypes.data))
    return V, status


def blind_request_dev(ctx, kinds, values, d, r_wide, rng_seed, count, out, status):
    """afx_blind_request_dev: device rows; out = dict(D, A, B, challenge, responses) of device rows (A, B may be None when h == 0)"""
    a = _blind_attrs(kinds, values, _dptr)
    rnd = BlindRequestRandomness(_dptr(r_wide), _dptr(rng_seed))
    soa = BlindRequestSoA(*(_dptr(out.get(f)) for f in REQUEST_FIELDS))
    check(lib().afx_blind_request_dev(ctx.h, C.byref(a), _dptr(d), C.byref(rnd), count, C.byref(soa), _dptr(status)))


def verify_blind_requests_dev(ctx, kinds, request, n_responses, count, status):
    a = _blind_attrs(kinds, None, _dptr)
    soa = BlindRequestSoA(*(_dptr(request.get(f)) for f in REQUEST_FIELDS))
    check(lib().afx_verify_blind_requests_dev(ctx.h, C.byref(a), C.byref(soa), n_responses, count, _dptr(status)))


def issue_blind_dev(ctx, kinds, values, request, request_n_responses, t_wide, U_wide, rprime_wide, rng_seed, count, out, status):
    a = _blind_attrs(kinds, values, _dptr)
    soa = BlindRequestSoA(*(_dptr(request.get(f)) for f in REQUEST_FIELDS))
    rnd = BlindIssueRandomness(*(_dptr(x) for x in (t_wide, U_wide, rprime_wide, rng_seed)))
    o = BlindIssuanceSoA(*(_dptr(out.get(f)) for f in BLIND_ISSUANCE_FIELDS))
    check(lib().afx_issue_blind_dev(ctx.h, C.byref(a), C.byref(soa), request_n_responses, C.byref(rnd), count, C.byref(o), _dptr(status)))


def unblind_issuances_dev(ctx, kinds, values, d, request, issuance, n_responses, count, V, status):
    a = _blind_attrs(kinds, values, _dptr)
    soa = BlindRequestSoA(_dptr(request.get("D")), _dptr(request.get("A")), _dptr(request.get("B")), None, None)
    iss = BlindIssuanceSoA(*(_dptr(issuance.get(f)) for f in BLIND_ISSUANCE_FIELDS))
    check(lib().afx_unblind_issuances_dev(ctx.h, C.byref(a), _dptr(d), C.byref(soa), C.byref(iss), n_responses, count, _dptr(V), _dptr(status)))


# ---- presentation tags (include/aeonflux_gpu.h "Presentation tags") -------------------------------------------------------------
TAG_FIELDS = ("T", "challenge", "responses")


def tag_scope_generator(ctx, scope):
    """afx_tag_scope_generator: H = RistrettoPoint::hash_from_bytes::<Sha512>(scope), 32 bytes"""
    scope = bytes(scope)
    out = np.zeros(32, np.uint8)
    check(lib().afx_tag_scope_generator(ctx.h, scope, len(scope), out.ctypes.data))
    return bytes(out)


def _tag_statement(position, H):
    H = bytes(H)
    assert len(H) == 32
    return TagStatement(position, H)


def show_tagged(ctx, kinds, values, t, U, V, keypairs, z_wide, rng_seed, position, H, nonce, tag_seed, enc_seeds=None, M2=None, m3=None):
    """afx_show_tagged: show() plus the tag of the hidden scalar at `position` under the scope generator H (32 bytes) and the per-item
    counters nonce [count, 32], its proof drawn from tag_seed [count, 32].
    Returns (presentation dict, dict(T, challenge [count, 32], responses [2, count, 32]), Shape, status)."""
    cs, kp, rnd, out, o, cnt, keep = _show_args(kinds, values, t, U, V, keypairs, z_wide, rng_seed, enc_seeds, M2, m3)
    nonce, tag_seed = _u8(nonce), _u8(tag_seed)
    tags = dict(T=np.zeros((cnt, 32), np.uint8), challenge=np.zeros((cnt, 32), np.uint8), responses=np.zeros((2, cnt, 32), np.uint8))
    tout = TagsOut(*(tags[f].ctypes.data for f in TAG_FIELDS))
    stmt = _tag_statement(position, H)
    shape = Shape()
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_show_tagged(ctx.h, C.byref(cs), C.byref(kp) if kp is not None else None, C.byref(rnd), C.byref(stmt), nonce.ctypes.data, tag_seed.ctypes.data,
                                cnt, C.byref(out), C.byref(tout), C.byref(shape), status.ctypes.data))
    return o, tags, shape, status


def tags_soa(nonce, tags, ptr=lambda a: a.ctypes.data):
    """afx_tags_soa over the counters and a tag dict(T, challenge, responses)"""
    return TagsSoA(ptr(nonce), *(ptr(tags[f]) for f in TAG_FIELDS))


def verify_presentations_tagged(ctx, shape, p, position, H, nonce, tags):
    """afx_verify_presentations_tagged: p as for verify_presentations, tags as show_tagged returned them -> status [count]"""
    p = dict(p, **{f: _u8(p[f]) for f in PRES_FIELDS}, enc=[{f: _u8(d[f]) for f in ENC_FIELDS} for d in p["enc"]])
    cnt = p["challenge"].shape[0]
    soa, keep = presentation_soa(p)
    nonce = _u8(nonce)
    tg = {f: _u8(tags[f]) for f in TAG_FIELDS}
    ts = tags_soa(nonce, tg)
    stmt = _tag_statement(position, H)
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_verify_presentations_tagged(ctx.h, C.byref(shape), C.byref(soa), C.byref(stmt), C.byref(ts), cnt, status.ctypes.data))
    return status


def verify_tag_proofs(ctx, position, H, C_y_p, nonce, tags):
    """afx_verify_tag_proofs: the tag proofs alone on the presentations' C_y[position] row [count, 32] -> status [count]"""
    C_y_p, nonce = _u8(C_y_p), _u8(nonce)
    tg = {f: _u8(tags[f]) for f in TAG_FIELDS}
    cnt = C_y_p.shape[0]
    ts = tags_soa(nonce, tg)
    stmt = _tag_statement(position, H)
    status = np.full(cnt, 255, np.uint8)
    check(lib().afx_verify_tag_proofs(ctx.h, C.byref(stmt), C_y_p.ctypes.data, C.byref(ts), cnt, status.ctypes.data))
    return status


def show_tagged_dev(ctx, kinds, creds, keypairs, rnd, position, H, nonce, tag_seed, count, out, tags_out, status):
    """afx_show_tagged_dev over device rows: creds = dict(values, t, U, V[, M2, m3]), keypairs = dict(a, a0, a1, pk) or None, rnd =
    dict(z_wide, rng_seed[, enc_seeds]), out = a presentation dict of device rows (as presentation_soa reads it), tags_out = dict(T,
    challenge, responses).  H: 32 bytes of HOST memory.  Returns the Shape."""
    cs = CredentialsSoA()
    cs.n_attributes = len(kinds)
    for i, k in enumerate(kinds):
        cs.kinds[i] = k
    for f in ("values", "M2", "m3", "t", "U", "V"):
        setattr(cs, f, _dptr(creds.get(f)))
    kp = KeypairsSoA(*(_dptr(keypairs[f]) for f in ("a", "a0", "a1", "pk"))) if keypairs is not None else None
    r = ShowRandomness(_dptr(rnd["z_wide"]), _dptr(rnd["rng_seed"]), _dptr(rnd.get("enc_seeds")))
    eouts = (EncProofOut * max(1, len(out["enc"])))()
    for e, d in enumerate(out["enc"]):
        for f in ENC_FIELDS:
            setattr(eouts[e], f, _dptr(d[f]))
    po = PresentationOut()
    for f in PRES_FIELDS:
        setattr(po, f, _dptr(out.get(f)))
    po.enc = C.cast(eouts, C.POINTER(EncProofOut))
    tout = TagsOut(*(_dptr(tags_out[f]) for f in TAG_FIELDS))
    stmt = _tag_statement(position, H)
    shape = Shape()
    check(lib().afx_show_tagged_dev(ctx.h, C.byref(cs), C.byref(kp) if kp is not None else None, C.byref(r), C.byref(stmt), _dptr(nonce), _dptr(tag_seed), count,
                                    C.byref(po), C.byref(tout), C.byref(shape), _dptr(status)))
    return shape


def verify_presentations_tagged_dev(ctx, shape, p, position, H, nonce, tags, count, status):
    """afx_verify_presentations_tagged_dev: p and tags dicts of device rows"""
    soa, keep = presentation_soa(p, ptr=_dptr)
    ts = tags_soa(nonce, tags, ptr=_dptr)
    stmt = _tag_statement(position, H)
    check(lib().afx_verify_presentations_tagged_dev(ctx.h, C.byref(shape), C.byref(soa), C.byref(stmt), C.byref(ts), count, _dptr(status)))


def verify_tag_proofs_dev(ctx, position, H, C_y_p, nonce, tags, count, status):
    ts = tags_soa(nonce, tags, ptr=_dptr)
    stmt = _tag_statement(position, H)
    check(lib().afx_verify_tag_proofs_dev(ctx.h, C.byref(stmt), _dptr(C_y_p), C.byref(ts), count, _dptr(status)))


# ---- the spent-tag set (include/aeonflux_gpu.h "The spent-tag set") ------------------------------------------------------------
TAG_FRESH, TAG_SPENT, TAG_SKIPPED = 0, 1, 2


class TagSet:
    """afx_tagset: a set of spent tags on the context's device.  spend() answers as the sequential loop would: per item TAG_SKIPPED
    (status[i] != 0), TAG_SPENT (in the set already, or an earlier item of this call) or TAG_FRESH (inserted now).  Close it before
    its context."""

    def __init__(self, ctx, capacity, salt=None):
        if salt is not None:
            salt = bytes(salt)
            assert len(salt) == 32
        self.ctx = ctx                       # (keeps the context alive for as long as the set)
        h = C.c_void_p()
        check(lib().afx_tagset_create(ctx.h, capacity, salt, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if self.ctx.h:                   # (a context closed first has taken the device buffers' stream with it: nothing left to free safely)
                lib().afx_tagset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass

    def size(self):
        """(tags in the set, capacity); waits for the queued calls"""
        n, cap = C.c_uint64(), C.c_uint64()
        check(lib().afx_tagset_size(self.h, C.byref(n), C.byref(cap)))
        return n.value, cap.value

    def spend(self, T, status=None, out=None):
        """T [count, 32], status [count] or None -> seen [count] (into `out` when given: a refused call leaves it untouched)"""
        T = _u8(T).reshape(-1, 32)
        cnt = T.shape[0]
        st = _u8(status).reshape(cnt) if status is not None else None
        seen = out if out is not None else np.full(cnt, 255, np.uint8)
        check(lib().afx_tagset_spend(self.h, T.ctypes.data, st.ctypes.data if st is not None else None, cnt, seen.ctypes.data))
        return seen

    def contains(self, T):
        """T [count, 32] -> [count], 1 where the tag is in the set"""
        T = _u8(T).reshape(-1, 32)
        seen = np.full(T.shape[0], 255, np.uint8)
        check(lib().afx_tagset_contains(self.h, T.ctypes.data, T.shape[0], seen.ctypes.data))
        return seen

    def spend_dev(self, T, status, count, seen):
        """afx_tagset_spend_dev over device rows (status may be None); asynchronous on the context's stream"""
        check(lib().afx_tagset_spend_dev(self.h, _dptr(T), _dptr(status), count, _dptr(seen)))

    def contains_dev(self, T, count, seen):
        check(lib().afx_tagset_contains_dev(self.h, _dptr(T), count, _dptr(seen)))


def multiscalar_mul(ctx, scalars, points):
    """out[i] = sum_k scalars[k,i] * points[k,i];  scalars, points: [n_terms, count, 32]"""
    scalars, points = _u8(scalars), _u8(points)
    nt, cnt = scalars.shape[0], scalars.shape[1]
    out = np.zeros((cnt, 32), np.uint8)
    ok = np.zeros(cnt, np.uint8)
    check(lib().afx_multiscalar_mul(ctx.h, nt, scalars.ctypes.data, points.ctypes.data, cnt, out.ctypes.data, ok.ctypes.data))
    return out, ok


def shape_key(shape):
    """the batch-uniform part of a presentation, as a hashable key (SURVEY.md §7 "heterogeneous batches")"""
    return bytes(shape)


def verify_mixed(ctx, items):
    """Issuer::verify over presentations of different shapes: items = [(Shape, presentation dict with count 1 or more)].
    The items of one shape become one afx_presentation_group (arrays concatenated here: bytes only); the library runs one GPU
    batch per group (afx_verify_presentations_mixed, or its afx_group_* form when ctx is a Group) and writes every status at
    its presentation's place in the order given.  Returns the list of per-item status arrays."""
    from . import PresentationGroup
    groups, start, total = {}, [], 0
    for pos, (shape, p) in enumerate(items):
        k = _u8(p["challenge"]).shape[0]
        groups.setdefault(shape_key(shape), (shape, []))[1].append((total, k, p))
        start.append((total, k))
        total += k
    arr = (PresentationGroup * max(1, len(groups)))()
    keep = []
    for g, (shape, members) in enumerate(groups.values()):
        cat = {f: np.concatenate([_u8(p[f]) for _, _, p in members], axis=-2) for f in PRES_FIELDS}
        cat["enc"] = [{f: np.concatenate([_u8(p["enc"][e][f]) for _, _, p in members], axis=-2) for f in ENC_FIELDS}
                      for e in range(shape.n_enc_proofs)]
        soa, encs = presentation_soa(cat)
        positions = np.concatenate([np.arange(o, o + k, dtype=np.uint64) for o, k, _ in members])
        arr[g].shape, arr[g].batch, arr[g].count = shape, soa, positions.size
        arr[g].positions = positions.ctypes.data_as(C.POINTER(C.c_uint64))
        keep.append((cat, soa, encs, positions))
    status = np.full(total, 255, np.uint8)
    fn = lib().afx_group_verify_presentations_mixed if hasattr(ctx, "member") else lib().afx_verify_presentations_mixed
    check(fn(ctx.h, arr, len(groups), status.ctypes.data, total))
    return [status[o:o + k] for o, k in start]
