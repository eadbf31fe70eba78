"""Wire format of a batch of same-shape presentations ("AFXP" v1, include/aeonflux_gpu.h): the reference crate
defines no serialisation for ProofOfValidCredential (src/nizk/presentation.rs:117-127), so this is the engine's
own, in the crate's `u32le n || 32-byte items` style (src/parameters.rs:155-184).  Pure byte shuffling."""
import struct

import numpy as np

from . import Shape

ENC_ORDER = ("challenge", "responses", "pk", "E1", "E2", "C_y_1", "C_y_2", "C_y_3", "C_y_2p")


def header(shape, count):
    n, nr, hs, ne = shape.n_attributes, shape.n_responses, shape.n_hidden_scalars, shape.n_enc_proofs
    pub = sum(1 for i in range(n) if shape.kinds[i] in (0, 2))
    cells = 1 + nr + 3 + n + pub + 14 * ne
    h = b"AFXP" + struct.pack("<7I", 1, count, cells, n, nr, hs, ne)
    h += bytes(shape.kinds[:n])
    h += b"".join(struct.pack("<H", shape.hidden_scalar_indices[i]) for i in range(hs))
    h += b"".join(struct.pack("<H", shape.enc_indices[i]) for i in range(ne))
    h += bytes(-len(h) % 32)
    return h, cells


def pack_presentations(shape, p):
    """SoA presentation dict ([count,32] / [k,count,32] uint8 arrays) -> wire bytes"""
    count = p["challenge"].shape[0]
    n = shape.n_attributes
    cols = [p["challenge"][None], p["responses"], p["C_x_0"][None], p["C_x_1"][None], p["C_V"][None], p["C_y"]]
    cols += [p["attr_values"][i][None] for i in range(n) if shape.kinds[i] in (0, 2)]
    for d in p["enc"]:
        cols += [d[f] if d[f].ndim == 3 else d[f][None] for f in ENC_ORDER]
    soa = np.concatenate([np.asarray(c, dtype=np.uint8) for c in cols], axis=0)      # [cells, count, 32]
    h, cells = header(shape, count)
    assert soa.shape == (cells, count, 32)
    return h + np.ascontiguousarray(soa.transpose(1, 0, 2)).tobytes()


def unpack_presentations(blob):
    """wire bytes -> (Shape, SoA presentation dict)"""
    assert blob[:4] == b"AFXP"
    ver, count, cells, n, nr, hs, ne = struct.unpack("<7I", blob[4:32])
    assert ver == 1
    shape = Shape()
    shape.n_attributes, shape.n_responses, shape.n_hidden_scalars, shape.n_enc_proofs = n, nr, hs, ne
    o = 32
    for i in range(n):
        shape.kinds[i] = blob[o + i]
    o += n
    for i in range(hs):
        shape.hidden_scalar_indices[i] = struct.unpack("<H", blob[o:o + 2])[0]
        o += 2
    for i in range(ne):
        shape.enc_indices[i] = struct.unpack("<H", blob[o:o + 2])[0]
        o += 2
    o = (o + 31) & ~31
    rec = np.frombuffer(blob, dtype=np.uint8, offset=o).reshape(count, cells, 32).transpose(1, 0, 2)
    it = iter(range(cells))
    take = lambda k: np.ascontiguousarray(np.stack([rec[next(it)] for _ in range(k)]))
    p = {"challenge": take(1)[0], "responses": take(nr), "C_x_0": take(1)[0], "C_x_1": take(1)[0], "C_V": take(1)[0], "C_y": take(n)}
    av = np.zeros((n, count, 32), np.uint8)
    for i in range(n):
        if shape.kinds[i] in (0, 2):
            av[i] = take(1)[0]
    p["attr_values"] = av
    p["enc"] = []
    for _ in range(ne):
        p["enc"].append({f: (take(6) if f == "responses" else take(1)[0]) for f in ENC_ORDER})
    return shape, p


def pack_mixed(items):
    """[(Shape, SoA presentation dict)] -> AFXP sections back to back, in the order given (a request stream of mixed shapes)"""
    return b"".join(pack_presentations(shape, p) for shape, p in items)


def verify_mixed_wire(ctx, blob):
    """afx_verify_presentations_mixed_wire: statuses of a stream of AFXP sections, in stream order.  ctx may be a Group."""
    import ctypes as C
    from . import check, lib
    n = C.c_size_t(0)
    cap = max(1, len(blob) // 32)   # a record is at least one cell
    status = np.full(cap, 255, np.uint8)
    fn = lib().afx_group_verify_presentations_mixed_wire if hasattr(ctx, "member") else lib().afx_verify_presentations_mixed_wire
    check(fn(ctx.h, blob, len(blob), status.ctypes.data, cap, C.byref(n)))
    return status[:n.value]


def verify_wire(ctx, blob, first=None, n=None):
    """Issuer::verify over one AFXP batch (afx_verify_presentations_wire); ctx may be a Group (its devices take byte ranges of the
    blob); with first/n only those records are verified (afx_verify_presentations_wire_range; the other status bytes stay 255)."""
    import ctypes as C
    from . import check, lib
    cnt = C.c_size_t(0)
    cap = max(1, len(blob) // 32)
    status = np.full(cap, 255, np.uint8)
    if first is not None:
        check(lib().afx_verify_presentations_wire_range(ctx.h, blob, len(blob), first, n, status.ctypes.data, cap, C.byref(cnt)))
    elif hasattr(ctx, "member"):
        check(lib().afx_group_verify_presentations_wire(ctx.h, blob, len(blob), status.ctypes.data, cap, C.byref(cnt)))
    else:
        check(lib().afx_verify_presentations_wire(ctx.h, blob, len(blob), status.ctypes.data, cap, C.byref(cnt)))
    return status[:cnt.value]


# ---- CredentialIssuance batches ("AFXI" v1) -------------------------------------------------------
def pack_issuances(kinds, values, iss):
    """kinds: AFX_ATTR_* per position; values [n,count,32]; iss: dict t,U,V,challenge [count,32], responses [nr,count,32]"""
    n = len(kinds)
    values = np.asarray(values, dtype=np.uint8).reshape(n, -1, 32) if n else np.zeros((0, iss["t"].shape[0], 32), np.uint8)
    count, nr = iss["t"].shape[0], iss["responses"].shape[0]
    cols = [iss["t"][None], iss["U"][None], iss["V"][None], iss["challenge"][None], iss["responses"], values]
    soa = np.concatenate([np.asarray(c, dtype=np.uint8) for c in cols], axis=0)
    cells = 4 + nr + n
    assert soa.shape == (cells, count, 32)
    h = b"AFXI" + struct.pack("<5I", 1, count, cells, n, nr) + bytes(kinds)
    h += bytes(-len(h) % 32)
    return h + np.ascontiguousarray(soa.transpose(1, 0, 2)).tobytes()


def unpack_issuances(blob):
    """wire bytes -> (kinds, values [n,count,32], issuance dict)"""
    assert blob[:4] == b"AFXI"
    ver, count, cells, n, nr = struct.unpack("<5I", blob[4:24])
    assert ver == 1 and cells == 4 + nr + n
    kinds = list(blob[24:24 + n])
    o = (24 + n + 31) & ~31
    rec = np.frombuffer(blob, dtype=np.uint8, offset=o).reshape(count, cells, 32).transpose(1, 0, 2)
    c = lambda a: np.ascontiguousarray(a)
    iss = {"t": c(rec[0]), "U": c(rec[1]), "V": c(rec[2]), "challenge": c(rec[3]), "responses": c(rec[4:4 + nr])}
    return kinds, c(rec[4 + nr:]), iss


def issuance_section_bytes(blob):
    """afx_issuance_wire_section_bytes: the length of the AFXI section at the start of blob (AfxError if its header is malformed)"""
    import ctypes as C
    from . import check, lib
    n = C.c_size_t(0)
    check(lib().afx_issuance_wire_section_bytes(blob, len(blob), C.byref(n)))
    return n.value


def verify_issuances_stream(ctx, blob):
    """afx_verify_issuances_mixed_wire (afx_group_verify_issuances_mixed_wire for a Group): CredentialIssuance::verify over a stream of
    AFXI sections, as issue_wire returns it.  Returns the status per issuance, in stream order."""
    import ctypes as C
    from . import check, lib
    n = C.c_size_t(0)
    cap = max(1, len(blob) // 128)   # a record is at least four cells
    status = np.full(cap, 255, np.uint8)
    fn = lib().afx_group_verify_issuances_mixed_wire if hasattr(ctx, "member") else lib().afx_verify_issuances_mixed_wire
    check(fn(ctx.h, blob, len(blob), status.ctypes.data, cap, C.byref(n)))
    return status[:n.value]


def show_wire(ctx, items):
    """afx_show_wire (afx_group_show_wire for a Group): AnonymousCredential::show into AFXP bytes.  items as for batch.show_mixed.
    Returns (one AFXP section per item, back to back; [Shape per item]; status in the caller's order)."""
    import ctypes as C
    from . import ShowGroup, check, lib
    from .batch import _positions, _show_args
    arr = (ShowGroup * max(1, len(items)))()
    keep, counts = [], []
    for g, it in enumerate(items):
        cs, kp, rnd, _, _, cnt, k = _show_args(it["kinds"], it["values"], it["t"], it["U"], it["V"], it.get("keypairs"), it["z_wide"], it["rng_seed"],
                                               it.get("enc_seeds"), it.get("M2"), it.get("m3"), outputs=False)
        arr[g].creds, arr[g].rnd, arr[g].count = cs, rnd, cnt
        if kp is not None:
            arr[g].keypairs = C.pointer(kp)
        keep.append((k, kp))
        counts.append(cnt)
    pos, total = _positions(list(zip(items, counts)))
    total = max([total] + [int(p.max()) + 1 for p in pos if p.size])
    for g, p in enumerate(pos):
        arr[g].positions = p.ctypes.data_as(C.POINTER(C.c_uint64))
    fn = lib().afx_group_show_wire if hasattr(ctx, "member") else lib().afx_show_wire
    out_len = C.c_size_t(0)
    check(fn(ctx.h, arr, len(items), None, 0, C.byref(out_len), None, 0))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, total), 255, np.uint8)
    check(fn(ctx.h, arr, len(items), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, total))
    shapes = [Shape.from_buffer_copy(bytes(arr[g].shape_out)) for g in range(len(items))]
    return out[:out_len.value].tobytes(), shapes, status[:total]


def _device_rng(seed, stream):
    from . import DeviceRng
    if seed is not None:
        seed = bytes(seed)
        assert len(seed) == 32, "a device-rng seed is 32 bytes"
    return DeviceRng(seed, stream)


def rng_expand(ctx, label, first, count, seed=None, stream=0):
    """afx_rng_expand: draw(seed, stream, first + i, label) for i < count -> [count, AFX_DRAW_BYTES(label)] uint8 (seed None: one from
    getrandom, which the caller never sees)"""
    import ctypes as C
    from . import check, draw_bytes, lib
    out = np.zeros((max(1, count), draw_bytes(label)), np.uint8)
    rng = _device_rng(seed, stream)
    check(lib().afx_rng_expand(ctx.h, C.byref(rng), label, first, count, out.ctypes.data))
    return out[:count]


def show_wire_rng(ctx, items, seed=None, stream=0):
    """afx_show_wire_rng (afx_group_show_wire_rng for a Group): show_wire with z_wide, rng_seed and enc_seeds drawn on the device from
    (seed, stream) at each credential's ordinal over the items; items need no randomness arrays"""
    import ctypes as C
    from . import ShowGroup, check, lib
    from .batch import _positions, _show_args
    arr = (ShowGroup * max(1, len(items)))()
    keep, counts = [], []
    for g, it in enumerate(items):
        nsp = sum(1 for k in it["kinds"] if k == 4)
        dummy64, dummy32 = np.zeros((1, 64), np.uint8), np.zeros((1, 32), np.uint8)   # (not read)
        cs, kp, rnd, _, _, cnt, k = _show_args(it["kinds"], it["values"], it["t"], it["U"], it["V"], it.get("keypairs"), dummy64, dummy32,
                                               np.zeros((max(1, nsp), 1, 32), np.uint8), it.get("M2"), it.get("m3"), outputs=False)
        arr[g].creds, arr[g].count = cs, cnt
        if kp is not None:
            arr[g].keypairs = C.pointer(kp)
        keep.append((k, kp))
        counts.append(cnt)
    pos, total = _positions(list(zip(items, counts)))
    total = max([total] + [int(p.max()) + 1 for p in pos if p.size])
    for g, p in enumerate(pos):
        arr[g].positions = p.ctypes.data_as(C.POINTER(C.c_uint64))
    fn = lib().afx_group_show_wire_rng if hasattr(ctx, "member") else lib().afx_show_wire_rng
    rng = _device_rng(seed, stream)
    out_len = C.c_size_t(0)
    check(fn(ctx.h, arr, len(items), C.byref(rng), None, 0, C.byref(out_len), None, 0))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, total), 255, np.uint8)
    check(fn(ctx.h, arr, len(items), C.byref(rng), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, total))
    shapes = [Shape.from_buffer_copy(bytes(arr[g].shape_out)) for g in range(len(items))]
    return out[:out_len.value].tobytes(), shapes, status[:total]


# ---- CredentialRequest batches ("AFXR" v1) and Issuer::issue over them --------------------------------
def pack_requests(kinds, values):
    """kinds: AFX_ATTR_* per position; values [n,count,32] -> one AFXR section"""
    n = len(kinds)
    values = np.asarray(values, dtype=np.uint8)
    assert values.ndim == 3 and values.shape[0] == n and values.shape[2] == 32
    count = values.shape[1]
    h = b"AFXR" + struct.pack("<4I", 1, count, n, n) + bytes(kinds)
    h += bytes(-len(h) % 32)
    return h + np.ascontiguousarray(values.transpose(1, 0, 2)).tobytes()


def unpack_requests(blob):
    """one AFXR section -> (kinds, values [n,count,32])"""
    assert blob[:4] == b"AFXR"
    ver, count, cells, n = struct.unpack("<4I", blob[4:20])
    assert ver == 1 and cells == n
    kinds = list(blob[20:20 + n])
    o = (20 + n + 31) & ~31
    assert len(blob) == o + count * n * 32
    rec = np.frombuffer(blob, dtype=np.uint8, count=count * n * 32, offset=o).reshape(count, n, 32)
    return kinds, np.ascontiguousarray(rec.transpose(1, 0, 2))


def issue_wire(ctx, blob, rnd):
    """afx_issue_wire (afx_group_issue_wire for a Group): a stream of AFXR sections -> (AFXI response bytes, status per request in
    stream order).  rnd: dict t_wide [count,64], U_wide [count,64], rng_seed [count,32] in stream order."""
    import ctypes as C
    from . import IssueRandomness, check, lib
    fn = lib().afx_group_issue_wire if hasattr(ctx, "member") else lib().afx_issue_wire
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    check(fn(ctx.h, blob, len(blob), None, None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    arrs = {k: np.ascontiguousarray(rnd[k], dtype=np.uint8) for k in ("t_wide", "U_wide", "rng_seed")}
    for k, w in (("t_wide", 64), ("U_wide", 64), ("rng_seed", 32)):
        assert arrs[k].size >= cnt.value * w, k
    r = IssueRandomness(arrs["t_wide"].ctypes.data, arrs["U_wide"].ctypes.data, arrs["rng_seed"].ctypes.data)
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, cnt.value), 255, np.uint8)
    check(fn(ctx.h, blob, len(blob), C.byref(r), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, status.size, C.byref(cnt)))
    return out[:out_len.value].tobytes(), status[:cnt.value]


def issue_wire_rng(ctx, blob, seed=None, stream=0):
    """afx_issue_wire_rng (afx_group_issue_wire_rng for a Group): issue_wire with t_wide, U_wide and rng_seed drawn on the device from
    (seed, stream) at each request's index in the stream -> (AFXI response bytes, status per request in stream order)"""
    import ctypes as C
    from . import check, lib
    fn = lib().afx_group_issue_wire_rng if hasattr(ctx, "member") else lib().afx_issue_wire_rng
    rng = _device_rng(seed, stream)
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    check(fn(ctx.h, blob, len(blob), C.byref(rng), None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, cnt.value), 255, np.uint8)
    check(fn(ctx.h, blob, len(blob), C.byref(rng), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, status.size, C.byref(cnt)))
    return out[:out_len.value].tobytes(), status[:cnt.value]


# ---- batchable presentations ("AFXB" v1: every challenge replaced by the proof's commitments) ------
def batchable_header(shape, n_main, count):
    n, nr, hs, ne = shape.n_attributes, shape.n_responses, shape.n_hidden_scalars, shape.n_enc_proofs
    pub = sum(1 for i in range(n) if shape.kinds[i] in (0, 2))
    cells = n_main + nr + 3 + n + pub + 18 * ne
    h = b"AFXB" + struct.pack("<8I", 1, count, cells, n, nr, hs, ne, n_main)
    h += bytes(shape.kinds[:n])
    h += b"".join(struct.pack("<H", shape.hidden_scalar_indices[i]) for i in range(hs))
    h += b"".join(struct.pack("<H", shape.enc_indices[i]) for i in range(ne))
    h += bytes(-len(h) % 32)
    return h, cells


def pack_batchable(shape, p, cm):
    """SoA presentation dict and commitments dict(main [n_main,count,32], enc [[5,count,32] per proof]) -> AFXB bytes"""
    count = p["responses"].shape[1]
    n, n_main = shape.n_attributes, cm["main"].shape[0]
    cols = [cm["main"], p["responses"], p["C_x_0"][None], p["C_x_1"][None], p["C_V"][None], p["C_y"]]
    cols += [p["attr_values"][i][None] for i in range(n) if shape.kinds[i] in (0, 2)]
    for d, c in zip(p["enc"], cm["enc"]):
        cols += [c] + [d[f] if d[f].ndim == 3 else d[f][None] for f in ENC_ORDER[1:]]
    soa = np.concatenate([np.asarray(c, dtype=np.uint8) for c in cols], axis=0)      # [cells, count, 32]
    h, cells = batchable_header(shape, n_main, count)
    assert soa.shape == (cells, count, 32)
    return h + np.ascontiguousarray(soa.transpose(1, 0, 2)).tobytes()


def unpack_batchable(blob):
    """AFXB bytes -> (Shape, SoA presentation dict without challenges, commitments dict)"""
    assert blob[:4] == b"AFXB"
    ver, count, cells, n, nr, hs, ne, n_main = struct.unpack("<8I", blob[4:36])
    assert ver == 1
    shape = Shape()
    shape.n_attributes, shape.n_responses, shape.n_hidden_scalars, shape.n_enc_proofs = n, nr, hs, ne
    o = 36
    for i in range(n):
        shape.kinds[i] = blob[o + i]
    o += n
    for i in range(hs):
        shape.hidden_scalar_indices[i] = struct.unpack("<H", blob[o:o + 2])[0]
        o += 2
    for i in range(ne):
        shape.enc_indices[i] = struct.unpack("<H", blob[o:o + 2])[0]
        o += 2
    o = (o + 31) & ~31
    rec = np.frombuffer(blob, dtype=np.uint8, offset=o, count=count * cells * 32).reshape(count, cells, 32).transpose(1, 0, 2)
    it = iter(range(cells))
    take = lambda k: np.ascontiguousarray(np.stack([rec[next(it)] for _ in range(k)])) if k else np.zeros((0, count, 32), np.uint8)
    cm = {"main": take(n_main), "enc": []}
    p = {"challenge": None, "responses": take(nr), "C_x_0": take(1)[0], "C_x_1": take(1)[0], "C_V": take(1)[0], "C_y": take(n)}
    av = np.zeros((n, count, 32), np.uint8)
    for i in range(n):
        if shape.kinds[i] in (0, 2):
            av[i] = take(1)[0]
    p["attr_values"] = av
    p["enc"] = []
    for _ in range(ne):
        cm["enc"].append(take(5))
        d = {"challenge": None}
        d.update({f: (take(6) if f == "responses" else take(1)[0]) for f in ENC_ORDER[1:]})
        p["enc"].append(d)
    return shape, p, cm


def verify_batchable_wire(ctx, blob, seed=None, stream=0):
    """afx_verify_presentations_batchable_wire: statuses of a stream of AFXB sections, in stream order.  seed: 32 bytes for a
    reproducible run; None: the library reads one from getrandom."""
    import ctypes as C
    from . import check, lib
    n = C.c_size_t(0)
    cap = max(1, len(blob) // 32)
    status = np.full(cap, 255, np.uint8)
    rng = _device_rng(seed, stream)
    check(lib().afx_verify_presentations_batchable_wire(ctx.h, blob, len(blob), C.byref(rng), status.ctypes.data, cap, C.byref(n)))
    return status[:n.value]


def show_batchable_wire(ctx, items):
    """afx_show_batchable_wire: AnonymousCredential::show into AFXB bytes.  items as for batch.show_mixed.
    Returns (one AFXB section per item, back to back; [Shape per item]; status in the caller's order)."""
    import ctypes as C
    from . import ShowGroup, check, lib
    from .batch import _positions, _show_args
    arr = (ShowGroup * max(1, len(items)))()
    keep, counts = [], []
    for g, it in enumerate(items):
        cs, kp, rnd, _, _, cnt, k = _show_args(it["kinds"], it["values"], it["t"], it["U"], it["V"], it.get("keypairs"), it["z_wide"], it["rng_seed"],
                                               it.get("enc_seeds"), it.get("M2"), it.get("m3"), outputs=False)
        arr[g].creds, arr[g].rnd, arr[g].count = cs, rnd, cnt
        if kp is not None:
            arr[g].keypairs = C.pointer(kp)
        keep.append((k, kp))
        counts.append(cnt)
    pos, total = _positions(list(zip(items, counts)))
    total = max([total] + [int(p.max()) + 1 for p in pos if p.size])
    for g, p in enumerate(pos):
        arr[g].positions = p.ctypes.data_as(C.POINTER(C.c_uint64))
    fn = lib().afx_show_batchable_wire
    out_len = C.c_size_t(0)
    check(fn(ctx.h, arr, len(items), None, 0, C.byref(out_len), None, 0))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, total), 255, np.uint8)
    check(fn(ctx.h, arr, len(items), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, total))
    shapes = [Shape.from_buffer_copy(bytes(arr[g].shape_out)) for g in range(len(items))]
    return out[:out_len.value].tobytes(), shapes, status[:total]


# ---- blind issuance on bytes: requests ("AFXQ" v1) in, issuances ("AFXJ" v1) out -------------------
def _blind_header(magic, kinds, count, cells, n_responses):
    h = magic + struct.pack("<5I", 1, count, cells, len(kinds), n_responses) + bytes(kinds)
    return h + bytes(-len(h) % 32)


def pack_blind_requests(kinds, values, req):
    """kinds: AFX_ATTR_* per position; values [n,count,32] (the rows of hidden positions are not read); req: the dict batch.blind_request
    returns (D, challenge [count,32]; A, B [h,count,32]; responses [1+h+hs,count,32]) -> one AFXQ section"""
    from .batch import blind_layout
    n = len(kinds)
    h, hs = blind_layout(kinds)
    count = np.asarray(req["D"]).shape[0]
    u8 = lambda a, rows: np.asarray(a, dtype=np.uint8).reshape(rows, count, 32)
    cols = [u8(req["D"], 1), u8(req["A"], h), u8(req["B"], h), u8(req["challenge"], 1), u8(req["responses"], 1 + h + hs)]
    if n > h:
        values = u8(values, n)
        cols += [values[i][None] for i in range(n) if kinds[i] not in (1, 4)]
    soa = np.concatenate(cols, axis=0)
    cells = 3 + 2 * h + hs + n
    assert soa.shape == (cells, count, 32)
    return _blind_header(b"AFXQ", kinds, count, cells, 1 + h + hs) + np.ascontiguousarray(soa.transpose(1, 0, 2)).tobytes()


def unpack_blind_requests(blob):
    """one AFXQ section -> (kinds, values [n,count,32] with zeros in the rows of hidden positions, request dict)"""
    from .batch import blind_layout
    assert blob[:4] == b"AFXQ"
    ver, count, cells, n, nr = struct.unpack("<5I", blob[4:24])
    kinds = list(blob[24:24 + n])
    h, hs = blind_layout(kinds)
    assert ver == 1 and nr == 1 + h + hs and cells == 3 + 2 * h + hs + n
    o = (24 + n + 31) & ~31
    assert len(blob) == o + count * cells * 32
    rec = np.frombuffer(blob, dtype=np.uint8, count=count * cells * 32, offset=o).reshape(count, cells, 32).transpose(1, 0, 2)
    c = lambda a: np.ascontiguousarray(a)
    req = {"D": c(rec[0]), "A": c(rec[1:1 + h]), "B": c(rec[1 + h:1 + 2 * h]), "challenge": c(rec[1 + 2 * h]), "responses": c(rec[2 + 2 * h:2 + 2 * h + nr])}
    values = np.zeros((n, count, 32), np.uint8)
    at = 2 + 2 * h + nr
    for i in range(n):
        if kinds[i] not in (1, 4):
            values[i] = rec[at]
            at += 1
    return kinds, values, req


def pack_blind_issuances(kinds, iss):
    """kinds: the layout the issuances answer; iss: the dict batch.issue_blind returns (t, U, S1, S2, challenge [count,32], responses
    [nr,count,32]) -> one AFXJ section"""
    count, nr = np.asarray(iss["t"]).shape[0], np.asarray(iss["responses"]).shape[0]
    cols = [np.asarray(iss[f], dtype=np.uint8).reshape(1, count, 32) for f in ("t", "U", "S1", "S2", "challenge")]
    cols.append(np.asarray(iss["responses"], dtype=np.uint8).reshape(nr, count, 32))
    soa = np.concatenate(cols, axis=0)
    return _blind_header(b"AFXJ", kinds, count, 5 + nr, nr) + np.ascontiguousarray(soa.transpose(1, 0, 2)).tobytes()


def unpack_blind_issuances(blob):
    """one AFXJ section -> (kinds, the issuance dict batch.unblind_issuances takes)"""
    assert blob[:4] == b"AFXJ"
    ver, count, cells, n, nr = struct.unpack("<5I", blob[4:24])
    assert ver == 1 and cells == 5 + nr
    kinds = list(blob[24:24 + n])
    o = (24 + n + 31) & ~31
    assert len(blob) == o + count * cells * 32
    rec = np.frombuffer(blob, dtype=np.uint8, count=count * cells * 32, offset=o).reshape(count, cells, 32).transpose(1, 0, 2)
    c = lambda a: np.ascontiguousarray(a)
    return kinds, {"t": c(rec[0]), "U": c(rec[1]), "S1": c(rec[2]), "S2": c(rec[3]), "challenge": c(rec[4]), "responses": c(rec[5:5 + nr])}


def blind_section_bytes(blob):
    """the length of the AFXQ or AFXJ section at the start of blob (AfxError if its header is malformed or it runs past the end)"""
    import ctypes as C
    from . import check, lib
    n = C.c_size_t(0)
    fn = lib().afx_blind_issuance_wire_section_bytes if blob[:4] == b"AFXJ" else lib().afx_blind_request_wire_section_bytes
    check(fn(blob, len(blob), C.byref(n)))
    return n.value


def issue_blind_wire(ctx, blob, rnd):
    """afx_issue_blind_wire (afx_group_issue_blind_wire for a Group): a stream of AFXQ sections -> (AFXJ bytes, status per request in
    stream order).  rnd: dict t_wide, U_wide, rprime_wide [count,64], rng_seed [count,32] in stream order."""
    import ctypes as C
    from . import BlindIssueRandomness, check, lib
    fn = lib().afx_group_issue_blind_wire if hasattr(ctx, "member") else lib().afx_issue_blind_wire
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    check(fn(ctx.h, blob, len(blob), None, None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    names = (("t_wide", 64), ("U_wide", 64), ("rprime_wide", 64), ("rng_seed", 32))
    arrs = {k: np.ascontiguousarray(rnd[k], dtype=np.uint8) for k, _ in names}
    for k, w in names:
        assert arrs[k].size >= cnt.value * w, k
        if arrs[k].size == 0:          # (an empty stream: the call still refuses a NULL array)
            arrs[k] = np.zeros(w, np.uint8)
    r = BlindIssueRandomness(*(arrs[k].ctypes.data for k, _ in names))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, cnt.value), 255, np.uint8)
    check(fn(ctx.h, blob, len(blob), C.byref(r), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, status.size, C.byref(cnt)))
    return out[:out_len.value].tobytes(), status[:cnt.value]


def issue_blind_wire_rng(ctx, blob, seed=None, stream=0):
    """afx_issue_blind_wire_rng (afx_group_issue_blind_wire_rng for a Group): issue_blind_wire with t_wide, U_wide, rprime_wide and
    rng_seed drawn on the device from (seed, stream) at each request's index in the stream"""
    import ctypes as C
    from . import check, lib
    fn = lib().afx_group_issue_blind_wire_rng if hasattr(ctx, "member") else lib().afx_issue_blind_wire_rng
    rng = _device_rng(seed, stream)
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    check(fn(ctx.h, blob, len(blob), C.byref(rng), None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, cnt.value), 255, np.uint8)
    check(fn(ctx.h, blob, len(blob), C.byref(rng), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, status.size, C.byref(cnt)))
    return out[:out_len.value].tobytes(), status[:cnt.value]


def verify_blind_requests_wire(ctx, blob):
    """afx_verify_blind_requests_wire: the status of every request of a stream of AFXQ sections, in stream order"""
    import ctypes as C
    from . import check, lib
    n = C.c_size_t(0)
    cap = max(1, len(blob) // 96)   # a record is at least three cells
    status = np.full(cap, 255, np.uint8)
    check(lib().afx_verify_blind_requests_wire(ctx.h, blob, len(blob), status.ctypes.data, cap, C.byref(n)))
    return status[:n.value]


# ---- blind issuance on bytes, the user's doors: columns -> AFXQ, AFXJ -> t, U, V ---------------------
def _blind_request_groups(groups, explicit):
    """groups: dicts kinds, values [n,count,32] and, for the explicit door, d [count,32], r_wide [h,count,64], rng_seed [count,32]
    -> (afx_blind_request_group array, the arrays it points into)"""
    from . import BlindRequestGroup, BlindRequestRandomness
    from .batch import _blind_attrs, _hptr
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    arr = (BlindRequestGroup * max(1, len(groups)))()
    keep = []
    for g, it in enumerate(groups):
        values = u8(it["values"])
        arr[g].attrs = _blind_attrs(list(it["kinds"]), values, _hptr)
        arr[g].count = int(it["count"]) if "count" in it else values.shape[1]
        keep.append(values)
        if explicit:
            d, r_wide, rng_seed = u8(it["d"]), u8(it["r_wide"]), u8(it["rng_seed"])
            arr[g].d = _hptr(d)
            arr[g].rnd = BlindRequestRandomness(_hptr(r_wide), _hptr(rng_seed))
            keep += [d, r_wide, rng_seed]
    return arr, keep


def blind_request_wire(ctx, groups):
    """afx_blind_request_wire (afx_group_blind_request_wire for a Group): afx_blind_request over groups of columns -> (one AFXQ section
    per group, back to back; status per item in stream order).  groups: dicts kinds, values [n,count,32], d [count,32], r_wide
    [h,count,64], rng_seed [count,32]."""
    import ctypes as C
    from . import check, lib
    fn = lib().afx_group_blind_request_wire if hasattr(ctx, "member") else lib().afx_blind_request_wire
    arr, keep = _blind_request_groups(groups, True)
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    check(fn(ctx.h, arr, len(groups), None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, cnt.value), 255, np.uint8)
    check(fn(ctx.h, arr, len(groups), out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, status.size, C.byref(cnt)))
    return out[:out_len.value].tobytes(), status[:cnt.value]


def blind_request_wire_rng(ctx, groups, seed=None, stream=0, keep_d=True):
    """afx_blind_request_wire_rng (its group form for a Group): blind_request_wire with d, r_wide and rng_seed drawn on the device from
    (seed, stream) at each item's index in the stream; groups need kinds and values only.  Returns (AFXQ bytes, status, d [total,32] -
    None with keep_d=False, which needs a seed: unblind_issuances_wire_rng derives d again from it)."""
    import ctypes as C
    from . import check, lib
    fn = lib().afx_group_blind_request_wire_rng if hasattr(ctx, "member") else lib().afx_blind_request_wire_rng
    arr, keep = _blind_request_groups(groups, False)
    rng = _device_rng(seed, stream)
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    check(fn(ctx.h, arr, len(groups), C.byref(rng), None, None, 0, C.byref(out_len), None, 0, C.byref(cnt)))
    out = np.zeros(max(1, out_len.value), np.uint8)
    status = np.full(max(1, cnt.value), 255, np.uint8)
    d = np.zeros((max(1, cnt.value), 32), np.uint8) if keep_d else None
    check(fn(ctx.h, arr, len(groups), C.byref(rng), d.ctypes.data if keep_d else None, out.ctypes.data, out.size, C.byref(out_len), status.ctypes.data, status.size,
             C.byref(cnt)))
    return out[:out_len.value].tobytes(), status[:cnt.value], (d[:cnt.value] if keep_d else None)


def _credential_out(total):
    from . import CredentialOut
    o = {k: np.zeros((max(1, total), 32), np.uint8) for k in ("t", "U", "V")}
    return o, CredentialOut(*(o[k].ctypes.data for k in ("t", "U", "V")))


def unblind_issuances_wire(ctx, issuances, requests, d):
    """afx_unblind_issuances_wire (its group form for a Group): a stream of AFXJ sections, the AFXQ stream they answer and d [total,32]
    in stream order -> (dict(t, U, V) [total,32] each: the credentials' t, U, V; status per item)"""
    import ctypes as C
    from . import check, lib
    fn = lib().afx_group_unblind_issuances_wire if hasattr(ctx, "member") else lib().afx_unblind_issuances_wire
    d = np.ascontiguousarray(d, dtype=np.uint8)
    total = max(d.size // 32, len(issuances) // 160)   # (an AFXJ record is at least five cells)
    o, co = _credential_out(total)
    status = np.full(max(1, total), 255, np.uint8)
    cnt = C.c_size_t(0)
    check(fn(ctx.h, issuances, len(issuances), requests, len(requests), d.ctypes.data if d.size else None, C.byref(co), status.ctypes.data, min(total, d.size // 32),
             C.byref(cnt)))
    return {k: v[:cnt.value] for k, v in o.items()}, status[:cnt.value]


def unblind_issuances_wire_rng(ctx, issuances, requests, seed, stream=0):
    """afx_unblind_issuances_wire_rng (its group form for a Group): unblind_issuances_wire with d derived again on the device from the
    (seed, stream) blind_request_wire_rng drew it from"""
    import ctypes as C
    from . import check, lib
    fn = lib().afx_group_unblind_issuances_wire_rng if hasattr(ctx, "member") else lib().afx_unblind_issuances_wire_rng
    rng = _device_rng(seed, stream)
    total = len(issuances) // 160
    o, co = _credential_out(total)
    status = np.full(max(1, total), 255, np.uint8)
    cnt = C.c_size_t(0)
    check(fn(ctx.h, issuances, len(issuances), requests, len(requests), C.byref(rng), C.byref(co), status.ctypes.data, total, C.byref(cnt)))
    return {k: v[:cnt.value] for k, v in o.items()}, status[:cnt.value]
