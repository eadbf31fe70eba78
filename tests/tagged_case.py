"""One 300-item case per layout for the tagged-presentation GPU tests (tests/test_gpu_tagged.py, tests/test_gpu_tagged_forgeries.py):
system parameters and the issuer key from the oracle, credentials issued by the engine on values chosen here, and every draw of a
tagged show.  Counts 1, 70 and 300 take the case's first items.

The hidden scalar at the tag's position p and the counter n of the first three items are chosen:
  item 0   m + n == 1              T == H
  item 1   m + n == l - 1          T == -H
  item 2   m == l - 1, n == 1      s == 0: the item must fail, with zeros in every output row
the rest are random, with n < 2^32."""
import hashlib

import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
# (credential kinds AFX_ATTR_*, p).  The 8-attribute layout is the C3 layout of bench.py (S S P P E E E E) with both scalars hidden as
# well as the four plaintext attributes; p is its last hidden scalar.
LAYOUTS = [([1], 0), ([1, 0, 2, 4], 0), ([1, 1, 2, 2, 4, 4, 4, 4], 1)]
STRICT_LAYOUTS = [([4, 1, 0], 1)]
COUNTS = (1, 70, 300)
TOTAL = 300
SAMPLE = (0, 1, 3, 4, 5, 6, 7, 63, 64, 69, 255, 256, 299)      # items whose tag bytes are compared with the yardstick
FAILING = 2
SCOPE = b"tests/tagged_case: scope one"


def sc(x):
    return np.frombuffer(int(x % L).to_bytes(32, "little"), np.uint8)


def to_int(row):
    return int.from_bytes(bytes(row), "little")


class Case:
    def __init__(self, kinds, p, strict=False):
        import aeonflux_amd as afx
        import oracle
        from aeonflux_amd import batch
        self.kinds, self.p, self.n, self.strict = list(kinds), p, len(kinds), strict
        n, cnt = self.n, TOTAL
        stream = hashlib.shake_256(b"tagged case %s %d" % (bytes(kinds), p)).digest(1 << 16)
        self.params, used = oracle.system_parameters_generate(n, stream)
        self.key, self.ip = oracle.issuer_new(self.params, stream[used:used + 64 * (4 + n)])
        self.issuer = afx.Context(self.params, self.key, self.ip)
        self.user = afx.Context(self.params, None, self.ip)
        for c in (self.issuer, self.user):
            c.set_strict(1 if strict else 0)
        rng = np.random.default_rng(to_int(hashlib.sha256(bytes(kinds) + bytes([p])).digest()[:8]))
        self.rb = rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
        values, M2, m3 = (np.zeros((n, cnt, 32), np.uint8) for _ in range(3))
        for i, k in enumerate(kinds):
            if k in (0, 1):
                values[i] = batch.scalars_from_wide(self.issuer, rb(cnt, 64))
            else:
                values[i] = batch.points_from_uniform(self.issuer, rb(cnt, 64))
                if k == 4:
                    M2[i] = batch.points_from_uniform(self.issuer, rb(cnt, 64))
                    m3[i] = batch.scalars_from_wide(self.issuer, rb(cnt, 64))
        nonce = np.zeros((cnt, 32), np.uint8)
        nonce[:, :4] = rb(cnt, 4)
        nonce[0], values[p][0] = sc(5), sc(1 - 5)
        nonce[1], values[p][1] = sc(7), sc(L - 1 - 7)
        nonce[2], values[p][2] = sc(1), sc(L - 1)
        self.values, self.M2, self.m3, self.nonce = values, M2, m3, nonce
        self.m = [to_int(values[p][i]) for i in range(cnt)]
        self.nn = [to_int(nonce[i]) for i in range(cnt)]
        assert (self.m[0] + self.nn[0]) % L == 1 and (self.m[1] + self.nn[1]) % L == L - 1 and (self.m[2] + self.nn[2]) % L == 0
        issue_kinds = [{1: 0, 4: 3}.get(k, k) for k in kinds]
        iss, st = batch.issue(self.issuer, issue_kinds, values, rb(cnt, 64), rb(cnt, 64), rb(cnt, 32))
        assert not st.any()
        self.t, self.U, self.V = iss["t"], iss["U"], iss["V"]
        self.nsp = sum(1 for k in kinds if k == 4)
        self.hs = sum(1 for k in kinds if k == 1)
        self.keypairs = None
        if self.nsp:
            g = max(3, n)
            gen = lambda idx: np.frombuffer(self.params[4 + 32 * idx:4 + 32 * idx + 32], np.uint8)
            a, a0, a1 = (batch.scalars_from_wide(self.issuer, rb(cnt, 64)) for _ in range(3))
            pk, ok = batch.multiscalar_mul(self.issuer, np.stack([a, a0, a1]), np.stack([np.broadcast_to(gen(5 + g + n + 1 + k), (cnt, 32)) for k in range(3)]))
            assert ok.all()
            self.keypairs = dict(a=a, a0=a0, a1=a1, pk=pk)
        self.draws = self.fresh_draws()
        self.H = batch.tag_scope_generator(self.user, SCOPE)
        self.shown = {}

    def fresh_draws(self):
        rb = self.rb
        return dict(z_wide=rb(TOTAL, 64), rng_seed=rb(TOTAL, 32), enc_seeds=rb(max(self.nsp, 1), TOTAL, 32), tag_seed=rb(TOTAL, 32))

    def close(self):
        self.issuer.close()
        self.user.close()

    def cut(self, a, cnt):
        return None if a is None else np.ascontiguousarray(a[..., :cnt, :])

    def show_args(self, cnt, draws=None):
        d = draws or self.draws
        kp = {f: self.cut(v, cnt) for f, v in self.keypairs.items()} if self.keypairs else None
        return dict(kinds=self.kinds, values=self.cut(self.values, cnt), t=self.cut(self.t, cnt), U=self.cut(self.U, cnt), V=self.cut(self.V, cnt), keypairs=kp,
                    z_wide=self.cut(d["z_wide"], cnt), rng_seed=self.cut(d["rng_seed"], cnt), enc_seeds=self.cut(d["enc_seeds"], cnt), M2=self.cut(self.M2, cnt),
                    m3=self.cut(self.m3, cnt))

    def show_tagged(self, cnt, ctx=None, draws=None, H=None):
        """(presentation, tags, shape, status) of the first cnt items"""
        from aeonflux_amd import batch
        a = self.show_args(cnt, draws)
        d = draws or self.draws
        return batch.show_tagged(ctx or self.user, a["kinds"], a["values"], a["t"], a["U"], a["V"], a["keypairs"], a["z_wide"], a["rng_seed"], self.p, H or self.H,
                                 self.cut(self.nonce, cnt), self.cut(d["tag_seed"], cnt), a["enc_seeds"], a["M2"], a["m3"])

    def shown_once(self, cnt):
        if cnt not in self.shown:
            self.shown[cnt] = self.show_tagged(cnt)
        return self.shown[cnt]


def flatten(pres, tags, status):
    """every output array of a tagged show, by name"""
    out = {"pres." + f: pres[f] for f in ("challenge", "responses", "C_x_0", "C_x_1", "C_V", "C_y", "attr_values")}
    for e, d in enumerate(pres["enc"]):
        out.update({"enc%d.%s" % (e, f): v for f, v in d.items()})
    out.update({"tag." + f: v for f, v in tags.items()})
    out["status"] = status
    return out


def item_of(arr, i):
    """item i of a [count, w] or [k, count, w] array"""
    return arr[i] if arr.ndim == 2 else (arr[i:i + 1] if arr.ndim == 1 else arr[:, i])
