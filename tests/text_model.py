"""CPU model of enc_fp_depth / enc_value_depth / enc_text (reference ops/encrypt.hpp:16-27, 162-287;
utils/text.hpp:15-61) over the oracle's primitives (helpers.Oracle: fp, ztag, prf_R, prf_noise_delta,
sigma), with its own compact_edges and shuffle_edges. TEST INFRASTRUCTURE ONLY: the model the ragged
GPU path (pvac_hip_enc_items) is compared with, itself pinned to the reference-minted fixtures of
tests/golden/text by test_text_model.py."""
import json
import math
import os

import numpy as np

from helpers import GOLD, LAYER_DT, Cipher, pack_meta, read_ct, splitmix_stream

TEXT = os.path.join(GOLD, "text")
M63 = (1 << 63) - 1
M64 = (1 << 64) - 1
FP, VALUE = 0, 1
DEFAULT_NOISE = (120.0, 0.55, 16.0)


class Draws:
    """csprng_u64 over a fixed segment; past its end it yields 0 and sets `over` (status 1)."""

    def __init__(self, words):
        self.w = np.asarray(words, np.uint64)
        self.i = 0
        self.over = False

    def next(self):
        if self.i < len(self.w):
            self.i += 1
            return int(self.w[self.i - 1])
        self.over = True
        return 0


def plan_noise(hint, noise=DEFAULT_NOISE, B=337):
    nb, t2, slope = noise
    budget = nb + slope * max(0, hint)
    per2, per3 = 2.0 * math.log2(B), 3.0 * math.log2(B)
    z2 = max(0, int(math.floor((budget * t2) / max(1e-6, per2))))
    z3 = max(0, int(math.floor((budget * (1.0 - t2)) / max(1e-6, per3))))
    if z2 + z3 == 1:
        if z3 > 0:
            z3 += 1
        else:
            z2 += 1
    return z2, z3


class Model:
    def __init__(self, orc, sk, canon, powg, H=None, noise=DEFAULT_NOISE, B=337):
        self.orc, self.sk, self.canon, self.H, self.noise, self.B = orc, sk, canon, H, noise, B
        pg = np.asarray(powg, np.uint64).reshape(-1, 2)
        self.powg = [(int(a), int(b)) for a, b in pg]

    # ---- Fp on (lo, hi) pairs, through the oracle (non-canonical inputs behave as in the reference)
    def _f(self, op, a, b=None):
        al, ah = np.array([a[0]], np.uint64), np.array([a[1]], np.uint64)
        if b is None:
            lo, hi = self.orc.fp(op, al, ah)
        else:
            lo, hi = self.orc.fp(op, al, ah, np.array([b[0]], np.uint64), np.array([b[1]], np.uint64))
        return int(lo[0]), int(hi[0])

    def _rand_fp_nonzero(self, rs):
        while True:
            lo = rs.next()
            hi = rs.next() & M63
            x = self._f("from_words", (lo, hi))
            if x != (0, 0) or rs.over:
                return x

    def enc_fp_depth(self, v, hint, rs, sigma=False):
        """v: (lo, hi) as given. Returns a one-layer Cipher (sigma rows when asked and H is known)."""
        f, B = self._f, self.B
        nlo, nhi = rs.next(), rs.next()
        ztag = self.orc.ztag(self.canon, nlo, nhi)
        seed = (ztag, nlo, nhi)
        idx, ch = [], []
        for _ in range(8):
            while True:
                x = rs.next() % B
                if x not in idx or rs.over:
                    break
            idx.append(x)
            ch.append(rs.next() & 1)
        r = []
        sumg = (0, 0)
        for j in range(7):
            r.append(self._rand_fp_nonzero(rs))
            term = f("mul", r[j], self.powg[idx[j]])
            sumg = f("add", sumg, term) if ch[j] == 0 else f("sub", sumg, term)
        rl = f("mul", f("sub", v, sumg), f("inv", self.powg[idx[7]]))
        r.append(f("neg", rl) if ch[7] == 1 else rl)
        R = self.orc.prf_R(self.sk, self.canon, seed)
        salts = [rs.next() for _ in range(8)]
        z2, z3 = plan_noise(hint, self.noise, B)
        total, gid, dacc = z2 + z3, 0, (0, 0)

        def next_delta(kind):
            nonlocal dacc
            if total - gid <= 1:
                return f("neg", dacc)
            d = self.orc.prf_noise_delta(self.sk, self.canon, seed, gid, kind)
            dacc = f("add", dacc, d)
            return d

        for _ in range(z2):
            i = rs.next() % B
            while True:
                j = rs.next() % B
                if j != i or rs.over:
                    break
            s1 = rs.next() & 1
            D = next_delta(0)
            Dp = D if s1 == 0 else f("neg", D)
            ri = self._rand_fp_nonzero(rs)
            rj = f("mul", f("sub", f("mul", ri, self.powg[i]), Dp), f("inv", self.powg[j]))
            idx += [i, j]
            ch += [s1, s1 ^ 1]
            r += [ri, rj]
            salts += [rs.next(), rs.next()]
            gid += 1
        for _ in range(z3):
            i = rs.next() % B
            while True:
                j = rs.next() % B
                if j != i or rs.over:
                    break
            while True:
                k = rs.next() % B
                if (k != i and k != j) or rs.over:
                    break
            s1, s2, s3 = rs.next() & 1, rs.next() & 1, rs.next() & 1
            D = next_delta(1)
            a, b = self._rand_fp_nonzero(rs), self._rand_fp_nonzero(rs)
            t1, t2 = f("mul", a, self.powg[i]), f("mul", b, self.powg[j])
            if s1:
                t1 = f("neg", t1)
            if s2:
                t2 = f("neg", t2)
            gk = self.powg[k] if s3 == 0 else f("neg", self.powg[k])
            c = f("mul", f("sub", D, f("add", t1, t2)), f("inv", gk))
            idx += [i, j, k]
            ch += [s1, s2, s3]
            r += [a, b, c]
            salts += [rs.next(), rs.next(), rs.next()]
            gid += 1
        n = len(idx)
        rl_, rh_ = np.array([x[0] for x in r], np.uint64), np.array([x[1] for x in r], np.uint64)
        wl, wh = self.orc.fp("mul", rl_, rh_, np.full(n, R[0], np.uint64), np.full(n, R[1], np.uint64))
        # compact_edges: per (idx, ch) the fp_add chain from 0 in creation order and the sigma XOR;
        # output sorted by (idx, P before M)
        groups = {}
        for e in range(n):
            groups.setdefault((idx[e], ch[e]), []).append(e)
        keys = sorted(groups)
        out = []
        for key in keys:
            w = (0, 0)
            s = np.zeros(128, np.uint64) if sigma else None
            for e in groups[key]:
                w = f("add", w, (int(wl[e]), int(wh[e])))
                if sigma:
                    s ^= self.orc.sigma(self.canon, self.H, ztag, nlo, nhi, idx[e], ch[e], salts[e])
            assert w != (0, 0) or (sigma and s.any()), "a merged group vanished: not modelled"
            out.append((key, w, s))
        for i in range(len(out) - 1, 0, -1):   # shuffle_edges
            j = rs.next() % (i + 1)
            out[i], out[j] = out[j], out[i]
        L = np.zeros(1, LAYER_DT)
        L["ztag"], L["nonce_lo"], L["nonce_hi"] = ztag, nlo, nhi
        return Cipher(L, pack_meta(np.zeros(len(out), np.uint64), [k[0] for k, _, _ in out], [k[1] for k, _, _ in out]),
                      [w[0] for _, w, _ in out], [w[1] for _, w, _ in out],
                      np.stack([s for _, _, s in out]) if sigma else None)

    def enc_value_depth(self, v, hint, rs, sigma=False):
        mask = self._rand_fp_nonzero(rs)
        b = self.enc_fp_depth(self._f("neg", mask), hint, rs, sigma)   # the second argument draws first
        a = self.enc_fp_depth(self._f("add", (v & M64, 0), mask), hint, rs, sigma)
        return Cipher(np.concatenate([a.layers, b.layers]), np.concatenate([a.meta, b.meta | np.uint64(1)]),
                      np.concatenate([a.w_lo, b.w_lo]), np.concatenate([a.w_hi, b.w_hi]),
                      np.concatenate([a.sigma, b.sigma]) if sigma else None)

    def enc_item(self, kind, v, hint, words, sigma=False):
        """One item of pvac_hip_enc_items from its draw segment: (Cipher, status 0 / 1)."""
        rs = Draws(words)
        c = self.enc_value_depth(v, hint, rs, sigma) if kind == VALUE else \
            self.enc_fp_depth((v & M64, v >> 64), hint, rs, sigma)
        return c, 1 if rs.over else 0


def text_pack(msg):
    """utils/text.hpp:15-26 restated: 15 little-endian bytes per block as one integer (< 2^120)."""
    return [int.from_bytes(msg[p:p + 15], "little") for p in range(0, len(msg), 15)]


def text_unpack(vals):
    """utils/text.hpp:63-87 restated over decrypted integers: (bytes, flags) with flag bit 0 = the
    length's high word is not 0, bit 1 = the length was clipped to the blocks present."""
    if not vals:
        return b"", 0
    n, flags = vals[0] & M64, 1 if vals[0] >> 64 else 0
    buf = b"".join((v & ((1 << 120) - 1)).to_bytes(15, "little") for v in vals[1:])
    if len(buf) < n:
        n, flags = len(buf), flags | 2
    return buf[:n], flags


def text_items(msg):
    """enc_text's items: (kind, v, hint) for the length, then the blocks with hints 2, 3, ..."""
    return [(VALUE, len(msg), 0)] + [(FP, v, 2 + b) for b, v in enumerate(text_pack(msg))]


# ---- the reference-minted fixtures (tools/mint_text.cpp)
def manifest():
    with open(os.path.join(TEXT, "manifest.json")) as f:
        return json.load(f)


def case_draws(case):
    if case["log_file"]:
        return np.fromfile(os.path.join(TEXT, case["name"] + ".u64"), dtype=np.uint64)
    return splitmix_stream(case["seed"], 0, case["draws"])


def case_ciphers(case):
    if case["sigma"]:
        return read_ct(os.path.join(TEXT, case["name"] + ".ct"))
    out = []
    for p in range(case["parts"]):
        out += read_ct(os.path.join(TEXT, f"{case['name']}_p{p}.ct"))
    return out


def case_noise(case):
    return (case["noise_entropy_bits"], case["tuple2_fraction"], case["depth_slope_bits"])


def case_items(case):
    """(kind, v, hint, off, cnt) per cipher of a fixture case, offsets into case_draws."""
    return [(c["kind"], c["v_lo"] | (c["v_hi"] << 64), c["hint"], c["off"], c["cnt"]) for c in case["ciphers"]]
