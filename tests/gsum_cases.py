"""Inputs for the gsum checker's tests (test_gsum_model.py on the CPU, test_gpu_check.py on the GPU):
base triples (A, B, C, product-slot nonces) and the table of mutations with the status each must
give. C need not come from ct_mul: the checker reads A, B, C and the nonces only, so most triples
here are built by hand with Python integers. TEST INFRASTRUCTURE ONLY."""
import copy

import numpy as np

from gsum_model import layer_gsums
from helpers import LAYER_DT, P, Cipher, pack_meta

M64 = (1 << 64) - 1
# p, p - 1, 2^127, 2^128 - 1, 0, 1, ... as (lo, hi): the non-canonical and edge weights of
# test_gpu_parity's full-range ct_mul tests
SPECIAL_W = [(2**64 - 1, 2**63 - 1), (2**64 - 2, 2**63 - 1), (0, 2**63), (2**64 - 1, 2**64 - 1), (0, 0), (1, 0),
             (1, 2**63), (2**64 - 1, 2**63), (2**63, 2**62), (5, 2**64 - 16)]


class Triple:
    """One pair of the check: A, B, C and nz, the (lo, hi) nonces of the |A.L||B.L| product slots."""

    def __init__(self, A, B, C, nz, name="", plain=True):
        self.A, self.B, self.C = A, B, C
        self.nz = np.ascontiguousarray(nz, np.uint64).reshape(-1, 2)
        self.name = name
        self.plain = plain   # False: a degenerate base on which the mutation classes need not hold

    def copy(self, name=None):
        t = copy.deepcopy(self)
        if name is not None:
            t.name = name
        return t


def powg_from(g, Bm):
    """powg[i] = g^i for i < Bm as (lo, hi) words; g of order Bm for a key's table (g^Bm == 1)."""
    out = np.zeros(2 * Bm, np.uint64)
    x = 1
    for i in range(Bm):
        out[2 * i], out[2 * i + 1] = x & M64, x >> 64
        x = x * g % P
    return out


def powg_int(powg):
    a = np.asarray(powg, np.uint64).reshape(-1, 2)
    return [int(a[i, 0]) | (int(a[i, 1]) << 64) for i in range(len(a))]


def _words(vals):
    return (np.array([v & M64 for v in vals], np.uint64), np.array([v >> 64 for v in vals], np.uint64))


def _layers(rng, n, rule=0):
    L = np.zeros(n, LAYER_DT)
    L["rule"] = rule
    L["ztag"] = rng.integers(0, 2**63, n, dtype=np.uint64)
    L["nonce_lo"] = rng.integers(0, 2**64, n, dtype=np.uint64)
    L["nonce_hi"] = rng.integers(0, 2**64, n, dtype=np.uint64)
    return L


def rand_cipher(rng, nl, Bm, epl=(5, 40), idx_span=24, special=False):
    """nl BASE layers of epl[0]..epl[1] edges each, idx within idx_span of Bm - 1 (sums of two wrap
    mod Bm), canonical weights below p; special: a fifth of the weights from SPECIAL_W instead."""
    lay, cnt = [], rng.integers(epl[0], epl[1] + 1, nl)
    for l in range(nl):
        lay += [l] * int(cnt[l])
    ne = len(lay)
    lay = np.array(lay, np.uint64)[rng.permutation(ne)] if ne else np.zeros(0, np.uint64)
    idx = rng.integers(Bm - idx_span, Bm, ne).astype(np.uint64)
    ch = rng.integers(0, 2, ne).astype(np.uint64)
    lo = rng.integers(0, 2**64, ne, dtype=np.uint64)
    hi = rng.integers(0, 2**63 - 1, ne, dtype=np.uint64)
    if special:
        for e in np.flatnonzero(rng.random(ne) < 0.2):
            lo[e], hi[e] = SPECIAL_W[rng.integers(0, len(SPECIAL_W))]
    return Cipher(_layers(rng, nl), pack_meta(lay, idx, ch), lo, hi)


def product_triple(oracle, rng, la, lb, Bm, name, special=True, epl=(5, 40)):
    """C = the pinned port's ct_mul(A, B) with random slot nonces; B takes the special weights."""
    A = rand_cipher(rng, la, Bm, epl)
    B = rand_cipher(rng, lb, Bm, epl, special=special)
    nz = rng.integers(0, 2**64, (la * lb, 2), dtype=np.uint64)
    return Triple(A, B, oracle.ct_mul(A, B, nz.reshape(-1), Bm=Bm), nz, name)


def hand_triple(oracle, rng, A, B, powg, Bm, name, c_layers=0, plain=True, big=None):
    """C built by hand: copies of A's and B's layers, then, somewhere among filler PROD layers that
    carry no slot's nonce, one PROD layer per slot whose product is nonzero, holding two edges whose
    signed sum is gsum(A, la) gsum(B, lb) (Python integers). Slots with a zero product are absent.
    c_layers: total layers of C (at least what the product layers need). big = (q, n): slot q's
    layer instead gets n edges of one idx and channel plus one closing edge."""
    la, lb = A.nL, B.nL
    nz = rng.integers(0, 2**64, (la * lb, 2), dtype=np.uint64)
    gA, gB = layer_gsums(oracle, A, powg), layer_gsums(oracle, B, powg)
    pg = powg_int(powg)
    want = {q: gA[q // lb] * gB[q % lb] % P for q in range(la * lb)}
    live = [q for q in want if want[q]]
    nC = max(c_layers, la + lb + len(live))
    L = _layers(rng, nC, rule=1)
    L[:la], L[la:la + lb] = A.layers, B.layers
    pos = la + lb + np.sort(rng.choice(nC - la - lb, len(live), replace=False)) if live else []
    lay, idx, ch, w = [], [], [], []
    for l, q in zip(pos, live):
        L[l]["nonce_lo"], L[l]["nonce_hi"] = nz[q]
        L[l]["pa"], L[l]["pb"] = q // lb, la + q % lb
        if big is not None and big[0] == q:
            i1, c1 = int(rng.integers(0, Bm)), int(rng.integers(0, 2))
            ws = [int(x) for x in rng.integers(1, 2**62, big[1])]
            ws = [(x << 64 | x) % P for x in ws]
            s = sum(ws) * pg[i1] % P
        else:
            i1, c1, ws = int(rng.integers(0, Bm)), int(rng.integers(0, 2)), [int(rng.integers(1, 2**62)) << 60 | 5]
            s = ws[0] * pg[i1] % P
        s = s if c1 == 0 else (P - s) % P
        i2 = int(rng.integers(0, Bm))
        w2 = (want[q] - s) * pow(pg[i2], -1, P) % P      # + w2 g^i2 closes the sum
        lay += [l] * (len(ws) + 1)
        idx += [i1] * len(ws) + [i2]
        ch += [c1] * len(ws) + [0]
        w += ws + [w2]
    order = rng.permutation(len(lay))
    lo, hi = _words(w)
    C = Cipher(L, pack_meta(np.array(lay, np.uint64), np.array(idx, np.uint64), np.array(ch, np.uint64))[order]
               if lay else np.zeros(0, np.uint64), lo[order] if lay else lo, hi[order] if lay else hi)
    return Triple(A, B, C, nz, name, plain)


def cancelling_cipher(rng, powg, Bm):
    """Two layers: layer 0 random, layer 1's three edges sum to gsum 0 (w g^i + w' g^j - w'' g^k = 0)."""
    X = rand_cipher(rng, 1, Bm)
    pg = powg_int(powg)
    i, j, k = (int(v) for v in rng.integers(0, Bm, 3))
    w1, w2 = int(rng.integers(1, 2**63)) << 50 | 3, int(rng.integers(1, 2**63)) << 40 | 9
    w3 = (w1 * pg[i] + w2 * pg[j]) * pow(pg[k], -1, P) % P
    lo, hi = _words([w1, w2, w3])
    L = np.concatenate([X.layers, _layers(rng, 1)])
    return Cipher(L, np.concatenate([X.meta, pack_meta([1, 1, 1], [i, j, k], [0, 0, 1])]),
                  np.concatenate([X.w_lo, lo]), np.concatenate([X.w_hi, hi]))


def lds_bases(oracle, rng, powg, Bm):
    """The base triples of the LDS-mode tests, all of status 0."""
    out = [product_triple(oracle, rng, 2, 3, Bm, "mul2x3"), product_triple(oracle, rng, 1, 1, Bm, "mul1x1"),
           product_triple(oracle, rng, 4, 4, Bm, "mul4x4")]
    out.append(hand_triple(oracle, rng, cancelling_cipher(rng, powg, Bm), rand_cipher(rng, 2, Bm), powg, Bm,
                           "cancel"))
    noE = Cipher(_layers(rng, 2), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    out.append(hand_triple(oracle, rng, noE, rand_cipher(rng, 1, Bm), powg, Bm, "A.E=0", plain=False))
    noL = Cipher(_layers(rng, 0), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    out.append(hand_triple(oracle, rng, noL, rand_cipher(rng, 2, Bm), powg, Bm, "A.L=0", plain=False))
    return out


LDS_BUDGET = 160 * 1024 - 16   # include/pvac_hip.h: 163,824 bytes


def table_bytes(Bm, la, lb, lc, lp):
    """The check's per-pair tables as include/pvac_hip.h documents them (pvac_hip_check_mul_gsum):
    seven arrays, each rounded up to 16 bytes. Above LDS_BUDGET the call runs over global slabs."""
    al16 = lambda v: (v + 15) & ~15
    return sum(al16(v) for v in (16 * Bm, 48 * la, 48 * lb, 48 * lc, 4 * lc, 16 * lp, 4 * lp))


def first_slab_layers(Bm, la, lb):
    """The smallest |C.L| at which a batch of (la x lb)-layer pairs leaves LDS."""
    lc = la + lb
    while table_bytes(Bm, la, lb, lc, la * lb) <= LDS_BUDGET:
        lc += 1
    return lc


def slab_bases(oracle, rng, powg, Bm):
    """Base triples whose tables exceed the LDS budget, all of status 0: four product layers among a
    few thousand, the same with ~5,000 edges on one (layer, channel), and a 64 x 48-layer product."""
    lc = first_slab_layers(Bm, 2, 2) + 40
    mk = lambda name, big: hand_triple(oracle, rng, rand_cipher(rng, 2, Bm), rand_cipher(rng, 2, Bm, special=True),
                                       powg, Bm, name, c_layers=lc, big=big)
    return [mk("slab2x2", None), mk("contended", (1, 5000)),
            product_triple(oracle, rng, 64, 48, Bm, "mul64x48", epl=(2, 2))]


_CASES = {}


def key_powg(Bm):
    from pvac_hfhe_cppbyv_amd import powg_table
    return powg_table(Bm)


def cases(oracle, Bm, mode):
    """[(row name, Triple, expected status or None)]: every base of `mode` ("lds" / "slab") as row
    "base" (expected 0) followed by its mutations. Built once per (Bm, mode), from a fixed seed."""
    if (Bm, mode) not in _CASES:
        rng = np.random.default_rng([0x65, Bm, mode == "slab"])
        powg = key_powg(Bm)
        out = []
        for b in (lds_bases if mode == "lds" else slab_bases)(oracle, rng, powg, Bm):
            out.append(("base", b, 0))
            out += list(mutations(oracle, b, rng, powg, Bm))
        _CASES[(Bm, mode)] = out
    return _CASES[(Bm, mode)]


# ----------------------------------------------------------------------------- the mutation table
def _set_edges(X, meta, lo, hi):
    X.meta = np.ascontiguousarray(meta, np.uint64)
    X.w_lo = np.ascontiguousarray(lo, np.uint64)
    X.w_hi = np.ascontiguousarray(hi, np.uint64)


def _wint(X, e):
    return (int(X.w_hi[e]) << 64 | int(X.w_lo[e])) % P


def _live_edges(X):
    """Edges that count: in a layer of X, with a weight that is not 0 mod p."""
    lay = X.layer_id()
    return [e for e in range(X.nE) if lay[e] < X.nL and _wint(X, e)]


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _edged_layers(C):
    lay = C.layer_id()
    return [int(l) for l in np.unique(lay[lay < C.nL])]


def _meta_with(m, layer=None, idx=None, ch=None):
    m = int(m)
    l, i, c = m & 0xFFFFFFFF, (m >> 32) & 0xFFFF, (m >> 48) & 0xFF
    l, i, c = (l if layer is None else layer), (i if idx is None else idx), (c if ch is None else ch)
    return np.uint64(l | i << 32 | c << 48)


def mutations(oracle, base, rng, powg, Bm):
    """Yield (name, mutated Triple, expected status or None) for every row of the table that applies
    to `base`. None: whatever the model says (rows the table leaves to it, and every row on a base
    that is not plain). Each mutated triple is an independent copy."""
    gA, gB = layer_gsums(oracle, base.A, powg), layer_gsums(oracle, base.B, powg)
    lb = max(base.B.nL, 1)
    slot = {(int(r[0]), int(r[1])): q for q, r in reversed(list(enumerate(base.nz)))}
    prod = lambda q: gA[q // lb] * gB[q % lb] % P
    cl = _edged_layers(base.C)
    slot_of = {l: slot.get((int(base.C.layers[l]["nonce_lo"]), int(base.C.layers[l]["nonce_hi"]))) for l in cl}

    def out(name, t, want):
        t.name = base.name + ":" + name
        return name, t, want if base.plain else None

    for X in "ABC":
        live = _live_edges(getattr(base, X))
        if not live:
            continue
        for name, field, bit in (("w_lo bit 0", "w_lo", 0), ("w_hi bit 62", "w_hi", 62)):
            t = base.copy()
            getattr(getattr(t, X), field)[_pick(rng, live)] ^= np.uint64(1 << bit)
            yield out(f"{name} of {X}", t, 1)
    for X in "CA":
        live = _live_edges(getattr(base, X))
        if live:
            t = base.copy()
            c, e = getattr(t, X), _pick(rng, live)
            c.meta[e] = _meta_with(c.meta[e], ch=1 - int(c.ch()[e]))
            yield out(f"ch flip in {X}", t, 1)
    live = _live_edges(base.C)
    if live:
        t = base.copy()
        e = _pick(rng, live)
        t.C.meta[e] = _meta_with(t.C.meta[e], idx=(int(t.C.idx()[e]) + 1) % Bm)   # g != 1: another power
        yield out("idx moved in C", t, 1)
    for X in "ABC":
        for v in (Bm, 0xFFFF):
            if getattr(base, X).nE:
                t = base.copy()
                c = getattr(t, X)
                e = int(rng.integers(0, c.nE))
                c.meta[e] = _meta_with(c.meta[e], idx=v)
                yield out(f"idx {'B' if v == Bm else '0xFFFF'} in {X}", t, 2)
    if live and len(cl) >= 2:
        t = base.copy()
        e = _pick(rng, live)
        t.C.meta[e] = _meta_with(t.C.meta[e], layer=_pick(rng, [l for l in cl if l != int(t.C.layer_id()[e])]))
        yield out("C edge moved to another product layer", t, 1)
    if live:
        C = base.C
        e = _pick(rng, live)
        keep = np.arange(C.nE) != e
        t = base.copy()
        _set_edges(t.C, C.meta[keep], C.w_lo[keep], C.w_hi[keep])
        yield out("C edge deleted", t, 1)
        t = base.copy()
        _set_edges(t.C, np.append(C.meta, C.meta[e]), np.append(C.w_lo, C.w_lo[e]), np.append(C.w_hi, C.w_hi[e]))
        yield out("C edge duplicated", t, 1)
    nonzero = [l for l in cl if slot_of[l] is not None and prod(slot_of[l])]
    if nonzero:
        C = base.C
        keep = C.layer_id() != _pick(rng, nonzero)
        t = base.copy()
        _set_edges(t.C, C.meta[keep], C.w_lo[keep], C.w_hi[keep])
        yield out("product layer emptied", t, 1)
    if cl:
        t = base.copy()
        t.C.layers[_pick(rng, cl)]["nonce_lo"] ^= np.uint64(1 << int(rng.integers(0, 64)))
        yield out("nonce bit of a layer with edges", t, 1)
        t = base.copy()
        t.C.layers[_pick(rng, cl)]["rule"] = 0
        yield out("rule 0 on a layer with edges", t, 1)
    empty = sorted(set(range(base.C.nL)) - set(cl))
    if empty:
        t = base.copy()
        t.C.layers[_pick(rng, empty)]["nonce_lo"] ^= np.uint64(1 << int(rng.integers(0, 64)))
        yield out("nonce bit of a layer without edges", t, 0)
    differ = [(a, b) for a in nonzero for b in nonzero if a < b and prod(slot_of[a]) != prod(slot_of[b])]
    if differ:
        a, b = _pick(rng, differ)
        t = base.copy()
        for f in ("nonce_lo", "nonce_hi"):
            t.C.layers[a][f], t.C.layers[b][f] = base.C.layers[b][f], base.C.layers[a][f]
        yield out("nonces of two product layers swapped", t, 1)
    if live:
        C = base.C
        e = _pick(rng, live)
        w = _wint(C, e)
        w1 = int(rng.integers(1, 2**63)) << 63 | 1
        (lo1, lo2), (hi1, hi2) = _words([w1, (w - w1) % P])
        t = base.copy()
        t.C.w_lo[e], t.C.w_hi[e] = lo1, hi1
        _set_edges(t.C, np.append(t.C.meta, C.meta[e]), np.append(t.C.w_lo, lo2), np.append(t.C.w_hi, hi2))
        yield out("C weight split in two", t, 0)
        tw = int(rng.integers(1, 2**63)) << 62 | 7
        (lo,), (hi,) = _words([tw])
        m = [_meta_with(C.meta[e], ch=0), _meta_with(C.meta[e], ch=1)]
        t = base.copy()
        _set_edges(t.C, np.concatenate([C.meta, m]), np.concatenate([C.w_lo, [lo, lo]]),
                   np.concatenate([C.w_hi, [hi, hi]]))
        yield out("+t on P and on M in C", t, 0)
    live = _live_edges(base.A)
    for k, lid in enumerate((base.A.nL, base.A.nL + 1000, 0xFFFFFFFF)):
        if live:
            t = base.copy()
            e = _pick(rng, live)
            t.A.meta[e] = _meta_with(t.A.meta[e], layer=lid)
            yield out(f"A edge in layer |A.L|+ ({k})", t, None)


ROWS = ["w_lo bit 0 of A", "w_lo bit 0 of B", "w_lo bit 0 of C", "w_hi bit 62 of A", "w_hi bit 62 of B",
        "w_hi bit 62 of C", "ch flip in C", "ch flip in A", "idx moved in C", "idx B in A", "idx B in B", "idx B in C",
        "idx 0xFFFF in A", "idx 0xFFFF in B", "idx 0xFFFF in C", "C edge moved to another product layer",
        "C edge deleted", "C edge duplicated", "product layer emptied", "nonce bit of a layer with edges",
        "nonce bit of a layer without edges", "rule 0 on a layer with edges", "nonces of two product layers swapped",
        "C weight split in two", "+t on P and on M in C", "A edge in layer |A.L|+ (0)", "A edge in layer |A.L|+ (1)",
        "A edge in layer |A.L|+ (2)"]
