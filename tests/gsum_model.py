"""Exact CPU model of pvac_hip_check_mul_gsum (include/pvac_hip.h): the reference's ct_mul invariant
check_mul_gsum_all (utils/metrics.hpp:88-113) restated over helpers.Cipher for a COMPACTED product C,
whose product layers are found by the nonce they carry. TEST INFRASTRUCTURE ONLY.

    gsum(X, l) = sum over X's edges of layer l of +/- fp_mul(w, powg_B[idx])   (metrics.hpp:70-86)

status() takes every term from the pinned port of the reference's fp_mul (oracle.fp) and sums the
terms as Python integers mod p; status_chain() evaluates agg_layer_gsum literally, the sequential
fp_add / fp_sub chain from 0 in edge order, and compares words as ct::fp_eq does. The two agree
unless a chain leaves the canonical range, which is what test_gsum_model.py pins.

nonce_pairs holds the (lo, hi) nonce words of the |A.L||B.L| product slots of the pair, slot
q = la |B.L| + lb: the words at C.l_off + |A.L| + |B.L| + q of the ct_mul ABI's nonce array."""
import numpy as np

from helpers import P

EDGE_LIMIT = 1 << 21   # status 3 from here on (the header's bound: limb sums of fewer terms stay below 2^64)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _terms(oracle, X, powg, keep):
    pg = np.asarray(powg, np.uint64).reshape(-1, 2)
    idx = X.idx()[keep].astype(np.int64)
    return oracle.fp("mul", X.w_lo[keep], X.w_hi[keep], pg[idx, 0], pg[idx, 1])


def layer_gsums(oracle, X, powg):
    """gsum(X, l) for every layer l of X as integers in [0, p): exact sums of the fp_mul terms.
    Edges whose layer_id names no layer of X are skipped (the reference's loops never ask for them)."""
    nL = X.nL
    keep = X.layer_id().astype(np.int64) < nL
    t_lo, t_hi = _terms(oracle, X, powg, keep)
    key = X.layer_id()[keep].astype(np.int64) * 2 + (X.ch()[keep] != 0)
    sums = [0] * (2 * nL)
    for half, shift in ((t_lo & _M32, 0), (t_lo >> _S32, 32), (t_hi & _M32, 64), (t_hi >> _S32, 96)):
        acc = np.zeros(2 * nL, np.uint64)   # < 2^21 addends below 2^32 each
        np.add.at(acc, key, half)
        for k in np.flatnonzero(acc):
            sums[k] += int(acc[k]) << shift
    return [(sums[2 * l] - sums[2 * l + 1]) % P for l in range(nL)]


def layer_gsums_chain(oracle, X, powg):
    """agg_layer_gsum literally: per layer the fp_add (P) / fp_sub (M) chain from 0 in edge order, as
    (lo, hi) words. One oracle call per edge: small ciphers only."""
    nL = X.nL
    keep = np.ones(X.nE, bool)
    t_lo, t_hi = _terms(oracle, X, powg, keep) if X.nE else (np.zeros(0, np.uint64),) * 2
    s = [(0, 0)] * nL
    lay, ch = X.layer_id(), X.ch()
    for e in range(X.nE):
        l = int(lay[e])
        if l >= nL:
            continue
        lo, hi = oracle.fp("add" if ch[e] == 0 else "sub", [s[l][0]], [s[l][1]], [t_lo[e]], [t_hi[e]])
        s[l] = (int(lo[0]), int(hi[0]))
    return s


class _Exact:
    def __init__(self, oracle):
        self.gsums = lambda X, powg: layer_gsums(oracle, X, powg)

    @staticmethod
    def product(a, b):
        return a * b % P

    @staticmethod
    def equal(a, b):
        return a == b

    @staticmethod
    def is_zero(a):
        return a == 0


class _Chain:
    def __init__(self, oracle):
        self.oracle = oracle
        self.gsums = lambda X, powg: layer_gsums_chain(oracle, X, powg)

    def product(self, a, b):
        lo, hi = self.oracle.fp("mul", [a[0]], [a[1]], [b[0]], [b[1]])
        return int(lo[0]), int(hi[0])

    @staticmethod
    def equal(a, b):
        return a == b            # ct::fp_eq: both words

    @staticmethod
    def is_zero(a):
        return a == (0, 0)       # against the gsum of a layer without edges, fp_from_u64(0)


def _invariant(ar, A, B, C, nonce_pairs, powg):
    LA, LB = A.nL, B.nL
    nz = np.asarray(nonce_pairs, np.uint64).reshape(-1, 2)
    assert len(nz) == LA * LB, "one (lo, hi) nonce per product slot"
    cand = {}
    for q in range(LA * LB):   # a nonce carried by two slots names the first
        cand.setdefault((int(nz[q, 0]), int(nz[q, 1])), q)
    gA, gB, gC = ar.gsums(A, powg), ar.gsums(B, powg), ar.gsums(C, powg)
    lay = C.layer_id().astype(np.int64)
    found = set()
    for l in np.unique(lay[lay < C.nL]):
        y = C.layers[l]
        q = cand.get((int(y["nonce_lo"]), int(y["nonce_hi"])))
        if q is None or int(y["rule"]) != 1:
            return 1
        found.add(q)
        if not ar.equal(gC[l], ar.product(gA[q // LB], gB[q % LB])):
            return 1
    for q in range(LA * LB):
        if q not in found and not ar.is_zero(ar.product(gA[q // LB], gB[q % LB])):
            return 1
    return 0


def _precheck(A, B, C, Bm):
    if max(A.nE, B.nE, C.nE) >= EDGE_LIMIT:
        return 3
    if any(X.nE and int(X.idx().max()) >= Bm for X in (A, B, C)):
        return 2
    return 0


def status(oracle, A, B, C, nonce_pairs, powg, Bm):
    """0 holds, 1 violated, 2 an edge idx >= Bm, 3 a cipher of 2^21 edges or more."""
    return _precheck(A, B, C, Bm) or _invariant(_Exact(oracle), A, B, C, nonce_pairs, powg)


def status_chain(oracle, A, B, C, nonce_pairs, powg, Bm):
    """status() with every gsum and product taken as the reference takes them (small ciphers)."""
    return _precheck(A, B, C, Bm) or _invariant(_Chain(oracle), A, B, C, nonce_pairs, powg)
