"""Python model of ct_recrypt (reference ops/recrypt.hpp:26-41) on top of the CPU oracle.

The loop's ct_add is the oracle's ct_add; the final compact_edges + compact_layers is the oracle's
ct_add with an empty cipher at edge_budget 0 (guard_budget then compacts every cipher);
gen_ubk_public (crypto/matrix.hpp:95-164) is restated with hashlib, the bit permutation
(apply_perm_sigma, :167-188) with numpy, and the density decision (ops/encrypt.hpp:29-37,
recrypt.hpp:21-24) in numpy's long double. guard_budget inside the loop changes nothing: ct_add has
applied it to the same edges."""
import hashlib
import struct

import numpy as np

from helpers import LAYER_DT, Cipher

M64 = (1 << 64) - 1


def gen_ubk(canon_tag, m_bits):
    """(perm, inv) of gen_ubk_public: Fisher-Yates from SHA-256("UBK" || le64 tag || le64 counter)
    words with rejection sampling; inv[perm[i]] = i."""
    state = {"c": 0, "buf": b"", "idx": 32}

    def r():
        if state["idx"] >= 32:
            state["buf"] = hashlib.sha256(b"UBK" + struct.pack("<Q", canon_tag & M64) +
                                          struct.pack("<Q", state["c"])).digest()
            state["c"] += 1
            state["idx"] = 0
        x = struct.unpack_from("<Q", state["buf"], state["idx"])[0]
        state["idx"] += 8
        return x

    def bounded(m):
        if m <= 1:
            return 0
        lim = M64 - (M64 % m)
        while True:
            x = r()
            if x <= lim:
                return x % m

    perm = list(range(m_bits))
    for i in range(m_bits - 1, 0, -1):
        j = bounded(i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    perm = np.array(perm, np.int32)
    inv = np.zeros(m_bits, np.int32)
    inv[perm] = np.arange(m_bits, dtype=np.int32)
    return perm, inv


def apply_perm(sigma, inv, m_bits):
    """apply_perm_sigma on every row of sigma (rows, words) u64: out[inv[src]] = in[src], src < m_bits."""
    sigma = np.ascontiguousarray(sigma, np.uint64)
    rows, words = sigma.shape
    if rows == 0:
        return sigma.copy()
    bits = np.unpackbits(sigma.view(np.uint8).reshape(rows, words * 8), axis=1, bitorder="little")
    out = np.zeros_like(bits)
    out[:, np.asarray(inv, np.int64)] = bits[:, :m_bits]
    return np.packbits(out, axis=1, bitorder="little").view(np.uint64).reshape(rows, words)


def popcount(sigma):
    return int(np.unpackbits(np.ascontiguousarray(sigma, np.uint64).view(np.uint8)).sum())


def needs_balance(ones, n_edges, m_bits):
    """sigma_needs_balance: strictly outside [0.495, 0.505]."""
    d = float(np.longdouble(ones) / np.longdouble(n_edges * m_bits))
    return d < 0.495 or d > 0.505


def empty_cipher(words=128):
    z = np.zeros(0, np.uint64)
    return Cipher(np.zeros(0, LAYER_DT), z, z, z, np.zeros((0, words), np.uint64))


def compact(orc, c):
    """compact_edges then compact_layers."""
    return orc.ct_add(c, empty_cipher(), edge_budget=0)


def recrypt(orc, x, pool, picks, inv, m_bits=8192):
    """ct_recrypt(x) with the draws picks[0..8) (consumed by the iterations that run, in order).
    Returns (cipher, iterations)."""
    if not pool or x.nE == 0:
        return x, 0
    res, it = x, 0
    while it < 8 and needs_balance(popcount(res.sigma), res.nE, m_bits):
        member = pool[int(picks[it]) % len(pool)]
        res = orc.ct_add(res, member)
        res = Cipher(res.layers, res.meta, res.w_lo, res.w_hi, apply_perm(res.sigma, inv, m_bits))
        it += 1
    return compact(orc, res), it
