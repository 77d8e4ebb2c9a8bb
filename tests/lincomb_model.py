"""Python model of ct_lincomb on top of the CPU oracle: the semantics, stated once.

fold():   the contract. Output = acc after acc = Cipher{}; for every term: t = X[term]; if flagged:
          t = ct_scale(pk, t, scale) (ops/arithmetic.hpp:33-37, Oracle.fp("mul")); acc = ct_add(pk, acc, t)
          (:12-31, Oracle.ct_add: guard_budget + compact_layers).
concat(): the independent form the one-pass kernels compute: compact_layers (ops/encrypt.hpp:73-104) of
          every term on its own, then concatenation with layer offsets. Equal to fold() for terms inside
          the Cipher contract and sums within edge_budget (tests/test_lincomb_model.py)."""
import json
import os

import numpy as np

from helpers import GOLD, LAYER_DT, Cipher, read_ct

M64 = (1 << 64) - 1
P = (1 << 127) - 1
TERM_SCALE = 1
NONE = 0xFFFFFFFF


def empty_cipher(sigma=False, words=128):
    z = np.zeros(0, np.uint64)
    return Cipher(np.zeros(0, LAYER_DT), z, z, z, np.zeros((0, words), np.uint64) if sigma else None)


def strip(c):
    return Cipher(c.layers, c.meta, c.w_lo, c.w_hi, None)


def scale_words(s):
    """A scale as (lo, hi) words: an int (any value below 2^128) or a pair of words."""
    if isinstance(s, (tuple, list, np.ndarray)):
        return int(s[0]), int(s[1])
    return int(s) & M64, (int(s) >> 64) & M64


def ct_scale(orc, c, s):
    lo, hi = scale_words(s)
    n = c.nE
    w_lo, w_hi = orc.fp("mul", c.w_lo, c.w_hi, np.full(n, lo, np.uint64), np.full(n, hi, np.uint64))
    return Cipher(c.layers, c.meta, w_lo, w_hi, c.sigma)


def is_scaled(k, scales, flags):
    return scales is not None and (flags is None or (int(flags[k]) & TERM_SCALE) != 0)


def fold(orc, X, terms, scales=None, flags=None, edge_budget=1200000, sigma=False):
    """One output: the reference's fold over `terms` (indices into the list of ciphers X)."""
    acc = empty_cipher(sigma)
    for k, t in enumerate(terms):
        c = X[int(t)] if sigma else strip(X[int(t)])
        if is_scaled(k, scales, flags):
            c = ct_scale(orc, c, scales[k])
        acc = orc.ct_add(acc, c, edge_budget=edge_budget)
    return acc


def fold_segments(orc, X, seg_off, term, scales=None, flags=None, edge_budget=1200000, sigma=False):
    out = []
    for i in range(len(seg_off) - 1):
        a, b = int(seg_off[i]), int(seg_off[i + 1])
        out.append(fold(orc, X, term[a:b], None if scales is None else scales[a:b],
                        None if flags is None else flags[a:b], edge_budget, sigma))
    return out


def compact_layers(c):
    """compact_layers of one cipher inside the contract (layer ids and PROD parents below |L|)."""
    L = c.nL
    if L == 0:
        return c
    used = np.zeros(L, bool)
    lid = c.layer_id()
    assert (lid < L).all()
    used[lid] = True
    changed = True
    while changed:
        changed = False
        for l in range(L):
            if used[l] and c.layers[l]["rule"] == 1:
                for p in (int(c.layers[l]["pa"]), int(c.layers[l]["pb"])):
                    assert p < L
                    if not used[p]:
                        used[p] = True
                        changed = True
    if used.all():
        return c
    remap = np.where(used, np.cumsum(used) - 1, NONE).astype(np.uint64)
    layers = c.layers[used].copy()
    prod = layers["rule"] == 1
    layers["pa"][prod] = remap[layers["pa"][prod]]
    layers["pb"][prod] = remap[layers["pb"][prod]]
    meta = (c.meta & np.uint64(~0xFFFFFFFF & M64)) | remap[lid]
    return Cipher(layers, meta, c.w_lo, c.w_hi, c.sigma)


def concat(orc, X, terms, scales=None, flags=None, sigma=False):
    """One output as the one-pass route builds it."""
    layers, meta, w_lo, w_hi, sg = [], [], [], [], []
    base = 0
    for k, t in enumerate(terms):
        c = X[int(t)] if sigma else strip(X[int(t)])
        if is_scaled(k, scales, flags):
            c = ct_scale(orc, c, scales[k])
        c = compact_layers(c)
        lay = c.layers.copy()
        prod = lay["rule"] == 1
        lay["pa"][prod] += base
        lay["pb"][prod] += base
        layers.append(lay)
        meta.append(c.meta + np.uint64(base))
        w_lo.append(c.w_lo)
        w_hi.append(c.w_hi)
        if sigma:
            sg.append(c.sigma)
        base += c.nL
    if not layers:
        return empty_cipher(sigma)
    return Cipher(np.concatenate(layers), np.concatenate(meta), np.concatenate(w_lo), np.concatenate(w_hi),
                  np.concatenate(sg) if sigma else None)


def same(a, b, sigma=False):
    """Byte-for-byte equality of two ciphers (layer records, edge headers, weight words, sigma rows)."""
    ok = (a.nL == b.nL and a.nE == b.nE and a.layers.tobytes() == b.layers.tobytes() and
          np.array_equal(a.meta, b.meta) and np.array_equal(a.w_lo, b.w_lo) and np.array_equal(a.w_hi, b.w_hi))
    if ok and sigma:
        ok = np.array_equal(np.asarray(a.sigma).reshape(a.nE, -1), np.asarray(b.sigma).reshape(b.nE, -1))
    return ok


# ---- the reference-minted fixtures (tools/mint_lincomb.cpp)
def manifest():
    with open(os.path.join(GOLD, "lincomb", "manifest.json")) as f:
        return json.load(f)


_FILES = {}


def golden_cipher(path):
    """The first cipher of tests/golden/<path>, read once."""
    if path not in _FILES:
        _FILES[path] = read_ct(os.path.join(GOLD, path))[0]
    return _FILES[path]


def case_inputs(case):
    """(pool of ciphers, term indices, scales or None, flags or None) of a manifest case."""
    names = sorted(set(case["terms"]))
    pool = [golden_cipher(p) for p in names]
    term = np.array([names.index(p) for p in case["terms"]], np.uint64)
    flags = np.array(case["flags"], np.uint32)
    if not flags.any():
        return pool, term, None, None
    return pool, term, [tuple(s) for s in case["scales"]], flags
