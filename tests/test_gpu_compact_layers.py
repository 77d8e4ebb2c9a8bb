"""GPU parity of the workgroup form of compact_layers (csrc/compact_layers.hpp) through every kernel
that runs it, against the CPU oracle: k_ct_add, k_ct_add_deep, k_merge_layers, k_lincomb_plan_wg,
k_compact_small and k_large_layers. (The deep ct_mul closure: test_gpu_deep.py.)

One cipher family, scaled to a layer count L: BASE layers below L / 2, PROD layers above with parents
anywhere below them and a chain several levels deep at the top, two PROD layers among the BASE ones whose
parents have LARGER indices (one ascending sweep cannot close the set), edges on a few layers only, so
most BASE layers are dropped and the remap is not the identity. Its twin has the same layers with an
edge on every one: the identity remap, parents untouched.

The sizes straddle what the shared code does per workgroup of BS threads: one sweep round (BS - 1, BS,
BS + 1) and one scan tile of T = 4 BS layers (T - 1, T, T + 1, 2 T + 1), besides 1 and 65."""
import ctypes as C

import numpy as np
import pytest

import lincomb_model as lm
from helpers import LAYER_DT, Cipher, default_params, pack_meta
from test_gpu_deep import _check_pairs, _run_mul

pytestmark = pytest.mark.gpu

B7 = 7
PER = 4   # layers one thread scans per tile (compact_layers.hpp: kRemapPer)


def sizes(bs, lo=1, hi=1 << 30):
    t = PER * bs
    return [L for L in (1, 65, bs - 1, bs, bs + 1, t - 1, t, t + 1, 2 * t + 1) if lo <= L <= hi]


# ------------------------------------------------------------------ the family
def family(rng, L, B=337, every=False, sigma=False, min_edges=0):
    """A cipher of L layers of the family above (every: its twin); at least min_edges edges."""
    lay = np.zeros(L, LAYER_DT)
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        lay[f] = rng.integers(0, 2**63, L, dtype=np.uint64)
    nb = max(1, L // 2)
    for l in range(nb, L):
        lay[l] = (1, int(rng.integers(0, l)), int(rng.integers(0, l)), 0, 0, 0, 0)
    at = [L - 1] if L else []
    if L >= 32:
        for l in (L - 1, L - 2, L - 3):   # L-1 -> L-2 -> L-3 -> L-4, a BASE parent beside each
            lay[l]["pa"], lay[l]["pb"] = l - 1, int(rng.integers(0, nb))
        h1, h2 = nb + (L - nb) // 2, nb + (L - nb) // 4
        # parents above their child: 2 -> h1 -> 3 -> h2
        lay[2] = (1, h1, 0, 0, 0, 0, 0)
        lay[h1]["pa"], lay[h1]["pb"] = 3, 1
        lay[3] = (1, h2, 1, 0, 0, 0, 0)
        at += [2] + rng.integers(3 * L // 4, L, 6).tolist() + rng.integers(4, nb, 6).tolist()
    if every:
        at = list(range(L))
    at = np.asarray(at, np.uint64)
    if L and len(at) < min_edges:
        at = np.concatenate([at, at[rng.integers(0, len(at), min_edges - len(at))]])
    n = len(at)
    rng.shuffle(at)
    meta = pack_meta(at, rng.integers(0, B, n), rng.integers(0, 2, n))
    sg = rng.integers(0, 2**64, (n, 128), dtype=np.uint64) if sigma else None
    return Cipher(lay, meta, rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**62, n, dtype=np.uint64), sg)


def pair(rng, L, **kw):
    """Two ciphers of the family with L layers between them."""
    return family(rng, L - L // 2, **kw), family(rng, L // 2, **kw)


def dev(eng, ciphers, sigma=False):
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    return DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in ciphers], eng.device,
                                 sigma=sigma)


def host(batch):
    return [Cipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in batch.to_host()]


def oracle_add(oracle, x, y, negate=False, edge_budget=1200000, B=337):
    prm = default_params(0, edge_budget, B=B)
    oc, ov = oracle._out(x.nL + y.nL, x.nE + y.nE, x.sigma is not None and y.sigma is not None)
    assert oracle.lib.orc_ct_add(C.byref(prm), C.byref(oracle._view(x)), C.byref(oracle._view(y)), int(negate), C.byref(ov)) == 0
    return oracle._trim(oc, ov)


def check_remaps(cases, outs):
    """cases: (inputs' layer count, twin?) per output. A twin keeps every layer; the others lose some
    (from 64 layers on: each cipher of a pair then has the family's unused BASE layers)."""
    for (L, every), o in zip(cases, outs):
        if every:
            assert o.nL == L, L
        elif L >= 64:
            assert 0 < o.nL < L, L


def make_engine(**kw):
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, **kw)


# ------------------------------------------------------------------ ct_add / ct_sub: k_ct_add, k_ct_add_deep
def add_case(rng, Ls):
    xs, ys, cases = [], [], []
    for L in Ls:
        for every in (False, True):
            x, y = pair(rng, L, every=every, sigma=True)
            xs.append(x); ys.append(y); cases.append((L, every))
    return xs, ys, cases


def run_add(oracle, eng, xs, ys, cases, negate):
    out = host(eng.ct_add(dev(eng, xs, True), dev(eng, ys, True), negate=negate, sigma=True))
    for x, y, o in zip(xs, ys, out):
        assert lm.same(o, oracle_add(oracle, x, y, negate), sigma=True), (x.nL, y.nL)
    check_remaps(cases, out)


@pytest.mark.parametrize("negate", [False, True])
def test_add_lds_table(oracle, negate):
    """k_ct_add (256 threads, the table in LDS): every pair of the call runs on it once the largest has
    more than 64 layers; 30,000, the last size of its table, once."""
    rng = np.random.default_rng(0xC1A0 + negate)
    xs, ys, cases = add_case(rng, sizes(256) + ([] if negate else [30000]))
    eng = make_engine()
    run_add(oracle, eng, xs, ys, cases, negate)
    assert eng.deep_path_counts() == (0, 0)


@pytest.mark.parametrize("negate", [False, True])
def test_add_slab_table(oracle, negate):
    """k_ct_add_deep (1,024 threads, the table in the global slab): a pair of 30,001 layers takes the
    whole call there."""
    rng = np.random.default_rng(0xC1A2 + negate)
    xs, ys, cases = add_case(rng, sizes(1024) + [30001])
    eng = make_engine(layer_limit=1 << 20)
    run_add(oracle, eng, xs, ys, cases, negate)
    assert eng.deep_path_counts() == (0, 1)


# ------------------------------------------------------------------ the merge route: k_merge_layers
def test_merge_route(oracle):
    """Every pair above edge_budget = 16: compact_edges, then k_merge_layers (1,024 threads, the table in
    global scratch) over the merged edges."""
    rng = np.random.default_rng(0xC1A4)
    xs, ys, cases = [], [], []
    for L in sizes(1024):
        for every in (False, True):
            x, y = pair(rng, L, every=every, sigma=True, min_edges=20)
            xs.append(x); ys.append(y); cases.append((L, every))
    assert all(x.nE + y.nE > 16 for x, y in zip(xs, ys))
    eng = make_engine(edge_budget=16)
    out = host(eng.ct_add(dev(eng, xs, True), dev(eng, ys, True), sigma=True))
    for x, y, o in zip(xs, ys, out):
        assert lm.same(o, oracle_add(oracle, x, y, edge_budget=16), sigma=True), (x.nL, y.nL)
    check_remaps(cases, out)


# ------------------------------------------------------------------ ct_sum: k_lincomb_plan_wg
def test_sum_workgroup_terms(oracle):
    """Terms of more than 64 layers (and one of 1 layer with more than 8,192 edges) take the workgroup
    route, each alone in a segment and all in one; a term with a kept PROD layer whose parent lies beyond
    it is out of contract and sends its segment to the fold."""
    rng = np.random.default_rng(0xC1A5)
    Ls = sizes(256, lo=65)
    pool = [family(rng, L, every=every) for L in Ls for every in (False, True)]
    cases = [(L, every) for L in Ls for every in (False, True)]
    pool.append(family(rng, 1, min_edges=8193))
    cases.append((1, True))
    n_in = len(pool)
    stray = family(rng, 300)
    stray.layers[299]["pb"] = 303   # layer 299 carries an edge
    pool.append(stray)
    segs = [[k] for k in range(n_in)] + [list(range(n_in)), [n_in, 0]]
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    term = np.array([t for s in segs for t in s], np.uint64)
    eng = make_engine()
    before = eng.ct_lincomb_path_counts()
    out = host(eng.ct_sum(dev(eng, pool), seg_off, term))
    want = lm.fold_segments(oracle, pool, seg_off, term)
    for i, (g, w) in enumerate(zip(out, want)):
        assert lm.same(g, w), i
    check_remaps(cases, out[:n_in])
    after = eng.ct_lincomb_path_counts()
    assert after["wg_terms"] - before["wg_terms"] == len(term)
    assert after["wave_terms"] == before["wave_terms"]
    assert after["fold"] - before["fold"] == 1 and after["one_pass"] - before["one_pass"] == len(segs) - 1
    assert list(eng.ct_lincomb_status(len(segs))) == [0] * (len(segs) - 1) + [2]


# ------------------------------------------------------------------ Engine.compact: k_compact_small
def test_compact_small_route(oracle):
    """B = 7: the batched kernel's key space admits up to 1,024 layers (512 threads: 1,024 is half a scan
    tile, the last size of the route)."""
    rng = np.random.default_rng(0xC1A6)
    Ls = sizes(512, hi=1024) + [1024]
    assert Ls == [1, 65, 511, 512, 513, 1024]
    cs = [family(rng, L, B=B7, every=every, sigma=True) for L in Ls for every in (False, True)]
    cases = [(L, every) for L in Ls for every in (False, True)]
    eng = make_engine(B=B7, m_bits=8192)
    out = host(eng.compact(dev(eng, cs, True)))
    empty = Cipher(np.zeros(0, LAYER_DT), [], [], [], np.zeros((0, 128), np.uint64))
    for c, o in zip(cs, out):
        assert lm.same(o, oracle_add(oracle, c, empty, edge_budget=0, B=B7), sigma=True), c.nL
    check_remaps(cases, out)
    assert eng.compact_path_counts() == {"small": len(cs), "merge": 0}


# ------------------------------------------------------------------ general-path ct_mul: k_large_layers
def test_mul_general_path(oracle):
    """k_large_layers (1,024 threads, T = 4,096) over A || B || products: (|A.L| + 1)(|B.L| + 1) - 1 layers
    = T - 1 = 16 * 256 - 1, T = 17 * 241 - 1 and T + 1 = 2 * 2049 - 1; the products of the twins all carry
    edges, so every layer stays."""
    rng = np.random.default_rng(0xC1A7)
    shapes = [(15, 255), (16, 240), (1, 2048)]
    assert [(a + 1) * (b + 1) - 1 for a, b in shapes] == [4095, 4096, 4097]
    xs, ys = [], []
    for la, lb in shapes:
        for every in (False, True):
            xs.append(family(rng, la, B=B7, every=every))
            ys.append(family(rng, lb, B=B7, every=every))
    eng = make_engine(B=B7, canon_tag=0xC1)
    out, plan, per, _, _ = _run_mul(eng, xs, ys, 11)
    assert plan.n_large == len(xs) and eng.deep_path_counts() == (0, 0)
    assert not eng.ct_mul_status(len(xs)).any()
    _check_pairs(oracle, out, xs, ys, per, canon_tag=0xC1)
    for p, (la, lb) in enumerate(shapes):
        assert 0 < out[2 * p].nL < la + lb + la * lb or la == 1
        assert out[2 * p + 1].nL == la + lb + la * lb
