"""pvac_hip_check_mul_gsum (k_check.hip) against its exact CPU model (gsum_model.py): per-pair statuses
of hand-built and ct_mul triples and of every mutation of gsum_cases.py, with the layer tables in LDS
and in global slabs, through the persistent loop in both orders, around the LDS / slab switch and at
the edge-count bound. test_gsum_model.py pins the model and the class of every mutation on the CPU."""
import time

import numpy as np
import pytest

import gsum_cases as gc
from gsum_model import EDGE_LIMIT, status
from helpers import LAYER_DT, P, Cipher, pack_meta

pytestmark = pytest.mark.gpu


def _engine(Bm=337, powg=True):
    from pvac_hfhe_cppbyv_amd import Engine
    eng = Engine(device=0, B=Bm)
    if powg:
        eng.set_powg(gc.key_powg(Bm))
    return eng


def _store(ciphers, caps):
    """Host ciphers back to back (cipher i in a layer region of caps[i] >= |L| slots): offsets, rows."""
    l_off = np.cumsum([0] + list(caps))
    e_off = np.cumsum([0] + [c.nE for c in ciphers])
    layers = np.zeros(max(int(l_off[-1]), 1), LAYER_DT)
    for c, o in zip(ciphers, l_off):
        layers[o:o + c.nL] = c.layers
    cat = lambda f: np.concatenate([getattr(c, f) for c in ciphers] + [np.zeros(1, np.uint64)])
    return l_off[:-1], e_off[:-1], layers, cat("meta"), cat("w_lo"), cat("w_hi")


def batch_of(eng, triples, order):
    """DeviceBatches A, B, C and the nonce array of the pairs triples[order[0]], triples[order[1]], ...
    with EXPLICIT offsets: every triple is stored once and any number of pairs alias it. A stored
    C owns |A.L| + |B.L| + |A.L||B.L| layer slots at least, so that its product slots' nonces (at
    C.l_off + |A.L| + |B.L| + q, as ct_mul_exec lays them out) are its own."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(eng.device)
    order = np.asarray(order, np.int64)
    out = []
    for X in "ABC":
        cs = [getattr(t, X) for t in triples]
        caps = [max(c.nL, t.A.nL + t.B.nL + t.A.nL * t.B.nL) if X == "C" else c.nL for c, t in zip(cs, triples)]
        l_off, e_off, layers, meta, lo, hi = _store(cs, caps)
        pick = lambda v: dev(np.asarray(v, np.uint64)[order] if len(order) else np.zeros(1, np.uint64))
        out.append(DeviceBatch(len(order), pick(l_off), pick([c.nL for c in cs]),
                               torch.from_numpy(layers.view(np.int64).reshape(-1, 5)).to(eng.device), pick(e_off),
                               pick([c.nE for c in cs]), dev(meta), dev(lo), dev(hi)))
        if X == "C":
            nonces = np.zeros(2 * (int(l_off[-1]) + caps[-1]) + 2, np.uint64)
            for t, o in zip(triples, l_off):
                s = 2 * (int(o) + t.A.nL + t.B.nL)
                nonces[s:s + 2 * len(t.nz)] = t.nz.reshape(-1)
            out.append(dev(nonces))
    return out


_MODEL = {}


def _expected(oracle, triples, order, Bm):
    powg = gc.key_powg(Bm)
    for t in triples:
        if id(t) not in _MODEL:
            _MODEL[id(t)] = (t, status(oracle, t.A, t.B, t.C, t.nz, powg, Bm))   # t kept: ids stay unique
    return [_MODEL[id(triples[i])][1] for i in order]


def _check(eng, oracle, triples, order, Bm, mode):
    """One call: statuses equal the model's element for element, n_bad the nonzero count, and the
    call ran in `mode`. Returns the expected list."""
    want = _expected(oracle, triples, order, Bm)
    before = eng.check_mul_gsum_path_counts()
    A, B, C_, nonces = batch_of(eng, triples, order)
    bad, st = eng.check_mul_gsum(A, B, C_, nonces, status=True)
    got = [int(v) for v in st]
    assert got == want, [(i, triples[order[i]].name, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert bad == sum(1 for v in want if v)
    assert eng.check_mul_gsum(A, B, C_, nonces) == bad     # without a status array
    after = eng.check_mul_gsum_path_counts()
    assert {k: after[k] - before[k] for k in after} == {"lds": 2 * (mode == "lds"), "slab": 2 * (mode == "slab")}
    return want


@pytest.mark.parametrize("mode", ["lds", "slab"])
@pytest.mark.parametrize("Bm", [337, 1022])
def test_mutation_table_matches_model(oracle, Bm, mode):
    """Every base triple and every mutation of the table, each followed by its unmutated base, in
    one batch per mode; B = 337 and 1022 = 2 * 7 * 73."""
    eng = _engine(Bm)
    rows = gc.cases(oracle, Bm, mode)
    triples = [t for _, t, _ in rows]
    base_at, order = None, []
    for i, (name, _, _) in enumerate(rows):
        if name == "base":
            base_at = i
        order += [i, base_at]
    want = _check(eng, oracle, triples, order, Bm, mode)
    assert {0, 1, 2} <= set(want) and want.count(1) > 40
    assert eng.check_mul_gsum_path_counts() == {"lds": 2 * (mode == "lds"), "slab": 2 * (mode == "slab")}


def test_switch_between_lds_and_slabs(oracle):
    """The layer count of a hand-built C stepped across the documented table budget (include/pvac_hip.h),
    one passing and one corrupted pair per call: LDS calls first, then slab calls, switching once
    and where the header says, with the model's statuses at every size. The (2 x 3)-layer shape has
    a size whose tables are 160 KiB exactly, the (1 x 2)-layer shape one that fills the budget."""
    Bm = 337
    eng = _engine(Bm)
    powg = gc.key_powg(Bm)
    rng = np.random.default_rng(0x5B)
    for la, lb in ((2, 3), (1, 2)):
        first = gc.first_slab_layers(Bm, la, lb)
        sizes = {lc: gc.table_bytes(Bm, la, lb, lc, la * lb) for lc in range(first - 3, first + 3)}
        assert (160 * 1024 if la == 2 else gc.LDS_BUDGET) in sizes.values()
        seen = []
        for lc in sizes:
            good = gc.hand_triple(oracle, rng, gc.rand_cipher(rng, la, Bm), gc.rand_cipher(rng, lb, Bm), powg, Bm,
                                  f"{la}x{lb} in {lc}", c_layers=lc)
            bad = good.copy(good.name + " corrupted")
            bad.C.w_hi[int(rng.integers(0, bad.C.nE))] ^= np.uint64(1 << 17)
            mode = "slab" if sizes[lc] > gc.LDS_BUDGET else "lds"
            assert _check(eng, oracle, [good, bad], [1, 0, 1], Bm, mode) == [1, 0, 1]
            seen.append(mode)
        assert seen == ["lds"] * 3 + ["slab"] * 3


def _by_name(rows, name):
    return next(t for _, t, _ in rows if t.name == name)


@pytest.mark.parametrize("mode", ["lds", "slab"])
def test_persistent_loop_carries_nothing_between_pairs(oracle, mode):
    """grid + 70 pairs aliasing a few stored triples (grid = 8 x CUs workgroups with LDS tables, 2 x CUs
    over slabs), so that 70 workgroups take a second pair: failing, status-2 and (LDS) status-3 pairs
    first and good pairs second in the same workgroups, then the reverse, then failing after
    failing. A status-1 pair of each call fails only through a dropped product layer, whose slot the
    pair before it in the same workgroup had found."""
    import torch
    Bm = 337
    eng = _engine(Bm)
    rows = gc.cases(oracle, Bm, mode)
    base = "mul2x3" if mode == "lds" else "slab2x2"
    G = _by_name(rows, base)
    S1a, S1b, S2 = (_by_name(rows, f"{base}:{m}") for m in ("w_lo bit 0 of C", "product layer emptied",
                                                             "idx B in B"))
    triples = [G, S1a, S1b, S2]
    if mode == "lds":
        z = np.zeros(EDGE_LIMIT, np.uint64)
        S3 = G.copy("2^21 edges")
        S3.A = Cipher(G.A.layers, np.concatenate([G.A.meta, z])[:EDGE_LIMIT], np.concatenate([G.A.w_lo, z])[:EDGE_LIMIT],
                      np.concatenate([G.A.w_hi, z])[:EDGE_LIMIT])
        triples.append(S3)
    grid = torch.cuda.get_device_properties(0).multi_processor_count * (8 if mode == "lds" else 2)
    n = grid + 70
    spots = {5: 1, 17: 3, 50: 2, 69: 1}
    if mode == "lds":
        spots[33] = 4
    first, second, mixed = [0] * n, [0] * n, [0] * n
    for p, k in spots.items():
        first[p] = k
        second[p + grid] = k
        mixed[p], mixed[p + grid] = k, 1 + k % (len(triples) - 1)
    mixed[6], mixed[6 + grid] = 1, 2       # a failing pair, then the dropped layer alone
    for order in (first, second, mixed):
        want = _check(eng, oracle, triples, order, Bm, mode)
        assert sum(1 for v in want if v) == sum(1 for k in order if k)
    assert _expected(oracle, triples, range(len(triples)), Bm) == [0, 1, 1, 2, 3][:len(triples)]


@pytest.mark.parametrize("weights", ["p-1", "random"])
def test_edge_count_bound(oracle, weights):
    """One layer of 2^21 - 1 edges, the most the check takes: all at idx 0 on P with weight p - 1 (limbs
    2^43 - 2, 2^42 - 1, 2^42 - 1: the largest limb sums the u64 accumulators meet), or random
    canonical weights on both channels. C's single edge is gsum(A) gsum(B) from Python integers:
    status 0; that weight changed by 1: status 1; A with one edge more: status 3 (not checked), and
    the pairs around it unaffected."""
    Bm = 337
    eng = _engine(Bm)
    powg = gc.key_powg(Bm)
    pg = gc.powg_int(powg)
    rng = np.random.default_rng(0xB0 + len(weights))
    n = EDGE_LIMIT - 1
    if weights == "p-1":
        idx, ch = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        lo, hi = np.full(n + 1, 2**64 - 2, np.uint64), np.full(n + 1, 2**63 - 1, np.uint64)
        gA = n * (P - 1) % P
    else:
        idx, ch = rng.integers(0, Bm, n + 1).astype(np.uint64), rng.integers(0, 2, n + 1).astype(np.uint64)
        lo, hi = rng.integers(0, 2**64, n + 1, dtype=np.uint64), rng.integers(0, 2**63 - 1, n + 1, dtype=np.uint64)
        gA = None
    meta = pack_meta(np.zeros(n + 1, np.uint64), idx, ch)
    lay = gc.rand_cipher(rng, 1, Bm).layers
    A = Cipher(lay, meta[:n], lo[:n], hi[:n])
    A_over = Cipher(lay, meta, lo, hi)
    from gsum_model import layer_gsums
    if gA is None:
        gA = layer_gsums(oracle, A, powg)[0]
    else:
        assert layer_gsums(oracle, A, powg)[0] == gA
    wb, ib = int(rng.integers(1, 2**63)) << 40 | 11, int(rng.integers(0, Bm))
    B = Cipher(gc.rand_cipher(rng, 1, Bm).layers, pack_meta([0], [ib], [1]), [wb & gc.M64], [wb >> 64])
    nz = rng.integers(0, 2**64, (1, 2), dtype=np.uint64)

    def product(w):
        L = np.zeros(3, LAYER_DT)
        L[0], L[1] = A.layers[0], B.layers[0]
        L[2]["rule"], L[2]["pb"], L[2]["nonce_lo"], L[2]["nonce_hi"] = 1, 1, nz[0, 0], nz[0, 1]
        return Cipher(L, pack_meta([2], [0], [0]), [w & gc.M64], [w >> 64])

    w = gA * (P - wb * pg[ib] % P) % P
    assert w not in (0, P - 1)
    small = gc.product_triple(oracle, rng, 1, 1, Bm, "1x1")
    triples = [gc.Triple(A, B, product(w), nz, "2^21-1 edges"), gc.Triple(A, B, product(w + 1), nz, "C off by 1"),
               gc.Triple(A_over, B, product(w), nz, "2^21 edges"), small]
    t0 = time.perf_counter()
    want = _check(eng, oracle, triples, [3, 0, 1, 2, 3, 0], Bm, "lds")
    print(f"edge-count bound ({weights}): model + two check calls {time.perf_counter() - t0:.2f} s")
    assert want == [0, 0, 1, 3, 0, 0]


def test_api_errors_leave_context_usable(oracle):
    """No powg: PvacError; batches of differing n: PvacError; n = 0: 0 failing pairs; and the same
    context still checks a batch afterwards."""
    from pvac_hfhe_cppbyv_amd import PvacError
    Bm = 337
    rows = gc.cases(oracle, Bm, "lds")
    triples = [rows[0][1], _by_name(rows, "mul2x3:C edge deleted")]
    eng = _engine(Bm, powg=False)
    A, B, C_, nonces = batch_of(eng, triples, [0, 1])
    with pytest.raises(PvacError):
        eng.check_mul_gsum(A, B, C_, nonces)
    eng.set_powg(gc.key_powg(Bm))
    A1 = batch_of(eng, triples, [0])[0]
    with pytest.raises(PvacError):
        eng.check_mul_gsum(A1, B, C_, nonces)
    with pytest.raises(PvacError):
        eng.check_mul_gsum(A, B, batch_of(eng, triples, [0, 1, 0])[2], nonces)
    A0, B0, C0, n0 = batch_of(eng, triples, [])
    assert eng.check_mul_gsum(A0, B0, C0, n0) == 0
    bad, st = eng.check_mul_gsum(A0, B0, C0, n0, status=True)
    assert bad == 0 and len(st) == 0
    assert eng.check_mul_gsum_path_counts() == {"lds": 0, "slab": 0}
    assert _check(eng, oracle, triples, [0, 1, 1, 0], Bm, "lds") == [0, 1, 1, 0]
