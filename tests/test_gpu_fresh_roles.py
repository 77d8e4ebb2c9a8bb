"""Role dealing of the fresh ct_mul kernel (k_ct_mul_fresh3): products and the staging of the next
pair are dealt by thread ids rotated by one wave, so these shapes put them on other waves than the
bins, scan segments and writer sweeps. Every output is bit-exact against the pinned CPU oracle
(layers, emit order, weights), and every batch asserts which path its pairs took.

Which shapes the planner admits to the fresh kernel (k_plan_mul): |A.L||B.L| B <= 1536 key slots,
|A.E||B.E| <= 4096 products and buckets + products + 3 <= 3 x key slots, where buckets is
libstdc++'s bucket count after reserve(products). At B = 337 that ends a little above 2,000
products: 48 x 48, 64 x 64 and 20 x 130 edges are general-path shapes (checked bit-exact there,
and asserted to be classed so). The loop of P5 that recomputes products past 4 x 512 needs more
than 1,366 key slots with B within the general path's 1,152, so two or more product layers of a
B near 768 (46 x 45 edges over 1 x 2 layers at B = 768 has its own case); every bucket count of
such a shape overflows the kernel's big-bucket list, so the pair is computed by the fresh kernel,
flagged, and redone on the general path: the case shows that the loop runs to its end under the
rotated ids, not its sums."""
import numpy as np
import pytest

from helpers import GOLDEN, LAYER_DT, M64, Cipher, P

pytestmark = pytest.mark.gpu

CANON = 0x7007


def _cipher(rng, nl, ne, Bm=337, layers=None):
    """A random cipher of nl BASE layers and ne edges; `layers` restricts the layers that get edges."""
    L = np.zeros(nl, LAYER_DT)
    L["ztag"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    L["nonce_lo"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    lay = rng.integers(0, nl if layers is None else layers, ne).astype(np.uint64)
    idx = rng.integers(0, Bm, ne).astype(np.uint64)
    ch = rng.integers(0, 2, ne).astype(np.uint64)
    meta = lay | (idx << np.uint64(32)) | (ch << np.uint64(48))
    return Cipher(L, meta, rng.integers(0, 2**64, ne, dtype=np.uint64), rng.integers(0, 2**64, ne, dtype=np.uint64))


def _dev_batch(eng, ciphers):
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    return DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, None) for c in ciphers], eng.device)


def _expect_fresh(oracle, x, y, Bm):
    """k_plan_mul's rule for one pair."""
    keys, prod = x.nL * y.nL * Bm, x.nE * y.nE
    return (keys <= 1536 and prod <= 4096 and x.nE <= 256 and y.nE <= 256 and x.nL + y.nL + x.nL * y.nL <= 64
            and oracle.bucket_count(prod) + prod + 3 <= 3 * keys)


def _member_list_overflows(oracle, x, y, Bm):
    """The fresh kernel keeps the slots of buckets with more than 3 key slots in a 256-entry list;
    a bucket count that needs more (few products, so few buckets for all |A.L||B.L| B slots) makes it
    flag every such pair, and the general path redoes them. Slot (lp, r) hashes to
    ((lp << 32 | r) * golden mod 2^64) mod buckets (ops/arithmetic.hpp:73)."""
    import collections
    nbk = oracle.bucket_count(x.nE * y.nE)
    sizes = collections.Counter((((lp << 32) | r) * GOLDEN & M64) % nbk for lp in range(x.nL * y.nL) for r in range(Bm))
    return sum(z for z in sizes.values() if z > 3) > 256


def _same(got, ref):
    for f in ("rule", "pa", "pb", "ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(got.layers[f], ref.layers[f]), f
    assert np.array_equal(got.meta, ref.meta)
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi)


def _run(eng, oracle, xs, ys, Bm=337, seed=5):
    """ct_mul of the batch; returns (device output, plan, nonce words, layer offsets)."""
    A, B = _dev_batch(eng, xs), _dev_batch(eng, ys)
    Cb, plan = eng.ct_mul_plan(A, B)
    nonces = eng.torch.empty(2 * max(plan.total_layer_slots, 1), dtype=eng.torch.int64, device=eng.device)
    eng.fill_random(nonces, seed)
    out = eng.ct_mul(A, B, nonces=nonces, C_=Cb, plan=plan)
    return out, plan, nonces.cpu().numpy().view(np.uint64), Cb.l_off.cpu().numpy().view(np.uint64), (A, B, Cb, nonces)


def _check(oracle, host, xs, ys, nz, loff, Bm=337, skip=()):
    for p, (x, y) in enumerate(zip(xs, ys)):
        if p in skip:
            continue
        base = int(loff[p]) + x.nL + y.nL
        ref = oracle.ct_mul(x, y, nz[2 * base:2 * base + 2 * x.nL * y.nL], canon_tag=CANON, Bm=Bm)
        _same(host[p], ref)


# (|A.L|, |A.E|), (|B.L|, |B.E|), B. The first eight are the shapes of the role re-deal: only the
# re-dealt wave holds products (1 x 1, 3 x 5), exactly three product rounds (32 x 48), the bench
# shape, two larger squares, and staging that spans more than one wave (100 x 20, 20 x 130). The
# 2,029 buckets of 100 x 20 overflow the big-bucket list (the pairs are flagged and redone), so
# 100 x 16 stages over two waves with its output kept; 130 x 12 and 12 x 130 stage over three waves
# (control, 0, 1) on either side; the last reaches P5's recompute loop (more than 2,048 products).
_SHAPES = [((2, 1), (2, 1), 337), ((2, 3), (2, 5), 337), ((2, 32), (2, 48), 337), ((2, 40), (2, 40), 337),
           ((2, 48), (2, 48), 337), ((2, 64), (2, 64), 337), ((2, 100), (2, 20), 337), ((2, 20), (2, 130), 337),
           ((2, 100), (2, 16), 337), ((2, 130), (2, 12), 337), ((2, 12), (2, 130), 337), ((1, 46), (2, 45), 768)]


@pytest.mark.parametrize("sa,sb,Bm", _SHAPES, ids=[f"{a[1]}x{b[1]}_B{m}" for a, b, m in _SHAPES])
def test_small_batch_shapes(oracle, sa, sb, Bm):
    from pvac_hfhe_cppbyv_amd import Engine
    n = 200
    rng = np.random.default_rng(sa[1] * 1000 + sb[1])
    eng = Engine(device=0, canon_tag=CANON, B=Bm)
    xs = [_cipher(rng, *sa, Bm=Bm) for _ in range(n)]
    ys = [_cipher(rng, *sb, Bm=Bm) for _ in range(n)]
    fresh = _expect_fresh(oracle, xs[0], ys[0], Bm)
    r0 = eng.ct_mul_redo_count()
    out, plan, nz, loff, _ = _run(eng, oracle, xs, ys, Bm)
    assert (plan.n_small, plan.n_large) == ((n, 0) if fresh else (0, n))
    if fresh:   # random full-range weights: no sum cancels, so only a member-list overflow is redone
        assert eng.ct_mul_redo_count() - r0 == (n if _member_list_overflows(oracle, xs[0], ys[0], Bm) else 0)
    assert not eng.ct_mul_status(n).any()
    _check(oracle, out.to_host(), xs, ys, nz, loff, Bm)


def test_fresh_shapes_are_fresh(oracle):
    """The planner's rule as restated above: which of the shapes run in the fresh kernel."""
    rng = np.random.default_rng(1)
    cs = [(_cipher(rng, *a, Bm=m), _cipher(rng, *b, Bm=m), m) for a, b, m in _SHAPES]
    fresh = [_expect_fresh(oracle, *c) for c in cs]
    assert fresh == [True, True, True, True, False, False, True, False, True, True, True, True]
    # of the fresh ones: the two tiny shapes, 100 x 20 and the last overflow the big-bucket list
    assert [_member_list_overflows(oracle, *c) for c, f in zip(cs, fresh) if f] == [True, True, False, False, True, False,
                                                                                  False, False, True]


def test_special_pairs_in_a_fresh_batch(oracle):
    """40 x 40-edge pairs with, among them: a pair with empty product layers (all of A's edges in
    layer 0: compact_layers removes layers), a cancelling key (flagged by the writer, redone on the
    general path), and a pair with an invalid layer reference (status 2, empty output) followed by
    valid pairs."""
    from pvac_hfhe_cppbyv_amd import Engine
    n = 96
    rng = np.random.default_rng(0x5EC1A1)
    eng = Engine(device=0, canon_tag=CANON)
    xs = [_cipher(rng, 2, 40) for _ in range(n)]
    ys = [_cipher(rng, 2, 40) for _ in range(n)]
    xs[5] = _cipher(rng, 2, 40, layers=1)
    c = xs[9]   # edge 1 repeats edge 0's key with the negated weight: every key of theirs sums to 0
    c.meta[1] = c.meta[0]
    w = ((int(c.w_hi[0]) << 64) | int(c.w_lo[0])) % P
    c.w_lo[1], c.w_hi[1] = (P - w) & (2**64 - 1), (P - w) >> 64
    xs[13].meta[0] = (xs[13].meta[0] & ~np.uint64(0xFFFFFFFF)) | np.uint64(2)   # layer_id == |A.L|
    r0 = eng.ct_mul_redo_count()
    out, plan, nz, loff, _ = _run(eng, oracle, xs, ys)
    assert (plan.n_small, plan.n_large) == (n, 0)
    assert eng.ct_mul_redo_count() - r0 == 1
    st = eng.ct_mul_status(n)
    assert [int(p) for p in np.flatnonzero(np.asarray(st) == 2)] == [13]
    host = out.to_host()
    assert host[13].nE == 0 and host[13].nL == 0
    assert host[5].nL < 2 + 2 + 4
    _check(oracle, host, xs, ys, nz, loff, skip=(13,))


def test_mixed_batch_general_pairs_a_grid_stride_after_fresh(oracle):
    """More than four times the persistent grid (3 workgroups per CU) of 40 x 40-edge pairs with
    general-path pairs placed a whole number of grid strides after fresh pairs, so the workgroup
    that meets one skips ahead while its other waves still hold the previous header words: one
    stride after a fresh pair with fresh pairs after it, two in a row, first in a workgroup's
    sequence, and last in it. Every output equals the oracle's and a rerun gives equal digests."""
    from pvac_hfhe_cppbyv_amd import Engine
    eng = Engine(device=0, canon_tag=CANON)
    G = 3 * eng.torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * G + 64
    general = sorted({3, G + 7, 2 * G + 9, 3 * G + 9, 4 * G + 11, G // 3 + 2 * G, G // 2 + G})
    rng = np.random.default_rng(0x313ED)
    xs = [_cipher(rng, 2, 40) for _ in range(n)]
    ys = [_cipher(rng, 2, 40) for _ in range(n)]
    for p in general:
        xs[p], ys[p] = _cipher(rng, 3, 60), _cipher(rng, 2, 70)
    r0 = eng.ct_mul_redo_count()
    out, plan, nz, loff, (A, B, Cb, nonces) = _run(eng, oracle, xs, ys)
    assert (plan.n_small, plan.n_large) == (n - len(general), len(general))
    assert eng.ct_mul_redo_count() == r0
    assert not eng.ct_mul_status(n).any()
    dig = eng.digest(out)[:n].cpu().numpy().copy()
    _check(oracle, out.to_host(), xs, ys, nz, loff)
    Cb2, plan2 = eng.ct_mul_plan(A, B)
    out2 = eng.ct_mul(A, B, nonces=nonces, C_=Cb2, plan=plan2)
    assert np.array_equal(eng.digest(out2)[:n].cpu().numpy(), dig)
