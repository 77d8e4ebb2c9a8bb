"""The fresh ct_mul kernel's 48/48/32-bit limb accumulators (fp_split3_48 / fp_fold3_48 in P5 and the
writer, fp_mul_fold1f) on the GPU: batches of at most 64 pairs, each compared with the pinned CPU
oracle (layer records, edge counts, edges in emit order), each with ct_mul_redo_count as expected, so
the pairs really ran on k_ct_mul_fresh3.

The shapes put the most addends the bench shape allows on one emit position: 40 x 40 edges over
2 x 2 layers with every A edge on (layer 0, idx a, ch 0) and every B edge on (layer 0, idx b, ch 0)
give one cell with all 1,600 products (and three empty product layers, so compact_layers' closure
runs). Weights p - 1 = 2^127 - 2 are the largest canonical operands; the raw words 2^128 - 1 and the
boundary values of the limb cuts (bits 47/48 and 95/96, single 16-bit words all ones) go through
stage_pair's canonicalisation first. No shape here needs more than 2,000 products: larger ones never
reach this kernel's result."""
import numpy as np
import pytest

from helpers import Cipher, P
from test_gpu_fresh_roles import CANON, _check, _cipher, _run

pytestmark = pytest.mark.gpu

BM = 337
M64 = (1 << 64) - 1
# raw 128-bit weight words on the limb cuts: the extremes, single 16-bit words all ones, runs of set
# bits across bits 47/48 and 95/96 (alone and on both cuts), whole limbs
BOUNDARY = ([1, P - 1, (1 << 127) - 2, P, (1 << 128) - 1, 1 << 127]
            + [0xFFFF << (16 * w) for w in range(8)]
            + [3 << 47, 7 << 46, 3 << 95, 7 << 94, (3 << 47) | (3 << 95), (15 << 46) | (15 << 94)]
            + [(1 << 48) - 1, (1 << 96) - 1, ((1 << 128) - 1) ^ ((1 << 96) - 1)])


def _placed(rng, idx, ch, weights):
    """A 2-layer cipher whose edges all sit in layer 0 at the given idx / ch / raw 128-bit weights."""
    c = _cipher(rng, 2, len(idx), Bm=BM)
    c.meta[:] = (np.asarray(idx, np.uint64) << np.uint64(32)) | (np.asarray(ch, np.uint64) << np.uint64(48))
    c.w_lo[:] = np.array([w & M64 for w in weights], np.uint64)
    c.w_hi[:] = np.array([w >> 64 for w in weights], np.uint64)
    return c


def _cell_sums(x, y):
    """{(idx sum mod B, channel): sum of products mod p} of one pair whose edges all sit in layer 0."""
    sums = {}
    for i in range(x.nE):
        wi = ((int(x.w_hi[i]) << 64) | int(x.w_lo[i])) % P
        ii, ci = (int(x.meta[i]) >> 32) & 0xFFFF, (int(x.meta[i]) >> 48) & 1
        for j in range(y.nE):
            wj = ((int(y.w_hi[j]) << 64) | int(y.w_lo[j])) % P
            ij, cj = (int(y.meta[j]) >> 32) & 0xFFFF, (int(y.meta[j]) >> 48) & 1
            k = ((ii + ij) % BM, ci ^ cj)
            sums[k] = (sums.get(k, 0) + wi * wj) % P
    return sums


def _run_fresh(oracle, xs, ys, redo):
    from pvac_hfhe_cppbyv_amd import Engine
    eng = Engine(device=0, canon_tag=CANON)
    r0 = eng.ct_mul_redo_count()
    out, plan, nz, loff, _ = _run(eng, oracle, xs, ys, BM)
    assert (plan.n_small, plan.n_large) == (len(xs), 0)
    assert eng.ct_mul_redo_count() - r0 == redo
    assert not eng.ct_mul_status(len(xs)).any()
    host = out.to_host()
    _check(oracle, host, xs, ys, nz, loff, BM)
    return host


# idx pairs (a, b): no wrap, a + b == B - 1, a + b == B (wraps to 0), both at the top
_IDX = [(0, 0), (5, 11), (100, 236), (200, 137), (336, 336), (336, 0), (1, 335), (170, 170)]


@pytest.mark.parametrize("w", [P - 1, (1 << 127) - 2, (1 << 128) - 1], ids=["p-1", "2^127-2", "2^128-1"])
def test_all_products_in_one_cell(oracle, w):
    """1,600 maximal products on one emit position; three product layers stay empty."""
    rng = np.random.default_rng(0x48)
    xs = [_placed(rng, [a] * 40, [0] * 40, [w] * 40) for a, _ in _IDX]
    ys = [_placed(rng, [b] * 40, [0] * 40, [w] * 40) for _, b in _IDX]
    for x, y in zip(xs, ys):   # one cell, and its sum is not 0 (the pair is not redone)
        s = _cell_sums(x, y)
        assert len(s) == 1 and all(s.values())
    host = _run_fresh(oracle, xs, ys, redo=0)
    assert all(h.nE == 1 for h in host)


def test_two_cells_per_channel_boundary_weights(oracle):
    """The same shape over two slots x two channels (400 products each), weights from the boundary set."""
    rng = np.random.default_rng(0x4848)
    xs, ys = [], []
    for p, (a, b) in enumerate(_IDX):
        wa = [BOUNDARY[(p + 3 * e) % len(BOUNDARY)] for e in range(40)]
        wb = [BOUNDARY[(5 * p + 7 * e + 1) % len(BOUNDARY)] for e in range(40)]
        xs.append(_placed(rng, [a] * 40, [e & 1 for e in range(40)], wa))
        ys.append(_placed(rng, [(b + ((e >> 1) & 1)) % BM for e in range(40)], [(e >> 2) & 1 for e in range(40)], wb))
    for x, y in zip(xs, ys):
        s = _cell_sums(x, y)
        assert len(s) == 4 and all(s.values())
    host = _run_fresh(oracle, xs, ys, redo=0)
    assert all(h.nE == 4 for h in host)


def test_gen_fresh_control(oracle):
    """An ordinary gen_fresh batch of 64 pairs at 20 edges per layer."""
    from pvac_hfhe_cppbyv_amd import Engine
    eng = Engine(device=0, canon_tag=CANON)
    torch = eng.torch
    A, B = eng.gen_fresh(64, 0x481, 20), eng.gen_fresh(64, 0x482, 20)
    r0 = eng.ct_mul_redo_count()
    Cb, plan = eng.ct_mul_plan(A, B)
    assert (plan.n_small, plan.n_large) == (64, 0)
    nonces = torch.empty(2 * plan.total_layer_slots, dtype=torch.int64, device=eng.device)
    eng.fill_random(nonces, 0x483)
    out = eng.ct_mul(A, B, nonces=nonces, C_=Cb, plan=plan).to_host()
    assert eng.ct_mul_redo_count() == r0
    assert not eng.ct_mul_status(64).any()
    xs = [Cipher(c.layers, c.meta, c.w_lo, c.w_hi) for c in A.to_host()]
    ys = [Cipher(c.layers, c.meta, c.w_lo, c.w_hi) for c in B.to_host()]
    _check(oracle, out, xs, ys, nonces.cpu().numpy().view(np.uint64), Cb.l_off.cpu().numpy().view(np.uint64), BM)


def test_cancelling_key_is_redone(oracle):
    """One pair of the one-cell shape whose 1,600 products sum to 0 mod p (half of A's weights negated):
    the writer folds a zero, the pair is flagged and redone on the general path, and still matches."""
    rng = np.random.default_rng(0x4849)
    w = 0x0123456789ABCDEF0123456789ABCDEF % P
    xs = [_placed(rng, [7] * 40, [0] * 40, [w if e < 20 else P - w for e in range(40)]), _cipher(rng, 2, 40, Bm=BM)]
    ys = [_placed(rng, [9] * 40, [0] * 40, [P - 1] * 40), _cipher(rng, 2, 40, Bm=BM)]
    assert list(_cell_sums(xs[0], ys[0]).values()) == [0]
    _run_fresh(oracle, xs, ys, redo=1)
