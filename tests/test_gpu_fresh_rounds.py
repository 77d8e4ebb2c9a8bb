"""Round classes of P1 / P5 and the writer's gated canonical finish in the fresh ct_mul kernel
(k_ct_mul_fresh3), on the GPU against the pinned CPU port: layer records, edge counts, edges in
emit order (metas and weights), and the per-pair status. Every batch asserts that the planner
classed its pairs as fresh-shaped (plan.n_small) and how many of them the general path redid.

Round classes. A wave's product round is full (64 products), empty or partial; a wave without a
partial round runs a path with no clamp and no mask, a wave with one runs the clamped loops. The
shapes put a partial round alone (1, 63 products), a full round alone (64), a full and a one-lane
partial round (65), exactly one full round on every wave (512), a one-lane partial round on the
rotated wave (513, 1,537), a partial round beside four full ones (1,640), the bench shape and the
largest square the planner still classes as fresh. They are mixed in one batch of more than one
grid stride, shifted by one shape per stride, so a workgroup that takes a second pair meets another
shape.

What the kernel itself decides for a shape: with 2 x 2 layers at B = 337 there are 1,348 key slots,
and every bucket count below 1,613 (fewer than about 1,540 products) puts more than 256 of them
into buckets of more than three, which overflows the kernel's big-bucket list: such a pair runs
through every phase of the fresh kernel, is flagged, and the general path redoes it. The mixed
batch of the listed shapes therefore expects exactly those pairs in the redo count (so it shows
that the phases run to their end for them, and the final outputs), and two further batches keep
the fresh kernel's own result with a redo count of 0: the four small shapes at B = 64 (no bucket
overflows there), and 1,537 / 1,600 / 1,640 / 1,849 products at B = 337. No B keeps 512 or 513
products out of the redo (541 buckets overflow the list for every admissible slot count).

Writer gate. 8 x 8-edge pairs at B = 64 (kept by the fresh kernel) whose weights make the gate
fire: a key whose two products sum to p, sums with the top word 0x7FFFFFFF that are not p, weights
below 2^32 (top word 0 in every lane of every round), a zero weight, and uniform weights."""
import collections

import numpy as np
import pytest

from helpers import M64, P
from test_gpu_fresh_roles import CANON, _check, _cipher, _expect_fresh, _member_list_overflows, _run

pytestmark = pytest.mark.gpu


def _engine(Bm):
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, canon_tag=CANON, B=Bm)


def _grid(eng):
    return 3 * eng.torch.cuda.get_device_properties(0).multi_processor_count


def _mixed(rng, shapes, n, G, Bm):
    """n pairs of 2 x 2 layers; pair p has shape (p + p // G) mod len(shapes): a workgroup of the
    persistent grid (stride G) meets the next shape at its next pair."""
    kind = [(p + p // G) % len(shapes) for p in range(n)]
    xs = [_cipher(rng, 2, shapes[k][0], Bm=Bm) for k in kind]
    ys = [_cipher(rng, 2, shapes[k][1], Bm=Bm) for k in kind]
    return kind, xs, ys


def _run_checked(oracle, eng, xs, ys, Bm, redo):
    r0 = eng.ct_mul_redo_count()
    out, plan, nz, loff, _ = _run(eng, oracle, xs, ys, Bm)
    assert (plan.n_small, plan.n_large) == (len(xs), 0)        # every pair classed PAIR_SMALL
    assert eng.ct_mul_redo_count() - r0 == redo
    assert not eng.ct_mul_status(len(xs)).any()
    host = out.to_host()
    _check(oracle, host, xs, ys, nz, loff, Bm)
    return host


def _largest_small_square(eng, oracle, rng, Bm):
    """The largest nA = nB the planner classes as fresh-shaped at 2 x 2 layers (asked pair by pair)."""
    from test_gpu_fresh_roles import _dev_batch
    best = 0
    for k in range(36, 65):
        x, y = _cipher(rng, 2, k, Bm=Bm), _cipher(rng, 2, k, Bm=Bm)
        _, plan = eng.ct_mul_plan(_dev_batch(eng, [x]), _dev_batch(eng, [y]))
        assert (plan.n_small == 1) == _expect_fresh(oracle, x, y, Bm)
        if plan.n_small == 1:
            best = k
    return best


def test_round_classes_listed_shapes(oracle):
    """The listed shapes at 2 x 2 layers and B = 337 in one batch; the pairs whose bucket count
    overflows the big-bucket list (all but 40 x 40 here) are redone, the others are not."""
    Bm = 337
    eng = _engine(Bm)
    rng = np.random.default_rng(0x90A1)
    k = _largest_small_square(eng, oracle, rng, Bm)
    assert k == 44
    shapes = [(1, 1), (7, 9), (8, 8), (5, 13), (16, 32), (19, 27), (40, 40), (k, k)]
    G = _grid(eng)
    n = G + 128
    kind, xs, ys = _mixed(rng, shapes, n, G, Bm)
    over = [_member_list_overflows(oracle, _cipher(rng, 2, a, Bm=Bm), _cipher(rng, 2, b, Bm=Bm), Bm) for a, b in shapes]
    assert over == [True, True, True, True, True, True, False, True]
    _run_checked(oracle, eng, xs, ys, Bm, redo=sum(over[s] for s in kind))


def test_round_classes_small_shapes_kept(oracle):
    """1, 63, 64 and 65 products at B = 64: no bucket overflows, the fresh kernel's result is kept."""
    Bm = 64
    eng = _engine(Bm)
    rng = np.random.default_rng(0x90A2)
    shapes = [(1, 1), (7, 9), (8, 8), (5, 13)]
    for a, b in shapes:
        x, y = _cipher(rng, 2, a, Bm=Bm), _cipher(rng, 2, b, Bm=Bm)
        assert _expect_fresh(oracle, x, y, Bm) and not _member_list_overflows(oracle, x, y, Bm)
    G = _grid(eng)
    _, xs, ys = _mixed(rng, shapes, G + 128, G, Bm)
    _run_checked(oracle, eng, xs, ys, Bm, redo=0)


def test_round_classes_large_shapes_kept(oracle):
    """1,537 (one-lane partial round on the rotated wave), 1,600 (the bench shape, and as 32 x 50),
    1,640 (a partial round beside four full ones) and 1,849 products at B = 337, all kept."""
    Bm = 337
    eng = _engine(Bm)
    rng = np.random.default_rng(0x90A3)
    shapes = [(29, 53), (40, 40), (32, 50), (40, 41), (43, 43)]
    for a, b in shapes:
        x, y = _cipher(rng, 2, a, Bm=Bm), _cipher(rng, 2, b, Bm=Bm)
        assert _expect_fresh(oracle, x, y, Bm) and not _member_list_overflows(oracle, x, y, Bm)
    G = _grid(eng)
    _, xs, ys = _mixed(rng, shapes, G + 128, G, Bm)
    _run_checked(oracle, eng, xs, ys, Bm, redo=0)


# ---------------------------------------------------------------- writer gate
GATE_B = 64


def _key_sums(x, y, Bm):
    """{(product layer, idx, channel): [sum of the products mod p, sum of the canonical products]}."""
    sums = collections.OrderedDict()
    for i in range(x.nE):
        wi = ((int(x.w_hi[i]) << 64) | int(x.w_lo[i])) % P
        la, ii, ci = int(x.meta[i]) & 0xFFFFFFFF, (int(x.meta[i]) >> 32) & 0xFFFF, (int(x.meta[i]) >> 48) & 1
        for j in range(y.nE):
            wj = ((int(y.w_hi[j]) << 64) | int(y.w_lo[j])) % P
            lb, ij, cj = int(y.meta[j]) & 0xFFFFFFFF, (int(y.meta[j]) >> 32) & 0xFFFF, (int(y.meta[j]) >> 48) & 1
            key = (la * y.nL + lb, (ii + ij) % Bm, ci ^ cj)
            s = sums.setdefault(key, [0, 0])
            s[0] = (s[0] + wi * wj) % P
            s[1] += (wi * wj) % P
    return sums


def _set_w(c, e, w):
    c.w_lo[e], c.w_hi[e] = np.uint64(w & M64), np.uint64(w >> 64)


def _gate_pair(rng, kind):
    x, y = _cipher(rng, 2, 8, Bm=GATE_B), _cipher(rng, 2, 8, Bm=GATE_B)
    if kind == "sum_is_p":      # edges 0 and 1 of A on one key, weights w and p - w: each of their keys sums to p
        x.meta[1] = x.meta[0]
        w = ((int(x.w_hi[0]) << 64) | int(x.w_lo[0])) % P
        _set_w(x, 0, w)
        _set_w(x, 1, P - w)
    elif kind == "top_word":    # A weights 1, B weights p - (small): every product has the top word 0x7FFFFFFF
        for e in range(8):
            _set_w(x, e, 1)
            _set_w(y, e, P - int(rng.integers(2, 2**40)))
    elif kind == "below_2_32":  # every product below 2^64, every sum below 2^70: top word 0 in every lane
        for e in range(8):
            _set_w(x, e, int(rng.integers(1, 2**32)))
            _set_w(y, e, int(rng.integers(1, 2**32)))
    elif kind == "zero_weight":
        _set_w(x, 3, 0)
    return x, y


_GATE_KINDS = ["sum_is_p", "top_word", "below_2_32", "zero_weight", "uniform"]


def test_writer_gate(oracle):
    """Eight pairs of each kind, mixed; the CPU sums of every pair are what its kind intends before
    anything runs: a key that sums to p (a multiple of p that is not 0 as an integer), a zero
    product, or neither. Pairs with a zero sum are flagged and redone, the others are kept."""
    eng = _engine(GATE_B)
    rng = np.random.default_rng(0x6A7E)
    kinds = [_GATE_KINDS[p % len(_GATE_KINDS)] for p in range(40)]
    pairs = [_gate_pair(rng, k) for k in kinds]
    xs, ys = [a for a, _ in pairs], [b for _, b in pairs]
    assert _expect_fresh(oracle, xs[0], ys[0], GATE_B) and not _member_list_overflows(oracle, xs[0], ys[0], GATE_B)
    redo = 0
    for k, x, y in zip(kinds, xs, ys):
        sums = _key_sums(x, y, GATE_B)
        zero = [s for s in sums.values() if s[0] == 0]
        if k == "sum_is_p":
            assert zero and all(s[1] > 0 and s[1] % P == 0 for s in zero)
        elif k == "zero_weight":
            assert zero and any(s[1] == 0 for s in zero)
        else:
            assert not zero
        if k == "top_word":     # kept sums with the top word 0x7FFFFFFF that are not p
            assert any(0 < s[0] < P and s[0] >> 96 == 0x7FFFFFFF for s in sums.values())
        if k == "below_2_32":
            assert all(0 < s[1] < 1 << 96 and s[1] == s[0] for s in sums.values())
        redo += bool(zero)
    assert redo == 16
    host = _run_checked(oracle, eng, xs, ys, GATE_B, redo=redo)
    for k, x, y, h in zip(kinds, xs, ys, host):   # no kept sum was zeroed, no zero sum was kept
        assert h.nE == sum(1 for s in _key_sums(x, y, GATE_B).values() if s[0] != 0), k
