"""The wide encryption route on the GPU (k_enc_wide.hip behind pvac_hip_enc_items): noise plans above 256
pre-merge edges per half, which the narrow kernels refuse. The two routes are held to each other on every
plan both can run (PVAC_ENC_WIDE_ALL), the wide one to the CPU model (tests/text_model.py) above that, and
the plan limit, the draw segments, the sub-batches and the uniform entry points to their contracts."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import text_model as tm
import text_wide_cases as tw
from helpers import fixture_secret, read_u64

pytestmark = pytest.mark.gpu

LIMIT = 2048   # pre-merge edges per half: hint 1000 has 1,923


def _engine(limit=None):
    from pvac_hfhe_cppbyv_amd import Engine
    sk, man, em = fixture_secret()
    e = Engine(device=0, canon_tag=man["canon_tag"], enc_plan_limit=limit)
    assert e.gen_H().hex() == man["H_digest"]
    e.set_secret(read_u64("sk_prf_k.u64"), read_u64("sk_lpn_s.u64"), em["lpn_n"], em["lpn_t"], em["lpn_tau_num"],
                 em["lpn_tau_den"])
    e.set_powg(read_u64("powg_B.u64"))
    return e


@pytest.fixture(scope="module")
def eng():
    return _engine(LIMIT)


npre = tw.npre


def _seeded_items(eng, rng, kinds, hints):
    """Seeded plaintexts (FP items: two words as given) on consecutive draws_hint segments."""
    vals = [int(rng.integers(0, 2**64, dtype=np.uint64)) | (0 if k else int(rng.integers(0, 2**63, dtype=np.uint64)) << 64)
            for k in kinds]
    dh = eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in zip(kinds, vals, hints)])[2]
    offs = np.concatenate([[0], np.cumsum(dh)]).astype(np.int64)
    rnd = rng.integers(0, 2**64, int(offs[-1]), dtype=np.uint64)
    return [(k, v, h, int(offs[i]), int(dh[i])) for i, (k, v, h) in enumerate(zip(kinds, vals, hints))], rnd


def _same_batches(X, Y, sx, sy, sigma=True):
    """Every output array: CSR offsets, counts, layers, meta, weights, sigma rows, status."""
    assert list(sx) == list(sy)
    for f in ("l_off", "l_cnt", "e_off", "e_cnt"):
        assert bool((getattr(X, f) == getattr(Y, f)).all()), f
    for i, (a, b) in enumerate(zip(X.to_host(), Y.to_host())):
        assert a.nL == b.nL and a.nE == b.nE, i
        assert a.layers.tobytes() == b.layers.tobytes(), i
        assert np.array_equal(a.meta, b.meta), i
        assert np.array_equal(a.w_lo, b.w_lo) and np.array_equal(a.w_hi, b.w_hi), i
        if sigma:
            assert np.array_equal(a.sigma, b.sigma), i


_records_equal = tw.records_equal


def test_routes_agree_on_the_narrow_plans(eng):
    """The 67-item mixed batch of test_gpu_text (hints 0, 2, 15, 16, 17 and 124, kinds alternating) as today
    and with PVAC_ENC_WIDE_ALL, both with sigma: every output array is equal, and the counters say 67
    narrow items, then 67 wide ones."""
    rng = np.random.default_rng(0x7E87)
    hints = [(0, 2, 15, 16, 17)[i % 5] for i in range(67)]
    hints[6] = hints[41] = 124
    kinds = [i % 2 for i in range(67)]
    items, rnd = _seeded_items(eng, rng, kinds, hints)
    c0 = eng.enc_path_counts()
    X, sx = eng.enc_items(items, rnd, sigma=True)
    c1 = eng.enc_path_counts()
    Y, sy = eng.enc_items(items, rnd, sigma=True, wide_all=True)
    c2 = eng.enc_path_counts()
    assert [b - a for a, b in zip(c0, c1)] == [67, 0, 1, 1]
    assert [b - a for a, b in zip(c1, c2)] == [0, 67, 1, 1]
    assert not sx.any()
    _same_batches(X, Y, sx, sy)
    # weights only: the same records, no sigma array
    Z, sz = eng.enc_items(items, rnd, sigma=False, wide_all=True)
    assert Z.sigma is None
    _same_batches(X, Z, sx, sz, sigma=False)


def _run_case(eng, name):
    """A fixture case, each cipher from its own draw segment, with sigma: records, counts and commit_ct with
    sigma against the manifest. Returns the batch and the ciphers."""
    case = tw.CASES[name]
    refs = tw.case_ciphers(case)
    X, st = eng.enc_items(tm.case_items(case), tw.case_draws(case), sigma=True)
    assert not st.any(), name
    out = X.to_host()
    digests = eng.commit_ct(X, with_sigma=True)
    assert len(out) == len(refs) == len(case["ciphers"])
    for k, (c, ref, rec) in enumerate(zip(out, refs, case["ciphers"])):
        assert (c.nL, c.nE) == (rec["layers"], rec["edges"]), (name, k)
        tw.records_equal(c, ref, (name, k))
        assert digests[k].tobytes().hex() == rec["commit"], (name, k)
    return X, out


@pytest.mark.parametrize("name", ["fpwide", "valwide", "b1875", "steep", "t2one", "t2zero"])
def test_reference_fixtures(eng, name):
    """Every case of tests/golden/text_wide, minted by the unmodified reference: hints 125 .. 1000 as bare
    and as masked items, a 125-block message whose last two ciphers are wide among 124 narrow ones, a steep
    slope, and a Z2-only and a Z3-only plan. The messages come back through dec_text."""
    case = tw.CASES[name]
    eng.set_noise(*tm.case_noise(case))
    try:
        X, out = _run_case(eng, name)
        if case["kind"] == "text":
            msg = bytes.fromhex(case["msg_hex"])
            assert eng.dec_text(X, [0, len(out)]) == [msg]
            segs = [(c["off"], c["cnt"]) for c in case["ciphers"]]
            Y, moff, st = eng.enc_text([msg], tw.case_draws(case), rnd_off=segs, sigma=False)
            assert not st.any() and moff == [0, len(out)]
            for k, (c, ref) in enumerate(zip(Y.to_host(), out)):
                tw.records_equal(c, ref, (name, k))
    finally:
        eng.set_noise()


MIXED_HINTS = [0, 125, 124, 126, 0, 200, 125, 0, 400, 124, 126, 0, 125, 200, 0, 126, 124, 125]
MIXED_KINDS = [1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1]


def test_mixed_ragged_batch_against_model(eng, oracle, H_dense):
    """18 items in one call, narrow (hints 0, 124) and wide (125, 126, 200, 400) interleaved, both kinds: the
    host permutation and both routes share the launch sequence. Every item equals the CPU model; three wide
    ones with sigma. Hint 400 has 782 edges on 674 keys: merging is forced, and more than 256 distinct keys
    survive, which 8-bit group ids could not hold."""
    sk, man, _ = fixture_secret()
    rng = np.random.default_rng(0x71DE)
    items, rnd = _seeded_items(eng, rng, MIXED_KINDS, MIXED_HINTS)
    c0 = eng.enc_path_counts()
    X, st = eng.enc_items(items, rnd, sigma=True)
    c1 = eng.enc_path_counts()
    n_wide = sum(h > 124 for h in MIXED_HINTS)
    assert [b - a for a, b in zip(c0, c1)] == [len(items) - n_wide, n_wide, 1, 1]
    assert not st.any()
    out = X.to_host()
    with_sigma = {1, 3, 8}   # hint 125 FP, hint 126 VALUE, hint 400 FP
    model = tm.Model(oracle, sk, man["canon_tag"], read_u64("powg_B.u64"), H_dense)

    def one(i):
        k, v, h, o, c = items[i]
        return model.enc_item(k, v, h, rnd[o:o + c], sigma=i in with_sigma)

    order = sorted(range(len(items)), key=lambda i: -npre(MIXED_HINTS[i]) * (1 + MIXED_KINDS[i]))
    with ThreadPoolExecutor(16) as pool:   # the CPU PRF dominates; the oracle calls drop the GIL
        refs = dict(zip(order, pool.map(one, order)))
    for i in range(len(items)):
        ref, rst = refs[i]
        assert rst == 0
        _records_equal(out[i], ref, i)
        if i in with_sigma:
            assert np.array_equal(out[i].sigma, ref.sigma), i
    assert npre(400) == 782 and 256 < out[8].nE < 782 and out[8].nE <= 674
    # the documented layout: prefix sums of the halves and of the pre-merge counts
    halves = [1 + k for k in MIXED_KINDS]
    pre = [(1 + k) * npre(h) for k, h in zip(MIXED_KINDS, MIXED_HINTS)]
    assert list(X.l_off.cpu().numpy()) == list(np.concatenate([[0], np.cumsum(halves)[:-1]]))
    assert list(X.e_off.cpu().numpy()) == list(np.concatenate([[0], np.cumsum(pre)[:-1]]))
    assert list(X.e_cnt.cpu().numpy()) == [c.nE for c in out]


def draws_used(kind, hint, words, B=337):
    """The draws one item consumes (its rejections included), or None when the segment runs out: the walk
    of text_model.Model.enc_fp_depth without the field arithmetic. The merged-edge count decides the
    shuffle's draws."""
    rs = tm.Draws(words)
    p = (1 << 127) - 1

    def fp_nonzero():
        while True:
            lo, hi = rs.next(), rs.next() & tm.M63
            if (lo | hi << 64) % p or rs.over:
                return

    def half():
        rs.next(), rs.next()
        idx, keys = [], set()
        for _ in range(8):
            while True:
                x = rs.next() % B
                if x not in idx or rs.over:
                    break
            idx.append(x)
            keys.add((x, rs.next() & 1))
        for _ in range(7):
            fp_nonzero()
        for _ in range(8):
            rs.next()
        z2, z3 = tm.plan_noise(hint, B=B)
        for _ in range(z2):
            i = rs.next() % B
            while True:
                j = rs.next() % B
                if j != i or rs.over:
                    break
            s1 = rs.next() & 1
            fp_nonzero()
            rs.next(), rs.next()
            keys.update([(i, s1), (j, s1 ^ 1)])
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
            s = [rs.next() & 1 for _ in range(3)]
            fp_nonzero(), fp_nonzero()
            rs.next(), rs.next(), rs.next()
            keys.update(zip((i, j, k), s))
        for _ in range(len(keys) - 1):
            rs.next()

    if kind == tm.VALUE:
        fp_nonzero()
        half()
    half()
    return None if rs.over else rs.i


def test_draw_segments(eng):
    """A wide item whose segment is one word short of what it consumes gets status 1 and leaves its
    neighbours byte-equal to the full run. 64 seeded wide items at hints 125..400 on consecutive draws_hint
    segments all return 0: the seed was checked on the CPU (draws_used, asserted here too) to need no more
    than its segments, and a wide draws_hint carries more slack than a narrow one."""
    rng = np.random.default_rng(0x5E65)
    items, rnd = _seeded_items(eng, rng, [0, 1, 0], [126, 125, 200])
    X, sx = eng.enc_items(items, rnd, sigma=True)
    assert list(sx) == [0, 0, 0]
    k, v, h, o, c = items[1]
    used = draws_used(k, h, rnd[o:o + c])
    assert used is not None and used <= c
    short = list(items)
    short[1] = (k, v, h, o, used - 1)
    exact = list(items)
    exact[1] = (k, v, h, o, used)
    Y, sy = eng.enc_items(short, rnd, sigma=True)
    assert list(sy) == [0, 1, 0]
    Z, sz = eng.enc_items(exact, rnd, sigma=True)
    assert list(sz) == [0, 0, 0]
    xs, ys, zs = X.to_host(), Y.to_host(), Z.to_host()
    for i in (0, 2):
        _records_equal(ys[i], xs[i], i)
        assert np.array_equal(ys[i].sigma, xs[i].sigma)
    _records_equal(zs[1], xs[1], "exact segment")
    # the slack: 32 a half up to 256 edges, max(146, ceil(6 (28 + Z2 + 3 Z3) / B)) above
    dh = eng.enc_items_caps([(tm.FP, 1, 124, 0, 0), (tm.FP, 1, 125, 0, 0), (tm.VALUE, 1, 125, 0, 0)])[2]
    det = lambda hint: 32 + 2 * npre(hint) + 5 * tm.plan_noise(hint)[0] + 10 * tm.plan_noise(hint)[1]
    assert [int(x) for x in dh] == [det(124) + 32, det(125) + 146, 2 + 2 * det(125) + 2 * 146]
    # 64 wide items
    rng = np.random.default_rng(0x5E66)
    hints = [int(x) for x in rng.integers(125, 401, 64)]
    kinds = [i % 2 for i in range(64)]
    items, rnd = _seeded_items(eng, rng, kinds, hints)
    assert all(draws_used(k, h, rnd[o:o + c]) is not None for k, v, h, o, c in items)
    _, st = eng.enc_items(items, rnd, sigma=False)
    assert not st.any()


def test_sub_batches_do_not_change_the_result(eng):
    """Nine items, narrow and wide, once in one sub-batch and once with the budget lowered to 900 pre-merge
    edges: at least three sub-batches (the counter), one item (hint 400 as a VALUE: 1,564 edges) above the
    budget on its own, and equal outputs."""
    rng = np.random.default_rng(0x5B5B)
    hints = [0, 125, 16, 400, 124, 126, 2, 200, 125]
    kinds = [1, 0, 0, 1, 1, 0, 0, 0, 1]
    items, rnd = _seeded_items(eng, rng, kinds, hints)
    X, sx = eng.enc_items(items, rnd, sigma=True)
    assert not sx.any()
    assert eng.enc_budget == 1 << 22
    eng.set_enc_budget(900)
    try:
        c0 = eng.enc_path_counts()
        Y, sy = eng.enc_items(items, rnd, sigma=True)
        c1 = eng.enc_path_counts()
    finally:
        eng.set_enc_budget(1 << 22)
    d = [b - a for a, b in zip(c0, c1)]
    assert d[0] + d[1] == 9 and d[2] >= 3 and d[3] == 1
    assert 2 * npre(400) > 900
    _same_batches(X, Y, sx, sy)


def test_uniform_entry_above_256_edges(eng):
    """enc_value_depth at hints 125 and 300 gives what the same values give as VALUE items of enc_items from
    the same draws, in the layout enc_caps_depth reports (2 layers, 2 npre slots a value); at hint 124 it
    keeps its own kernels and the counter says narrow."""
    rng = np.random.default_rng(0x0E17)
    for hint, n in ((125, 5), (300, 3)):
        lp, ep, dh = eng.enc_caps(hint)
        assert (lp, ep) == (2, 2 * npre(hint))
        vals = rng.integers(0, 2**64, n, dtype=np.uint64)
        rnd = rng.integers(0, 2**64, (n, dh), dtype=np.uint64)
        c0 = eng.enc_path_counts()
        X, sx = eng.enc_value(vals, rnd, sigma=True, depth=hint)
        c1 = eng.enc_path_counts()
        assert [b - a for a, b in zip(c0, c1)] == [0, n, 1, 1]
        items = [(tm.VALUE, int(v), hint, i * dh, dh) for i, v in enumerate(vals)]
        Y, sy = eng.enc_items(items, rnd.reshape(-1), sigma=True)
        assert not sx.any()
        _same_batches(X, Y, sx, sy)
        assert list(X.l_off.cpu().numpy()) == [2 * i for i in range(n)]
        assert list(X.e_off.cpu().numpy()) == [ep * i for i in range(n)]
        dec, st = eng.dec_value(X, eng.base_R(X))
        assert not st.any() and [int(d) for d in dec] == [int(v) for v in vals]
    # the valwide fixtures (enc_value_depth at 125 and 300, enc_zero_depth at 125) through the uniform entry
    case = tw.CASES["valwide"]
    draws, refs = tw.case_draws(case), tw.case_ciphers(case)
    for rec, ref in zip(case["ciphers"], refs):
        assert rec["kind"] == tm.VALUE
        X, sx = eng.enc_value(np.array([rec["v_lo"]], np.uint64), draws[rec["off"]:rec["off"] + rec["cnt"]].reshape(1, -1),
                              sigma=True, depth=rec["hint"])
        assert not sx.any()
        tw.records_equal(X.to_host()[0], ref, rec["hint"])
        assert eng.commit_ct(X, with_sigma=True)[0].tobytes().hex() == rec["commit"]
    lp, ep, dh = eng.enc_caps(124)
    c0 = eng.enc_path_counts()
    X, sx = eng.enc_value(np.array([7, 0], np.uint64), rng.integers(0, 2**64, (2, dh), dtype=np.uint64), depth=124)
    c1 = eng.enc_path_counts()
    assert not sx.any() and [b - a for a, b in zip(c0, c1)][:2] == [2, 0]


def test_long_texts_round_trip(eng):
    """dec_text(enc_text(m)) = m for seeded messages of 1,846 and 2,000 bytes with sigma, and with a
    4,000-byte message (268 ciphers, hints up to 268) next to them weights-only, each set in one call on
    consecutive draws_hint segments; the same call twice gives the same bytes."""
    rng = np.random.default_rng(0x7E89)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1846, 2000, 4000)]
    for sel, sigma in ((msgs[:2], True), (msgs, False)):
        items, _ = eng.text_items(sel)
        total = int(eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in items])[2].sum())
        rnd = rng.integers(0, 2**64, total, dtype=np.uint64)
        X, moff, st = eng.enc_text(sel, rnd, sigma=sigma)
        assert not st.any() and moff[-1] == len(items)
        assert eng.dec_text(X, moff) == sel
        Y, _, st2 = eng.enc_text(sel, rnd, sigma=sigma)
        ne = int((X.e_off + X.e_cnt).max().item())
        for a, b in zip((X.l_off, X.l_cnt, X.e_off, X.e_cnt, X.layers, X.meta[:ne], X.w_lo[:ne], X.w_hi[:ne]),
                        (Y.l_off, Y.l_cnt, Y.e_off, Y.e_cnt, Y.layers, Y.meta[:ne], Y.w_lo[:ne], Y.w_hi[:ne])):
            assert bool((a == b).all())
        if sigma:
            ec, eo = X.e_cnt.cpu().numpy(), X.e_off.cpu().numpy()
            for i in (0, len(items) // 2, len(items) - 1):
                a, b = int(eo[i]), int(eo[i] + ec[i])
                assert bool((X.sigma[a:b] == Y.sigma[a:b]).all())


def test_defaults_and_refusals():
    """A fresh Engine reports limit 256 and refuses hint 125 with -38 as it always did; the limit's range is
    [256, 2^24]; above a raised limit the refusal returns, naming the limit."""
    from pvac_hfhe_cppbyv_amd import ENC_PLAN_LIMIT_DEFAULT, ENC_PLAN_LIMIT_MAX, Engine, PvacError
    e = Engine(device=0)
    assert e.enc_plan_limit == ENC_PLAN_LIMIT_DEFAULT == 256 and ENC_PLAN_LIMIT_MAX == 1 << 24
    for bad in (255, (1 << 24) + 1, 0):
        with pytest.raises(PvacError, match="-22"):
            e.set_enc_plan_limit(bad)
    assert e.enc_plan_limit == 256
    with pytest.raises(PvacError, match="-38.*256 pre-merge edges"):
        e.enc_items_caps([(tm.FP, 5, 125, 0, 0)])
    with pytest.raises(PvacError, match="-38"):
        e.enc_caps(125)
    assert e.enc_caps(124)[1] == 2 * 255
    e.set_enc_plan_limit(257)
    ls, es, dh = e.enc_items_caps([(tm.FP, 5, 125, 0, 0), (tm.VALUE, 5, 125, 0, 0)])
    assert (ls, es) == (3, 3 * 257)
    assert e.enc_caps(125)[:2] == (2, 514)
    with pytest.raises(PvacError, match="-38.*257 pre-merge edges"):
        e.enc_items_caps([(tm.FP, 5, 126, 0, 0)])
    e.set_enc_plan_limit(1 << 24)
    assert e.enc_plan_limit == 1 << 24
    with pytest.raises(PvacError, match="-22"):
        e.set_enc_budget(0)
