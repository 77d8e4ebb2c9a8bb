"""pvac_hip_batch_gather (Engine.gather / cat / select / split) on the GPU against tests/gather_model.py:
every field of every output cipher through to_host(), the full 40-byte layer records included, dense
offsets, arrays of exactly the planned size, and sentinels around everything the call must not touch."""
import ctypes as C
import os

import numpy as np
import pytest

import gather_model as gm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EINVAL, ENOMEM = -22, -12
CANARY = 0x25A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pvac_hfhe_cppbyv_amd import Engine
    e = Engine(device=0, canon_tag=0x5EED)
    e.set_H_digest(bytes(range(32)))
    return e


@pytest.fixture(scope="module")
def codec():
    from pvac_hfhe_cppbyv_amd import codec
    return codec


# ---------------------------------------------------------------------------------------- helpers
def u64(t):
    return t.cpu().numpy().view(np.uint64)


def make(rng, l_cnt, e_cnt, sw=0):
    """Random host ciphers: every byte of the layer records random (pad included), sigma rows of sw words."""
    from pvac_hfhe_cppbyv_amd import LAYER_DT, HostCipher
    out = []
    for nl, ne in zip(l_cnt, e_cnt):
        layers = np.frombuffer(rng.bytes(40 * nl), LAYER_DT).copy()
        r = lambda *s: rng.integers(0, 2**64, s, dtype=np.uint64)
        out.append(HostCipher(layers, r(ne), r(ne), r(ne), r(ne, sw) if sw else None))
    return out


def upload(eng, ciphers, gaps=None, sw=0, shift=0):
    """Host ciphers as a DeviceBatch whose cipher i starts gaps[i] slots after the end of cipher i - 1
    (capacity-padded CSR; the gaps hold canaries); shift: words by which the sigma base is moved."""
    import torch
    from pvac_hfhe_cppbyv_amd import LAYER_DT, DeviceBatch
    n = len(ciphers)
    gaps = gaps or [0] * n
    lo, eo, la, ea = [], [], 0, 0
    for c, g in zip(ciphers, gaps):
        la, ea = la + g, ea + g
        lo.append(la)
        eo.append(ea)
        la, ea = la + c.nL, ea + c.nE
    lay = np.frombuffer(np.full(5 * max(la, 1), CANARY, np.uint64).tobytes(), LAYER_DT).copy()
    arr = {f: np.full(max(ea, 1), CANARY, np.uint64) for f in ("meta", "w_lo", "w_hi")}
    sg = np.full((max(ea, 1), sw), CANARY, np.uint64) if sw else None
    for c, a, b in zip(ciphers, lo, eo):
        lay[a:a + c.nL] = c.layers
        for f in arr:
            arr[f][b:b + c.nE] = getattr(c, f)
        if sw:
            sg[b:b + c.nE] = c.sigma
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, np.uint64)).view(np.int64)).to(eng.device)
    sig = None
    if sw:
        flat = torch.zeros(sg.size + shift + 1, dtype=torch.int64, device=eng.device)
        flat[shift:shift + sg.size] = torch.from_numpy(sg.view(np.int64).reshape(-1)).to(eng.device)
        sig = flat[shift:shift + sg.size].view(sg.shape[0], sw)
        assert sig.data_ptr() % 16 == (8 * shift) % 16
    return DeviceBatch(n, t(np.array(lo, np.uint64)), t(np.array([c.nL for c in ciphers], np.uint64)),
                       torch.from_numpy(lay.view(np.int64).reshape(-1, 5)).to(eng.device), t(np.array(eo, np.uint64)),
                       t(np.array([c.nE for c in ciphers], np.uint64)), t(arr["meta"]), t(arr["w_lo"]), t(arr["w_hi"]), sig)


def check(out, want, sigma=False):
    """`out` is exactly `want`: counts, dense offsets, arrays of the planned size, every field of every cipher."""
    n = len(want)
    assert out.n == n
    lc = np.array([len(c.layers) for c in want], np.uint64)
    ec = np.array([len(c.meta) for c in want], np.uint64)
    ex = lambda c: np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.uint64) if n else c
    assert np.array_equal(u64(out.l_cnt)[:n], lc) and np.array_equal(u64(out.e_cnt)[:n], ec)
    assert np.array_equal(u64(out.l_off)[:n], ex(lc)) and np.array_equal(u64(out.e_off)[:n], ex(ec))
    assert out.layers.shape[0] == int(lc.sum())
    for f in ("meta", "w_lo", "w_hi"):
        assert getattr(out, f).shape[0] == int(ec.sum()), f
    assert (out.sigma is not None) == sigma
    if sigma:
        assert out.sigma.shape[0] == int(ec.sum())
    got = out.to_host()
    for k, (g, w) in enumerate(zip(got, want)):
        assert gm.same(g, w, sigma), k


def canvas(eng, m, lcap, ecap, sw=0):
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    f = lambda *shape: torch.full(shape, CANARY, dtype=torch.int64, device=eng.device)
    k = max(m, 1)
    return DeviceBatch(m, f(k), f(k), f(max(lcap, 1), 5), f(k), f(k), f(max(ecap, 1)), f(max(ecap, 1)), f(max(ecap, 1)),
                       f(max(ecap, 1), sw) if sw else None)


def untouched(D, index=True, rows=True):
    ts = ([D.l_off, D.l_cnt, D.e_off, D.e_cnt] if index else []) + \
         ([D.layers, D.meta, D.w_lo, D.w_hi] + ([D.sigma] if D.sigma is not None else []) if rows else [])
    return all(bool((t == CANARY).all()) for t in ts)


class Raw:
    """The two ABI calls on explicit arguments; keeps what the structures point to alive."""

    def __init__(self, eng, srcs, m, pick_src, pick_idx, n_src=None):
        import pvac_hfhe_cppbyv_amd as pv
        self.eng = eng
        self.structs = (pv.CtBatch * max(len(srcs), 1))(*[s.struct() for s in srcs])
        self.ps = None if pick_src is None else eng._index_tensor(pick_src, np.uint32)
        self.pi = None if pick_idx is None else eng._index_tensor(pick_idx)
        self.G = pv.Gather(C.cast(self.structs, C.c_void_p), len(srcs) if n_src is None else n_src, 0, m,
                           None if self.ps is None else self.ps.data_ptr(), None if self.pi is None else self.pi.data_ptr())
        self.tot = (C.c_uint64 * 2)()

    def plan(self, D):
        sd = D.struct()
        rc = self.eng.lib.pvac_hip_batch_gather_plan(self.eng.ctx, C.byref(self.G), C.byref(sd), self.tot)
        self.eng.sync()
        return rc

    def exec(self, D, lcap=None, ecap=None):
        sd = D.struct()
        rc = self.eng.lib.pvac_hip_batch_gather_exec(self.eng.ctx, C.byref(self.G), C.byref(sd),
                                                     int(self.tot[0]) if lcap is None else lcap,
                                                     int(self.tot[1]) if ecap is None else ecap)
        self.eng.sync()
        return rc


def check_canvas(D, want, sigma=False):
    """A canvas after exec: the gathered ciphers, then canaries in every slot past the totals."""
    from pvac_hfhe_cppbyv_amd import LAYER_DT
    n = len(want)
    nl, ne = sum(len(c.layers) for c in want), sum(len(c.meta) for c in want)
    lo, eo = u64(D.l_off), u64(D.e_off)
    assert np.array_equal(u64(D.l_cnt)[:n], [len(c.layers) for c in want])
    assert np.array_equal(u64(D.e_cnt)[:n], [len(c.meta) for c in want])
    assert np.array_equal(lo[:n], np.concatenate([[0], np.cumsum([len(c.layers) for c in want])[:-1]]))
    assert np.array_equal(eo[:n], np.concatenate([[0], np.cumsum([len(c.meta) for c in want])[:-1]]))
    lay = D.layers.cpu().numpy()
    want_l = np.concatenate([c.layers for c in want]) if nl else np.zeros(0, LAYER_DT)
    assert lay[:nl].tobytes() == np.ascontiguousarray(want_l).tobytes()
    assert (lay[nl:] == CANARY).all()
    for f in ("meta", "w_lo", "w_hi"):
        got = u64(getattr(D, f))
        assert np.array_equal(got[:ne], np.concatenate([getattr(c, f) for c in want])), f
        assert (got[ne:] == CANARY).all(), f
    if sigma:
        got = u64(D.sigma)
        assert np.array_equal(got[:ne], np.concatenate([c.sigma for c in want]))
        assert (got[ne:] == CANARY).all()


# ---------------------------------------------------------------------------------------- 1. mixed sources
@pytest.fixture(scope="module")
def mixed(eng, codec):
    """(device batches, host lists): a dense ragged batch with a fully empty cipher and one with layers but
    no edges, a capacity-padded ct_mul output of 8 fresh pairs, and a chain result loaded weights-only."""
    rng = np.random.default_rng(11)
    H0 = make(rng, [2, 0, 3, 1, 4, 2], [5, 0, 0, 7, 12, 1])
    S0 = upload(eng, H0)
    S1 = eng.ct_mul(eng.gen_fresh(8, 21, 20), eng.gen_fresh(8, 22, 20), nonce_seed=23)
    eng.sync()
    eo, ec = u64(S1.e_off), u64(S1.e_cnt)
    assert (eo[1:] > eo[:-1] + ec[:-1]).any()   # padded
    S2 = codec.load_ct_device(eng, os.path.join(GOLD, "ref", "chain3.ct"), sigma=False)
    assert S2.sigma is None and S2.n == 1
    return [S0, S1, S2], [H0, S1.to_host(), S2.to_host()]


def test_a_permutation_with_repeats_over_three_sources(eng, mixed):
    S, H = mixed
    ps = [2, 0, 1, 1, 0, 0, 2, 1, 0, 0, 1, 0, 1, 1]
    pi = [0, 4, 7, 0, 1, 2, 0, 7, 5, 3, 3, 0, 5, 2]
    check(eng.gather(S, ps, pi), gm.gather(H, ps, pi))
    # the same picks as CUDA tensors
    import torch
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device=eng.device)
    check(eng.gather(S, dev(ps, torch.int32), dev(pi, torch.int64)), gm.gather(H, ps, pi))


def test_a_source_may_go_unused_and_m_may_be_zero(eng, mixed):
    S, H = mixed
    ps, pi = [2, 0, 0, 2], [0, 3, 4, 0]
    check(eng.gather(S, ps, pi), gm.gather(H, ps, pi))
    before = eng.gather_path_counts()
    check(eng.gather(S, [], []), [])
    check(eng.gather([], [], []), [])
    check(eng.cat([]), [])
    assert eng.gather_path_counts() == before   # m == 0 launches nothing and counts nothing


def test_one_source_without_pick_src_and_no_picks_at_all(eng, mixed):
    S, H = mixed
    for j in range(3):
        idx = np.arange(S[j].n)[::-1].copy()
        check(eng.select(S[j], idx), gm.gather([H[j]], None, idx))
    before = eng.gather_path_counts()
    check(eng.cat(S), gm.gather(H))
    check(eng.cat([S[2], S[0], S[0]]), gm.gather([H[2], H[0], H[0]]))
    after = eng.gather_path_counts()
    assert after["narrow"] - before["narrow"] == 2 and after["wide"] == before["wide"]
    assert after["ciphers"] - before["ciphers"] == 15 + 13 and after["tiles"] > before["tiles"]
    from pvac_hfhe_cppbyv_amd import PvacError
    with pytest.raises(PvacError):
        eng.gather(S, None, [0])            # pick_src null needs exactly one source
    with pytest.raises(PvacError):
        eng.gather(S, [0], None)


# ---------------------------------------------------------------------------------------- 2. parity and bounds
@pytest.mark.parametrize("sw", [0, 2])
def test_all_four_parity_combinations_and_the_slots_past_the_totals(eng, sw):
    rng = np.random.default_rng(2 + sw)
    e_cnt, l_cnt = [3, 5, 4, 7, 1, 6, 9, 33], [1, 3, 2, 5, 0, 1, 2, 3]
    gaps = [0, 0, 1, 0, 2, 0, 0, 3]
    H = make(rng, l_cnt, e_cnt, sw)
    X = upload(eng, H, gaps, sw)
    pick = [0, 0, 2, 1, 1, 3, 6, 5, 4, 7, 7, 7]
    src_off, at = u64(X.e_off), 0
    combos = set()
    for k in pick:
        if e_cnt[k] >= 3:
            combos.add((int(src_off[k]) & 1, at & 1))
        at += e_cnt[k]
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for t in (X.meta, X.w_lo, X.w_hi):
        assert t.data_ptr() % 16 == 0   # so the offsets' parities are the addresses'
    want = gm.gather([H], None, pick)
    nl, ne = sum(len(c.layers) for c in want), sum(len(c.meta) for c in want)
    D = canvas(eng, len(pick), nl + 7, ne + 9, sw)
    r = Raw(eng, [X], len(pick), None, pick)
    assert r.plan(D) == 0 and list(r.tot) == [nl, ne]
    assert untouched(D, index=False)
    assert r.exec(D, nl + 7, ne + 9) == 0
    check_canvas(D, want, sigma=bool(sw))


# ---------------------------------------------------------------------------------------- 3. sigma paths
def test_sigma_rows_of_two_files_on_the_wide_path(eng, codec):
    A = codec.load_ct_device(eng, os.path.join(GOLD, "bounty", "a.ct"))
    B = codec.load_ct_device(eng, os.path.join(GOLD, "bounty", "b.ct"))
    assert A.sigma is not None and A.sigma.shape[1] == 128
    before = eng.gather_path_counts()
    out = eng.gather([A, B], [1, 0, 1], [0, 0, 0])
    after = eng.gather_path_counts()
    check(out, gm.gather([A.to_host(), B.to_host()], [1, 0, 1], [0, 0, 0]), sigma=True)
    assert after["wide"] - before["wide"] == 1 and after["narrow"] == before["narrow"]
    # sigma=False over sigma-carrying sources copies none, and counts under the 8-byte path
    out = eng.cat([A, B], sigma=False)
    check(out, gm.gather([A.to_host(), B.to_host()]), sigma=False)
    assert eng.gather_path_counts()["narrow"] - after["narrow"] == 1


@pytest.mark.parametrize("sw,shift", [(3, 0), (128, 1)])
def test_odd_width_and_an_unaligned_base_take_the_8_byte_path(eng, sw, shift):
    rng = np.random.default_rng(30 + sw)
    H = make(rng, [1, 2, 0, 3], [4, 1, 0, 19], sw)
    X = upload(eng, H, [0, 1, 0, 2], sw, shift)
    before = eng.gather_path_counts()
    out = eng.select(X, [3, 0, 1, 2, 3])
    after = eng.gather_path_counts()
    check(out, gm.gather([H], None, [3, 0, 1, 2, 3]), sigma=True)
    assert out.sigma.shape[1] == sw
    assert after["narrow"] - before["narrow"] == 1 and after["wide"] == before["wide"]


def test_sigma_true_needs_sigma_on_every_source(eng, mixed):
    from pvac_hfhe_cppbyv_amd import PvacError
    S, _ = mixed
    with pytest.raises(PvacError):
        eng.cat(S, sigma=True)


# ---------------------------------------------------------------------------------------- 4. tile boundaries
def tile(eng, sw):
    out = (C.c_uint32 * 2)()
    assert eng.lib.pvac_hip_batch_gather_tile(sw, out) == 0
    return int(out[0]), int(out[1])


@pytest.mark.parametrize("sw", [0, 128])
def test_ciphers_at_the_edge_tile_boundaries(eng, sw):
    ept, _ = tile(eng, sw)
    sizes = [ept - 1, ept, ept + 1, 2 * ept + 1]
    rng = np.random.default_rng(40 + sw)
    H = make(rng, [2, 1, 3, 2], sizes, sw)
    X = upload(eng, H, [1, 0, 3, 0], sw)
    for i in range(4):   # alone: one cipher, its tiles the whole launch
        check(eng.select(X, [i]), [H[i]], sigma=bool(sw))
    before = eng.gather_path_counts()["tiles"]
    check(eng.select(X, [3, 1, 0, 2, 3]), gm.gather([H], None, [3, 1, 0, 2, 3]), sigma=bool(sw))
    assert eng.gather_path_counts()["tiles"] - before == (3 + 1 + 1 + 2 + 3) + 5   # edge tiles, then a layer tile each


def test_forty_thousand_layers_cross_the_layer_tiles(eng):
    from pvac_hfhe_cppbyv_amd import LAYER_DT
    _, lpt = tile(eng, 0)
    rng = np.random.default_rng(44)
    H = make(rng, [lpt - 1, 40000, lpt + 1, lpt, 2 * lpt + 1], [2, 5, 0, 1, 3])
    for c in H:   # synthetic BASE layers
        c.layers["rule"] = 0
    assert 40000 > 30000 and 40000 % lpt
    X = upload(eng, H)
    check(eng.select(X, [1, 4, 0, 3, 2, 1]), gm.gather([H], None, [1, 4, 0, 3, 2, 1]))


# ---------------------------------------------------------------------------------------- 5. one big, many small
def test_one_big_cipher_among_thousands_of_small_ones(eng):
    import torch
    rng = np.random.default_rng(5)
    n = 4097
    e_cnt = rng.integers(1, 4, n)
    l_cnt = rng.integers(1, 3, n)
    big = int(rng.integers(0, n))
    e_cnt[big], l_cnt[big] = 50001, 36
    H = make(rng, l_cnt.tolist(), e_cnt.tolist())
    X = upload(eng, H)
    perm = rng.permutation(n)
    out = eng.select(X, perm)
    dperm = torch.from_numpy(perm).to(eng.device)
    assert torch.equal(eng.sumdigest(out), eng.sumdigest(X)[dperm])
    assert np.array_equal(eng.commit_ct(out, with_sigma=False), eng.commit_ct(X, with_sigma=False)[perm])
    got = out.to_host()
    where_big = int(np.nonzero(perm == big)[0][0])
    for k in [where_big] + rng.choice(n, 63, replace=False).tolist():
        assert gm.same(got[k], H[perm[k]]), k
    lc, ec = u64(out.l_cnt), u64(out.e_cnt)
    assert np.array_equal(u64(out.l_off), np.concatenate([[0], np.cumsum(lc)[:-1]]))
    assert np.array_equal(u64(out.e_off), np.concatenate([[0], np.cumsum(ec)[:-1]]))
    assert out.meta.shape[0] == int(e_cnt.sum()) and out.layers.shape[0] == int(l_cnt.sum())


# ---------------------------------------------------------------------------------------- 6. errors
@pytest.fixture(scope="module")
def small(eng):
    rng = np.random.default_rng(6)
    HA, HB = make(rng, [2, 1, 3], [4, 0, 6]), make(rng, [1, 2], [3, 5])
    return [upload(eng, HA), upload(eng, HB)], [HA, HB]


@pytest.mark.parametrize("ps,pi", [([0, 2, 1], [0, 0, 0]), ([0, 1, 1], [2, 2, 0])])
def test_a_pick_out_of_range_is_einval_and_dst_is_untouched(eng, small, ps, pi):
    S, H = small
    D = canvas(eng, 3, 16, 16)
    r = Raw(eng, S, 3, ps, pi)
    assert r.plan(D) == EINVAL
    assert untouched(D)
    assert r.exec(D, 16, 16) == EINVAL      # a failed plan is no plan
    assert untouched(D)


def test_caps_one_below_the_totals_are_enomem_with_the_rows_untouched(eng, small):
    S, H = small
    ps, pi = [1, 0, 0, 1], [1, 2, 0, 0]
    want = gm.gather(H, ps, pi)
    nl, ne = sum(len(c.layers) for c in want), sum(len(c.meta) for c in want)
    D = canvas(eng, 4, nl, ne)
    r = Raw(eng, S, 4, ps, pi)
    assert r.plan(D) == 0 and list(r.tot) == [nl, ne]
    assert r.exec(D, nl - 1, ne) == ENOMEM and untouched(D, index=False)
    assert r.exec(D, nl, ne - 1) == ENOMEM and untouched(D, index=False)
    assert r.exec(D, nl, ne) == 0
    check_canvas(D, want)


def test_sigma_on_dst_needs_the_same_sigma_on_every_source(eng, small):
    S, H = small
    rng = np.random.default_rng(61)
    with3 = upload(eng, make(rng, [1], [2], 3), sw=3)
    with128 = upload(eng, make(rng, [1], [2], 128), sw=128)
    for srcs in ([S[0], with128], [with3, with128]):
        D = canvas(eng, 1, 8, 8, 128)
        assert Raw(eng, srcs, 1, [1], [0]).plan(D) == EINVAL
        assert untouched(D)
    D = canvas(eng, 1, 8, 8, 128)
    r = Raw(eng, [with128], 1, [0], [0])
    assert r.plan(D) == 0 and r.exec(D) == 0


def test_exec_takes_the_latest_plan_of_the_same_call_only(eng, small):
    S, H = small
    eng2 = type(eng)(device=0)
    D = canvas(eng2, 2, 16, 16)
    r = Raw(eng2, S, 2, [0, 1], [0, 0])
    assert r.exec(D, 16, 16) == EINVAL      # no plan on this context yet
    assert r.plan(D) == 0
    other = Raw(eng2, S, 1, [0], [0])
    assert other.exec(D, 16, 16) == EINVAL  # another m
    D2 = canvas(eng2, 2, 16, 16)
    assert r.exec(D2, 16, 16) == EINVAL     # another dst
    assert untouched(D2) and untouched(D, index=False)
    assert r.exec(D, 16, 16) == 0
    check_canvas(D, gm.gather(H, [0, 1], [0, 0]))


def test_the_null_pick_rules_and_the_source_limit(eng, small):
    import pvac_hfhe_cppbyv_amd as pv
    S, H = small
    D = canvas(eng, 5, 16, 32)
    assert Raw(eng, S, 1, None, [0]).plan(D) == EINVAL          # pick_src null with two sources
    assert Raw(eng, S, 1, [0], None).plan(D) == EINVAL          # pick_src without pick_idx
    assert Raw(eng, S, 4, None, None).plan(D) == EINVAL         # no picks: m must be 3 + 2
    assert Raw(eng, [], 1, [0], [0]).plan(D) == EINVAL          # ciphers without a source
    many = [S[0]] * (pv.GATHER_MAX_SOURCES + 1)
    assert Raw(eng, many, 1, [0], [0]).plan(D) == EINVAL
    assert untouched(D)
    r = Raw(eng, [S[0]] * pv.GATHER_MAX_SOURCES, 1, [pv.GATHER_MAX_SOURCES - 1], [2])
    assert r.plan(D) == 0 and r.exec(D) == 0
    check_canvas(D, [H[0][2]])
    D = canvas(eng, 5, 16, 32)
    r = Raw(eng, S, 5, None, None)
    assert r.plan(D) == 0 and r.exec(D) == 0
    check_canvas(D, H[0] + H[1])


# ---------------------------------------------------------------------------------------- 7. end to end
def test_two_files_become_one_on_the_device(eng, codec, tmp_path):
    a, b = os.path.join(GOLD, "bounty", "a.ct"), os.path.join(GOLD, "bounty", "b.ct")
    both = eng.cat([codec.load_ct_device(eng, a), codec.load_ct_device(eng, b)])
    out = str(tmp_path / "ab.ct")
    size = codec.save_ct_device(eng, both, out)
    want = codec.write_ct(codec.read_ct(a) + codec.read_ct(b), 8192, threads=1)
    with open(out, "rb") as f:
        assert f.read() == want
    assert size == len(want)


def test_lincomb_over_the_concatenation_of_two_products(eng, oracle):
    import lincomb_model as lm
    from helpers import Cipher
    C1 = eng.ct_mul(eng.gen_fresh(3, 71, 4), eng.gen_fresh(3, 72, 4), nonce_seed=73)
    C2 = eng.ct_mul(eng.gen_fresh(2, 74, 5), eng.gen_fresh(2, 75, 5), nonce_seed=76)
    X = eng.cat([C1, C2])
    pool = [Cipher(c.layers, c.meta, c.w_lo, c.w_hi) for c in C1.to_host() + C2.to_host()]
    seg_off, term = [0, 2, 2, 5, 6], [0, 3, 4, 1, 3, 2]
    got = eng.ct_lincomb(X, seg_off, term).to_host()
    want = lm.fold_segments(oracle, pool, seg_off, term)
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert lm.same(Cipher(g.layers, g.meta, g.w_lo, g.w_hi), w)


def test_split_inverts_cat(eng, mixed):
    S, H = mixed
    parts = eng.split(eng.cat(S), [s.n for s in S] + [0])
    assert len(parts) == 4
    for p, h in zip(parts, H + [[]]):
        check(p, h)


def test_a_pending_ct_mul_plan_survives_a_gather(eng):
    A, B = eng.gen_fresh(16, 81, 20), eng.gen_fresh(16, 82, 20)
    want = eng.ct_mul(A, B, nonce_seed=83).to_host()
    Cb, plan = eng.ct_mul_plan(A, B)
    both = eng.cat([A, B])
    assert both.n == 32
    got = eng.ct_mul(A, B, C_=Cb, plan=plan, nonce_seed=83).to_host()
    for g, w in zip(got, want):
        assert gm.same(g, w)
    check(both, A.to_host() + B.to_host())
