"""GPU parity of ct_recrypt and its parts (k_recrypt.hip): sigma popcounts against numpy,
ubk_apply against the numpy bit permutation, the batched compact_edges + compact_layers against the
CPU oracle (ct_add with an empty cipher at edge_budget 0), and ct_recrypt against the Python model of
tests/recrypt_model.py (reference ops/recrypt.hpp:26-41), fixtures of the unmodified reference
included."""
import json
import os

import numpy as np
import pytest

import recrypt_model as rm
from helpers import GOLD, LAYER_DT, REF, Cipher, read_ct, read_u64
from test_gpu_add_merge import _mk, _same

pytestmark = pytest.mark.gpu

RC = os.path.join(GOLD, "recrypt")
P_LO, P_HI = np.uint64(2**64 - 1), np.uint64(2**63 - 1)


def _bits(m_bits):
    return (m_bits + 63) // 64


def _padded_batch(engine, ciphers, words, pad=3, misalign=False):
    """Capacity-padded device batch: `pad` unused slots after every cipher, filled with 0xFF.. (a read
    past e_cnt shows); misalign: the sigma array starts 8 bytes off a 16-byte boundary."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    n = len(ciphers)
    lc = np.array([c.nL for c in ciphers], np.uint64)
    ec = np.array([c.nE for c in ciphers], np.uint64)
    lo = np.concatenate([[0], np.cumsum(lc + np.uint64(1))[:-1]]).astype(np.uint64)
    eo = np.concatenate([[0], np.cumsum(ec + np.uint64(pad))[:-1]]).astype(np.uint64)
    nl, ne = int((lc + np.uint64(1)).sum()), int((ec + np.uint64(pad)).sum())
    layers = np.zeros(nl, LAYER_DT)
    layers.view(np.uint8)[:] = 0xFF
    meta = np.full(ne, 2**64 - 1, np.uint64)
    wlo, whi = meta.copy(), meta.copy()
    sg = np.full((ne, words), 2**64 - 1, np.uint64)
    for i, c in enumerate(ciphers):
        a, b = int(lo[i]), int(eo[i])
        layers[a:a + c.nL] = c.layers
        meta[b:b + c.nE], wlo[b:b + c.nE], whi[b:b + c.nE] = c.meta, c.w_lo, c.w_hi
        sg[b:b + c.nE] = c.sigma
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(engine.device)
    if misalign:
        flat = torch.empty(ne * words + 1, dtype=torch.int64, device=engine.device)
        sig = flat[1:].view(ne, words)
        sig.copy_(dev(sg))
        assert sig.data_ptr() % 16 == 8
    else:
        sig = dev(sg)
    return DeviceBatch(n, dev(lo), dev(lc), dev(layers.view(np.int64).reshape(-1, 5)), dev(eo), dev(ec), dev(meta),
                       dev(wlo), dev(whi), sig)


def _dev_batch(engine, ciphers):
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    return DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in ciphers],
                                 engine.device, sigma=True)


def _sigma_rows(rng, ne, m_bits, first=0):
    """Rows cycling through: all ones, one bit at 0 / 63 / 64 / m_bits - 1, random."""
    w = _bits(m_bits)
    s = np.zeros((ne, w), np.uint64)
    for r in range(ne):
        k = (first + r) % 6
        if k == 0:
            s[r] = np.uint64(2**64 - 1)
            if m_bits % 64:
                s[r, -1] = np.uint64((1 << (m_bits % 64)) - 1)
        elif k == 5:
            s[r] = rng.integers(0, 2**64, w, dtype=np.uint64)
            if m_bits % 64:
                s[r, -1] &= np.uint64((1 << (m_bits % 64)) - 1)
        else:
            pos = (0, 63, 64, m_bits - 1)[k - 1]
            s[r, pos // 64] = np.uint64(1 << (pos % 64))
    return s


def _plain(rng, nl, ne, m_bits, first=0):
    c = _mk(rng, nl, ne)
    return Cipher(c.layers, c.meta, c.w_lo, c.w_hi, _sigma_rows(rng, c.nE, m_bits, first))


def _engine(m_bits=8192, **kw):
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, m_bits=m_bits, **kw)


# ------------------------------------------------------------------------------ popcount
@pytest.mark.parametrize("m_bits,misalign", [(8192, False), (8192, True), (320, False)])
def test_sigma_popcount(m_bits, misalign):
    """0 / 1 / 63 / 64 / 65 / 513 edges in one capacity-padded batch whose unused slots are all ones;
    m_bits = 320 (5 words per row) and a sigma array off the 16-byte boundary take the kernel's
    8-byte path."""
    rng = np.random.default_rng(5 + m_bits)
    eng = _engine(m_bits)
    cs = [_plain(rng, 2, ne, m_bits, first=i) for i, ne in enumerate((0, 1, 63, 64, 65, 513))]
    X = _padded_batch(eng, cs, _bits(m_bits), misalign=misalign)
    got = eng.sigma_popcount(X).cpu().numpy().view(np.uint64)
    want = np.array([rm.popcount(c.sigma) for c in cs], np.uint64)
    assert np.array_equal(got, want)
    dens = eng.sigma_density(X)
    assert dens[0] == 0.0
    for i in range(1, len(cs)):
        assert dens[i] == float(np.longdouble(int(want[i])) / np.longdouble(cs[i].nE * m_bits))


# ------------------------------------------------------------------------------ ubk_apply
def _perms(m_bits, manifest):
    rng = np.random.default_rng(m_bits)
    out = {"identity": np.arange(m_bits, dtype=np.int32), "reversal": np.arange(m_bits, dtype=np.int32)[::-1].copy()}
    if m_bits == 8192:
        out["fixture"] = rm.gen_ubk(manifest["canon_tag"], m_bits)[1]
    else:
        out["random"] = rng.permutation(m_bits).astype(np.int32)
    return out


@pytest.mark.parametrize("m_bits", [8192, 320])
def test_ubk_apply(manifest, m_bits):
    """Identity, reversal and the fixture key's permutation: one-bit rows land exactly at inv[src],
    random rows of 1 / 3 / 130 edges match the numpy model, a masked cipher stays bit-identical, and
    the slots between the ciphers are not touched."""
    rng = np.random.default_rng(77 + m_bits)
    words = _bits(m_bits)
    eng = _engine(m_bits)
    ones = _plain(rng, 1, 4, m_bits)
    for r, pos in enumerate((0, 63, 64, m_bits - 1)):
        ones.sigma[r] = 0
        ones.sigma[r, pos // 64] = np.uint64(1 << (pos % 64))
    cs = [ones] + [_plain(rng, 2, ne, m_bits, first=5) for ne in (1, 3, 130, 0, 7)]
    for c in cs[1:]:
        c.sigma[:] = rng.integers(0, 2**64, c.sigma.shape, dtype=np.uint64)
    for name, inv in _perms(m_bits, manifest).items():
        eng.set_ubk(inv)
        for active in (None, np.array([1, 1, 0, 1, 1, 0], np.uint32)):
            X = _padded_batch(eng, cs, words)
            before = X.sigma.cpu().numpy().view(np.uint64).copy()
            eng.ubk_apply(X, active)
            after = X.sigma.cpu().numpy().view(np.uint64)
            want = before.copy()
            eo = X.e_off.cpu().numpy().view(np.uint64)
            for i, c in enumerate(cs):
                if active is None or active[i]:
                    want[int(eo[i]):int(eo[i]) + c.nE] = rm.apply_perm(c.sigma, inv, m_bits)
            assert np.array_equal(after, want), (name, active is not None)
            if active is None:
                for r, pos in enumerate((0, 63, 64, m_bits - 1)):
                    j = int(inv[pos])
                    row = after[r]
                    assert row[j // 64] == np.uint64(1 << (j % 64)) and rm.popcount(row) == 1, (name, pos)


def test_set_ubk_rejects_non_permutations():
    from pvac_hfhe_cppbyv_amd import PvacError
    eng = _engine(320)
    bad = np.arange(320, dtype=np.int32)
    bad[5] = 6
    for inv in (bad, np.arange(319, dtype=np.int32), np.arange(320, dtype=np.int32) - 1):
        with pytest.raises(PvacError):
            eng.set_ubk(inv)
    X = _padded_batch(eng, [_plain(np.random.default_rng(1), 1, 2, 320)], 5)
    with pytest.raises(PvacError):
        eng.ubk_apply(X)   # no set_ubk yet


# ------------------------------------------------------------------------------ compact
def _uniform_sigma(rng, c):
    return Cipher(c.layers, c.meta, c.w_lo, c.w_hi, rng.integers(0, 2**64, (c.nE, 128), dtype=np.uint64))


def _cancelling(rng, same_sigma):
    """Every edge twice with weights w and p - w: the sums are 0; with equal sigmas the XOR is 0 too
    (dropped), with different sigmas the group stays with w = 0."""
    half = _mk(rng, 3, 150, sigma=True)
    keep = (half.w_lo != 0) | (half.w_hi != 0)
    meta, lo, hi, sg = half.meta[keep], half.w_lo[keep], half.w_hi[keep], half.sigma[keep]
    other = sg if same_sigma else rng.integers(0, 2**63, sg.shape, dtype=np.uint64)
    extra = _mk(rng, 1, 10, sigma=True)   # a fourth layer with edges of its own: something survives
    em = (np.arange(10, dtype=np.uint64) << np.uint64(32)) | np.uint64(3)
    return Cipher(np.concatenate([half.layers, extra.layers]), np.concatenate([meta, meta, em]),
                  np.concatenate([lo, P_LO - lo, extra.w_lo]), np.concatenate([hi, P_HI - hi, extra.w_hi]),
                  np.concatenate([sg, other, extra.sigma]))


def _compact_cases(rng):
    cs = [
        _mk(rng, 3, 300, idx_range=8, sigma=True),                 # heavy duplicates in a narrow idx range
        _mk(rng, 2, 260, idx_range=20, sigma=True, noncanon=0.5),  # non-canonical weights in the folds
        _cancelling(rng, True),
        _cancelling(rng, False),
        _mk(rng, 0, 0, sigma=True),                                # empty cipher
        _mk(rng, 3, 0, sigma=True),                                # layers, no edge
    ]
    prod = _mk(rng, 5, 180, idx_range=30, sigma=True)              # PROD layers with parents, one unused layer
    prod.meta = (prod.meta & ~np.uint64(0xFFFFFFFF)) | np.minimum(prod.meta & np.uint64(0xFFFFFFFF), np.uint64(3))
    prod.meta[prod.meta & np.uint64(0xFFFFFFFF) == np.uint64(1)] += np.uint64(2)   # layer 1 only as a parent
    prod.layers["rule"][3] = 1
    prod.layers["pa"][3], prod.layers["pb"][3] = 0, 1
    cs.append(prod)
    unused = _mk(rng, 4, 90, sigma=True)                           # layer 2 referenced by nothing
    unused.meta[unused.meta & np.uint64(0xFFFFFFFF) == np.uint64(2)] += np.uint64(1)
    cs.append(unused)
    cs += [_mk(rng, 2, ne, idx_range=40, sigma=True) for ne in (1, 64, 65, 513)]
    return cs


def test_compact_vs_oracle(oracle):
    """Every shape of the merge path's tests, the last layer count inside the batched kernel's key
    space (21 layers at B = 337: 14,154 of 14,336 cells) and the first one above it (22: the merge
    path), in one batch; both paths ran and agree with the oracle."""
    rng = np.random.default_rng(91)
    eng = _engine()
    cs = _compact_cases(rng)
    cs += [_mk(rng, 21, 200, idx_range=50, sigma=True), _mk(rng, 22, 200, idx_range=50, sigma=True),
           _mk(rng, 40, 700, sigma=True)]
    X = _padded_batch(eng, cs, 128)
    out = eng.compact(X).to_host()
    for i, c in enumerate(cs):
        _same(out[i], rm.compact(oracle, c), sigma=True)
    assert out[2].nE < 20 < out[3].nE and out[2].nL == 1 and out[4].nL == 0 and out[5].nL == 0
    assert eng.compact_path_counts() == {"small": len(cs) - 2, "merge": 2}


def _oracle_compact_B(oracle, c, B):
    import ctypes as C
    from helpers import default_params
    prm = default_params(0, 0, B=B)
    e = rm.empty_cipher()
    oc, ov = oracle._out(c.nL, c.nE, True)
    assert oracle.lib.orc_ct_add(C.byref(prm), C.byref(oracle._view(c)), C.byref(oracle._view(e)), 0, C.byref(ov)) == 0
    return oracle._trim(oc, ov)


def test_compact_at_the_key_space_bound(oracle):
    """B = 256: 28 layers are exactly the 14,336 cells the batched kernel holds, 29 one layer more."""
    rng = np.random.default_rng(92)
    eng = _engine(B=256)
    cs = [_mk(rng, nl, 900, B=256, sigma=True) for nl in (28, 29)]
    for c in cs:   # the last cell of the key space is in use
        c.meta[0] = np.uint64(c.nL - 1) | (np.uint64(255) << np.uint64(32)) | (np.uint64(1) << np.uint64(48))
    out = eng.compact(_dev_batch(eng, cs)).to_host()
    for i, c in enumerate(cs):
        _same(out[i], _oracle_compact_B(oracle, c, 256), sigma=True)
    assert eng.compact_path_counts() == {"small": 1, "merge": 1}


def test_compact_needs_sigma():
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher, PvacError
    eng = _engine()
    c = _mk(np.random.default_rng(3), 2, 10)
    X = DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi)], eng.device)
    with pytest.raises(PvacError):
        eng.compact(X)


# ------------------------------------------------------------------------------ recrypt
def _skew(c, k):
    """s &= rotl(s, 1) on the first k edges: their density falls to a quarter."""
    s = c.sigma.copy()
    s[:k] &= (s[:k] << np.uint64(1)) | (s[:k] >> np.uint64(63))
    return Cipher(c.layers, c.meta, c.w_lo, c.w_hi, s)


def _with_ones(rng, ones):
    """25 edges whose sigmas hold exactly `ones` set bits (0.495 and 0.505 of 204,800 are integers)."""
    c = _mk(rng, 2, 25)
    bits = np.zeros(25 * 8192, np.uint8)
    bits[rng.permutation(25 * 8192)[:ones]] = 1
    sg = np.packbits(bits.reshape(25, 8192), axis=1, bitorder="little").view(np.uint64).reshape(25, 128)
    return Cipher(c.layers, c.meta, c.w_lo, c.w_hi, sg)


def _recrypt_batch(rng):
    u = lambda nl, ne, **kw: _uniform_sigma(rng, _mk(rng, nl, ne, **kw))
    cs = [u(2, 39), u(2, 40), u(8, 1222)]                                   # in range
    cs += [_skew(u(2, 39), k) for k in (1, 2, 4, 8, 20, 39)]
    zero, one = u(2, 39), u(2, 39)
    zero.sigma[:] = 0
    one.sigma[:] = np.uint64(2**64 - 1)                                     # the > 0.505 branch
    cs += [zero, one]
    cs += [_with_ones(rng, k) for k in (101376, 101375, 103424, 103425)]    # exactly at and one past the thresholds
    dbl = u(2, 39)
    cs.append(Cipher(dbl.layers, np.concatenate([dbl.meta, dbl.meta]), np.concatenate([dbl.w_lo, dbl.w_lo]),
                     np.concatenate([dbl.w_hi, dbl.w_hi]), np.concatenate([dbl.sigma, dbl.sigma])))   # duplicates
    cs.append(_skew(cs[-1], 30))                                            # duplicates that iterate
    prod = u(4, 120)
    prod.layers["rule"][3] = 1
    prod.layers["pa"][3], prod.layers["pb"][3] = 0, 1
    cs += [prod, _skew(prod, 40)]
    unused = u(4, 90)
    unused.meta[unused.meta & np.uint64(0xFFFFFFFF) == np.uint64(2)] += np.uint64(1)
    cs += [unused, _skew(unused, 12)]
    cs += [u(2, 0), u(0, 0), _skew(u(2, 64), 3), _skew(u(3, 65), 5)]
    return cs


@pytest.fixture(scope="module")
def recrypt_inputs(manifest):
    rng = np.random.default_rng(2024)
    cs = _recrypt_batch(rng)
    pool = [_uniform_sigma(rng, _mk(rng, 2, 39 + k)) for k in range(4)]
    picks = rng.integers(0, 2**64, (len(cs), 8), dtype=np.uint64)           # uniform over all 64 bits
    inv = rm.gen_ubk(manifest["canon_tag"], 8192)[1]
    return cs, pool, picks, inv


@pytest.mark.parametrize("pool_size", [1, 3, 4, 0])
def test_recrypt_batch_vs_model(oracle, recrypt_inputs, pool_size):
    cs, pool, picks, inv = recrypt_inputs
    pool = pool[:pool_size]
    want = [rm.recrypt(oracle, c, pool, picks[i], inv) for i, c in enumerate(cs)]
    its = [w[1] for w in want]
    if pool_size:
        assert 0 in its and 1 in its and 8 in its and any(2 <= k <= 7 for k in its), its
        assert (picks >> np.uint64(63)).any()   # draws a signed modulo would get wrong
        thr = [its[i] for i in range(11, 15)]
        assert thr[0] == 0 and thr[1] > 0 and thr[2] == 0 and thr[3] > 0, thr
    eng = _engine()
    eng.set_ubk(inv)
    X = _padded_batch(eng, cs, 128)
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    P = _dev_batch(eng, pool) if pool_size else DeviceBatch.empty(0, 0, 0, eng.device, sigma=True)
    out, iters = eng.ct_recrypt(X, P, picks)
    out = out.to_host()
    assert list(iters) == its
    for i, c in enumerate(cs):
        _same(out[i], want[i][0], sigma=True)


def _fixture_cases():
    with open(os.path.join(RC, "manifest.json")) as f:
        return json.load(f)


def test_recrypt_fixtures(oracle, manifest):
    """The unmodified reference's ct_recrypt outputs, byte for byte, from its own draws."""
    man = _fixture_cases()
    inv = np.fromfile(os.path.join(RC, "ubk_inv.i32"), dtype=np.int32)
    pool = read_ct(os.path.join(RC, "pool.ct"))
    cases = [k for k in man["cases"] if k["sigma"]]
    xs = [read_ct(os.path.join(RC, k["name"] + "_in.ct"))[0] for k in cases]
    picks = np.zeros((len(xs), 8), np.uint64)
    for i, k in enumerate(cases):
        picks[i, :len(k["draws"])] = np.array(k["draws"], np.uint64)
    eng = _engine()
    eng.set_ubk(inv)
    out, iters = eng.ct_recrypt(_dev_batch(eng, xs), _dev_batch(eng, pool), picks)
    out = out.to_host()
    H_digest = bytes.fromhex(manifest["H_digest"])
    for i, k in enumerate(cases):
        ref = read_ct(os.path.join(RC, k["name"] + "_out.ct"))[0]
        assert iters[i] == k["iterations"], k["name"]
        _same(out[i], ref, sigma=True, view=True)
        got = Cipher(out[i].layers, out[i].meta, out[i].w_lo, out[i].w_hi, out[i].sigma)
        assert oracle.commit(got, manifest["canon_tag"], H_digest).hex() == k["commit"], k["name"]


def test_recrypt_product_fixture(oracle, manifest):
    """ct_recrypt of the fresh x fresh product pair0 (1,219 edges with sigma): the reference's output
    is stored weights-only with its commit_ct digest, which covers the sigmas."""
    from pvac_hfhe_cppbyv_amd import MUL_WITH_SIGMA
    man = _fixture_cases()
    case = [k for k in man["cases"] if not k["sigma"]][0]
    inv = np.fromfile(os.path.join(RC, "ubk_inv.i32"), dtype=np.int32)
    pool = read_ct(os.path.join(RC, "pool.ct"))
    x = read_ct(os.path.join(REF, "pair0_x.ct"))[0]
    y = read_ct(os.path.join(REF, "pair0_y.ct"))[0]
    stream = read_u64("pair0_mul_stream.u64")
    eng = _engine(canon_tag=manifest["canon_tag"])
    assert eng.gen_H().hex() == manifest["H_digest"]
    eng.set_ubk(inv)
    import torch
    A, B = _dev_batch(eng, [x]), _dev_batch(eng, [y])
    Cb, plan = eng.ct_mul_plan(A, B)
    nn = 2 * x.nL * y.nL
    nonces = np.zeros(2 * plan.total_layer_slots, np.uint64)
    nonces[2 * (x.nL + y.nL):2 * (x.nL + y.nL) + nn] = stream[:nn]
    salts = np.zeros(plan.total_edge_slots, np.uint64)
    salts[:len(stream) - nn] = stream[nn:]
    dev = lambda a: torch.from_numpy(a.view(np.int64)).to(eng.device)
    prod = eng.ct_mul(A, B, nonces=dev(nonces), salts=dev(salts), flags=MUL_WITH_SIGMA, C_=Cb, plan=plan)
    picks = np.zeros((1, 8), np.uint64)
    picks[0, :len(case["draws"])] = np.array(case["draws"], np.uint64)
    out, iters = eng.ct_recrypt(prod, _dev_batch(eng, pool), picks)
    got = out.to_host()[0]
    ref = read_ct(os.path.join(RC, case["name"] + "_out.ct"))[0]
    assert iters[0] == case["iterations"]
    assert np.array_equal(got.meta, ref.meta)
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi)
    c = Cipher(got.layers, got.meta, got.w_lo, got.w_hi, got.sigma)
    assert oracle.commit(c, manifest["canon_tag"], bytes.fromhex(manifest["H_digest"])).hex() == case["commit"]
