"""The ragged encryption path on the GPU (pvac_hip_enc_items: k_enc_items.hip) and enc_text / dec_text
on top of it, against the reference-minted fixtures of tests/golden/text (each cipher from its own
draw segment) and, for a mixed batch no fixture covers, against the CPU model (tests/text_model.py,
itself pinned to the fixtures by test_text_model.py)."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import text_model as tm
from helpers import REF, Cipher, fixture_secret, read_ct, read_u64, write_ct

pytestmark = pytest.mark.gpu

MAN = tm.manifest()
CASES = {c["name"]: c for c in MAN["cases"]}
TEXT_DEFAULT = ["empty", "one", "b15", "b16", "b30", "b31", "utf8", "b240", "b1845"]


@pytest.fixture(scope="module")
def eng():
    from pvac_hfhe_cppbyv_amd import Engine
    sk, man, em = fixture_secret()
    e = Engine(device=0, canon_tag=man["canon_tag"])
    assert e.gen_H().hex() == man["H_digest"]
    e.set_secret(read_u64("sk_prf_k.u64"), read_u64("sk_lpn_s.u64"), em["lpn_n"], em["lpn_t"], em["lpn_tau_num"],
                 em["lpn_tau_den"])
    e.set_powg(read_u64("powg_B.u64"))
    return e


def _concat(names):
    """The cases' messages, their draw logs back to back and every cipher's (offset, count) in them."""
    msgs, logs, segs, base = [], [], [], 0
    for n in names:
        case = CASES[n]
        d = tm.case_draws(case)
        msgs.append(bytes.fromhex(case["msg_hex"]))
        segs += [(base + c["off"], c["cnt"]) for c in case["ciphers"]]
        logs.append(d)
        base += len(d)
    return msgs, np.concatenate(logs), segs


def _records_equal(got, ref, what):
    assert got.nL == ref.nL and got.nE == ref.nE, what
    for f in ("rule", "ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(got.layers[f], ref.layers[f]), (what, f)
    assert np.array_equal(got.meta, ref.meta), what
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi), what


def _bytes(cs):
    return write_ct([Cipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in cs])


def _check_text_cases(eng, names):
    msgs, rnd, segs = _concat(names)
    X, moff, st = eng.enc_text(msgs, rnd, rnd_off=segs, sigma=True)
    assert not st.any()
    out = X.to_host()
    digests = eng.commit_ct(X, with_sigma=True)
    for m, n in enumerate(names):
        case, mine = CASES[n], out[moff[m]:moff[m + 1]]
        assert len(mine) == len(case["ciphers"]), n
        for k, (c, rec) in enumerate(zip(mine, case["ciphers"])):
            assert c.nE == rec["edges"] and c.nL == rec["layers"], (n, k)
            assert digests[moff[m] + k].tobytes().hex() == rec["commit"], (n, k)
        if case["sigma"]:
            with open(os.path.join(tm.TEXT, n + ".ct"), "rb") as f:
                assert _bytes(mine) == f.read(), n
        else:
            for k, (c, ref) in enumerate(zip(mine, tm.case_ciphers(case))):
                _records_equal(c, ref, (n, k))
    return X, moff, msgs


def test_enc_text_reproduces_the_fixture_messages(eng):
    """Every default-Params message in one call, each cipher from its segment: the files' bytes (stored
    with sigma), the long messages' records, and every cipher's commit_ct with sigma. The last cipher
    of the 1,845-byte message is the hint-124 item (255 pre-merge edges)."""
    assert CASES["b1845"]["ciphers"][-1]["hint"] == 124
    X, moff, msgs = _check_text_cases(eng, TEXT_DEFAULT)
    assert eng.dec_text(X, moff) == msgs
    # weights-only: the same records, no sigma array
    lm, lr, ls = _concat(["b240", "b1845"])
    Y, yoff, st = eng.enc_text(lm, lr, rnd_off=ls, sigma=False)
    assert not st.any() and Y.sigma is None
    refs = tm.case_ciphers(CASES["b240"]) + tm.case_ciphers(CASES["b1845"])
    for k, (c, ref) in enumerate(zip(Y.to_host(), refs)):
        _records_equal(c, ref, k)


def test_enc_items_fpraw(eng):
    """Bare enc_fp_depth(v, 3) on plaintext words as given: 0, 1, p - 1, p, 2^127, 2^128 - 1."""
    case = CASES["fpraw"]
    X, st = eng.enc_items(tm.case_items(case), tm.case_draws(case), sigma=True)
    assert not st.any()
    out = X.to_host()
    assert all(c.nL == 1 for c in out)
    with open(os.path.join(tm.TEXT, "fpraw.ct"), "rb") as f:
        assert _bytes(out) == f.read()


def test_enc_items_mixed_batch_against_model(eng, oracle, H_dense):
    """67 items in one call (a partial last block of the 64-thread plan kernel): kinds alternate, hints
    from {0, 2, 15, 16, 17, 124} (both plan-record classes of the uniform path, the largest plan as an
    FP and as a VALUE item), seeded plaintexts and draws. Every item equals the model; 4 with sigma."""
    sk, man, _ = fixture_secret()
    rng = np.random.default_rng(0x7E87)
    hints = [(0, 2, 15, 16, 17)[i % 5] for i in range(67)]
    hints[6] = hints[41] = 124
    kinds = [i % 2 for i in range(67)]
    vals = [int(rng.integers(0, 2**64, dtype=np.uint64)) | (0 if k else int(rng.integers(0, 2**63, dtype=np.uint64)) << 64)
            for k in kinds]
    dh = eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in zip(kinds, vals, hints)])[2]
    offs = np.concatenate([[0], np.cumsum(dh)]).astype(np.int64)
    rnd = rng.integers(0, 2**64, int(offs[-1]), dtype=np.uint64)
    items = [(k, v, h, int(offs[i]), int(dh[i])) for i, (k, v, h) in enumerate(zip(kinds, vals, hints))]
    X, st = eng.enc_items(items, rnd, sigma=True)
    assert not st.any()
    out = X.to_host()
    with_sigma = {0, 6, 33, 66}
    model = tm.Model(oracle, sk, man["canon_tag"], read_u64("powg_B.u64"), H_dense)

    def one(i):
        k, v, h, o, c = items[i]
        return model.enc_item(k, v, h, rnd[o:o + c], sigma=i in with_sigma)

    with ThreadPoolExecutor(8) as pool:   # the CPU PRF dominates; the oracle calls drop the GIL
        refs = list(pool.map(one, range(67)))
    lo, eo = X.l_off.cpu().numpy(), X.e_off.cpu().numpy()
    for i, (ref, rst) in enumerate(refs):
        assert rst == 0
        _records_equal(out[i], ref, i)
        assert out[i].nL == 1 + kinds[i]
        if i in with_sigma:
            assert np.array_equal(out[i].sigma, ref.sigma), i
    # capacity-padded CSR: offsets are the prefix sums of the halves and of the pre-merge edge counts
    npre = [(1 + k) * (8 + 2 * tm.plan_noise(h)[0] + 3 * tm.plan_noise(h)[1]) for k, h in zip(kinds, hints)]
    assert list(lo) == list(np.concatenate([[0], np.cumsum([1 + k for k in kinds])[:-1]]))
    assert list(eo) == list(np.concatenate([[0], np.cumsum(npre)[:-1]]))


def test_enc_items_value_fixtures_of_the_uniform_entry(eng):
    """The 12 enc{i}.ct fixtures as VALUE items at hint 0: what test_enc_value_fixtures asks of
    pvac_hip_enc_value, byte for byte."""
    import json
    with open(os.path.join(REF, "enc_manifest.json")) as f:
        em = json.load(f)
    logs = [read_u64(f"enc{i}_stream.u64") for i in range(len(em["enc"]))]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in logs])])
    items = [(tm.VALUE, r["v"], 0, int(offs[i]), len(logs[i])) for i, r in enumerate(em["enc"])]
    X, st = eng.enc_items(items, np.concatenate(logs), sigma=True)
    assert not st.any()
    for i, c in enumerate(X.to_host()):
        with open(os.path.join(REF, f"enc{i}.ct"), "rb") as f:
            assert _bytes([c]) == f.read(), i


@pytest.mark.parametrize("name", ["nonoise", "bump"])
def test_enc_text_under_other_noise_params(eng, name):
    """A plan without noise groups, and one whose single group is bumped to two (hint 0 next to it
    still has none): the plans come from the context's noise fields, per item."""
    case = CASES[name]
    eng.set_noise(*tm.case_noise(case))
    try:
        X, moff, msgs = _check_text_cases(eng, [name])
        assert eng.dec_text(X, moff) == msgs
    finally:
        eng.set_noise()


def _raw(eng, items, rnd, X, ls, es):
    arr = eng._items(items)
    st = eng.torch.zeros(len(items), dtype=eng.torch.int32, device=eng.device)
    sx = X.struct()
    return eng.lib.pvac_hip_enc_items(eng.ctx, len(items), C.cast(arr, C.c_void_p), C.c_void_p(rnd.data_ptr()),
                                      rnd.numel(), C.byref(sx), ls, es, 1, C.c_void_p(st.data_ptr()))


def test_enc_items_refusals(eng):
    from pvac_hfhe_cppbyv_amd import DeviceBatch, PvacError
    case = CASES["b16"]
    items, draws, refs = tm.case_items(case), tm.case_draws(case), tm.case_ciphers(case)
    # a segment one word short: status 1 on that item only, its neighbours as in the fixture
    short = list(items)
    short[1] = short[1][:4] + (short[1][4] - 1,)
    X, st = eng.enc_items(short, draws, sigma=True)
    assert list(st) == [0, 1, 0]
    out = X.to_host()
    assert _bytes([out[0]]) == write_ct([refs[0]]) and _bytes([out[2]]) == write_ct([refs[2]])
    # hint 125 among valid items, an unknown kind, a range past the draws: nothing launched, C untouched
    ls, es, _ = eng.enc_items_caps(items)
    rnd = eng.torch.from_numpy(draws.view(np.int64)).to(eng.device)
    for bad, code in (((tm.FP, 5, 125, 0, 100), -38), ((2, 5, 2, 0, 100), -22), ((tm.FP, 5, 2, len(draws) - 10, 11), -22)):
        Y = DeviceBatch.empty(4, ls + 1, es + 600, eng.device, sigma=True)
        for t in (Y.l_off, Y.l_cnt, Y.e_off, Y.e_cnt, Y.layers, Y.meta, Y.w_lo, Y.w_hi, Y.sigma):
            t.fill_(-7)
        assert _raw(eng, items[:2] + [bad] + items[2:], rnd, Y, ls + 1, es + 600) == code, bad
        eng.sync()
        for t in (Y.l_off, Y.l_cnt, Y.e_off, Y.e_cnt, Y.layers, Y.meta, Y.w_lo, Y.w_hi, Y.sigma):
            assert bool((t == -7).all()), bad
    with pytest.raises(PvacError, match="-38"):
        eng.enc_items_caps([(tm.FP, 5, 125, 0, 0)])
    # caps one slot short
    for caps in ((ls - 1, es), (ls, es - 1)):
        with pytest.raises(PvacError, match="-12"):
            eng.enc_items(items, draws, sigma=True, caps=caps)
    assert eng.enc_items(items, draws, sigma=True, caps=(ls, es))[1].tolist() == [0, 0, 0]


def test_text_roundtrip_and_determinism(eng):
    """dec_text(enc_text(m)) = m for the fixture messages and 16 seeded random messages of 0 .. 100
    bytes in one batch on consecutive draws_hint segments; the same batch twice gives the same bytes."""
    rng = np.random.default_rng(0x7E88)
    msgs = [bytes.fromhex(CASES[n]["msg_hex"]) for n in TEXT_DEFAULT]
    msgs += [rng.integers(0, 256, int(rng.integers(0, 101)), dtype=np.uint8).tobytes() for _ in range(16)]
    items, _ = eng.text_items(msgs)
    total = int(eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in items])[2].sum())
    rnd = rng.integers(0, 2**64, total, dtype=np.uint64)
    X, moff, st = eng.enc_text(msgs, rnd)
    assert not st.any() and moff[-1] == len(items)
    assert eng.dec_text(X, moff) == msgs
    Y, _, st2 = eng.enc_text(msgs, rnd)
    assert not st2.any()
    for a, b in zip((X.l_off, X.l_cnt, X.e_off, X.e_cnt), (Y.l_off, Y.l_cnt, Y.e_off, Y.e_cnt)):
        assert bool((a == b).all())
    ne = int((X.e_off + X.e_cnt).max().item())
    for a, b in zip((X.layers, X.meta[:ne], X.w_lo[:ne], X.w_hi[:ne]), (Y.layers, Y.meta[:ne], Y.w_lo[:ne], Y.w_hi[:ne])):
        assert bool((a == b).all())
    xs, ys = X.to_host(), Y.to_host()
    assert all(np.array_equal(a.sigma, b.sigma) for a, b in zip(xs, ys))
