"""The CPU model of enc_fp_depth / enc_text (tests/text_model.py) against the reference-minted
fixtures of tests/golden/text (tools/mint_text.cpp): every cipher from its own draw segment, the
value form against the pinned oracle, and the fixtures decrypting to their messages. CPU only."""
import numpy as np
import pytest

import text_model as tm
from helpers import Cipher, fixture_secret, read_u64, write_ct

MAN = tm.manifest()
CASES = {c["name"]: c for c in MAN["cases"]}


@pytest.fixture(scope="module")
def key():
    sk, man, _ = fixture_secret()
    assert man["canon_tag"] == MAN["canon_tag"]
    return sk, man["canon_tag"], read_u64("powg_B.u64")


def _same(got, ref, sigma):
    assert got.nL == ref.nL and got.nE == ref.nE
    for f in ("rule", "ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(got.layers[f], ref.layers[f]), f
    assert np.array_equal(got.meta, ref.meta)
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi)
    if sigma:
        assert write_ct([got]) == write_ct([ref])


def test_fixture_set_is_the_issue_set():
    assert set(CASES) == {"empty", "one", "b15", "b16", "b30", "b31", "utf8", "b240", "b1845", "nonoise", "bump", "fpraw"}
    assert [len(bytes.fromhex(CASES[k]["msg_hex"])) for k in ("empty", "one", "b15", "b16", "b30", "b31", "b240", "b1845")] == \
        [0, 1, 15, 16, 30, 31, 240, 1845]
    assert CASES["b1845"]["ciphers"][-1]["hint"] == 124 and CASES["b240"]["ciphers"][-1]["hint"] == 17
    assert tm.plan_noise(2) == (4, 2) and 8 + 2 * tm.plan_noise(124)[0] + 3 * tm.plan_noise(124)[1] == 255
    assert tm.plan_noise(0, tm.case_noise(CASES["nonoise"])) == (0, 0)
    assert tm.plan_noise(2, tm.case_noise(CASES["bump"])) == (2, 0)      # one group, bumped to two
    P = (1 << 127) - 1
    assert [c["v_lo"] | (c["v_hi"] << 64) for c in CASES["fpraw"]["ciphers"]] == [0, 1, P - 1, P, 1 << 127, (1 << 128) - 1]
    for c in MAN["cases"]:   # the items a message implies are the ones the reference encrypted
        if c["kind"] == "text":
            msg = bytes.fromhex(c["msg_hex"])
            assert [(k, v, h) for k, v, h, _, _ in tm.case_items(c)] == tm.text_items(msg)


@pytest.mark.parametrize("name", ["empty", "one", "b15", "b16", "b30", "b31", "utf8", "nonoise", "bump", "fpraw"])
def test_model_reproduces_sigma_fixtures(oracle, H_dense, key, name):
    """Byte-exact, sigma rows included."""
    sk, canon, powg = key
    case = CASES[name]
    model = tm.Model(oracle, sk, canon, powg, H_dense, tm.case_noise(case))
    draws, refs = tm.case_draws(case), tm.case_ciphers(case)
    got = []
    for (kind, v, hint, off, cnt), ref in zip(tm.case_items(case), refs):
        c, st = model.enc_item(kind, v, hint, draws[off:off + cnt], sigma=True)
        assert st == 0
        _same(c, ref, True)
        got.append(c)
    with open(tm.os.path.join(tm.TEXT, name + ".ct"), "rb") as f:
        assert write_ct(got) == f.read()


def _long_case(oracle, key, name, pick):
    sk, canon, powg = key
    case = CASES[name]
    model = tm.Model(oracle, sk, canon, powg, None, tm.case_noise(case))
    draws, refs = tm.case_draws(case), tm.case_ciphers(case)
    assert len(refs) == len(case["ciphers"])
    items = tm.case_items(case)
    for i in (range(len(items)) if pick is None else pick):
        kind, v, hint, off, cnt = items[i]
        c, st = model.enc_item(kind, v, hint, draws[off:off + cnt])
        assert st == 0
        _same(c, refs[i], False)


def test_model_reproduces_long_fixtures(oracle, key):
    """Weights and layers of every cipher of the 240-byte message (hints 2 .. 17) and of the length,
    first, a middle and the two last ciphers of the 1,845-byte one (hints 2, 63, 123, 124): a cipher
    costs one CPU PRF evaluation per noise group, 105 at hint 124."""
    _long_case(oracle, key, "b240", None)
    _long_case(oracle, key, "b1845", [0, 1, 62, 122, 123])


@pytest.mark.slow
def test_model_reproduces_every_cipher_of_the_longest_fixture(oracle, key):
    _long_case(oracle, key, "b1845", None)


@pytest.mark.parametrize("hint", [0, 2, 16])
def test_value_item_equals_oracle_enc_value(oracle, key, hint):
    sk, canon, powg = key
    rng = np.random.default_rng(500 + hint)
    words = rng.integers(0, 2**64, 1024, dtype=np.uint64)
    v = int(rng.integers(0, 2**64, dtype=np.uint64))
    ref, used = oracle.enc_value(sk, v, words, powg, canon_tag=canon, depth=hint)
    got, st = tm.Model(oracle, sk, canon, powg).enc_item(tm.VALUE, v, hint, words[:used])
    assert st == 0
    _same(got, ref, False)
    assert tm.Model(oracle, sk, canon, powg).enc_item(tm.VALUE, v, hint, words[:used - 1])[1] == 1


def test_fixture_messages_decrypt_and_unpack(oracle, key):
    sk, canon, powg = key
    for case in MAN["cases"]:
        if case["kind"] != "text":
            continue
        vals = []
        for c in tm.case_ciphers(case):
            R = np.zeros(2 * c.nL, np.uint64)
            for i, L in enumerate(c.layers):
                R[2 * i:2 * i + 2] = oracle.prf_R(sk, canon, (int(L["ztag"]), int(L["nonce_lo"]), int(L["nonce_hi"])))
            lo, hi = oracle.dec(Cipher(c.layers, c.meta, c.w_lo, c.w_hi), powg, R)
            vals.append(lo | (hi << 64))
        assert tm.text_unpack(vals) == (bytes.fromhex(case["msg_hex"]), 0), case["name"]


def test_unpack_flags_of_the_restatement():
    assert tm.text_unpack([]) == (b"", 0)
    assert tm.text_unpack([3, int.from_bytes(b"abcdef", "little")]) == (b"abc", 0)
    assert tm.text_unpack([40, int.from_bytes(b"abcdef", "little")]) == (b"abcdef" + b"\0" * 9, 2)
    assert tm.text_unpack([2 | (1 << 64), int.from_bytes(b"abcdef", "little")]) == (b"ab", 1)
