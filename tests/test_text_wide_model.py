"""The CPU model of enc_fp_depth / enc_value_depth (tests/text_model.py) against the reference-minted
fixtures of tests/golden/text_wide (tools/mint_text_wide.cpp): plans above 256 pre-merge edges per half,
where tests/golden/text does not pin it. Every cipher from its own draw segment. CPU only."""
import numpy as np
import pytest

import text_model as tm
import text_wide_cases as tw
from helpers import Cipher, fixture_secret, read_u64

CASES = tw.CASES


@pytest.fixture(scope="module")
def key():
    sk, man, _ = fixture_secret()
    assert man["canon_tag"] == tw.MAN["canon_tag"]
    return sk, man["canon_tag"], read_u64("powg_B.u64")


def test_fixture_set_is_the_issue_set():
    assert set(CASES) == {"fpwide", "valwide", "b1875", "steep", "t2one", "t2zero"}
    assert [tw.npre(h) for h in (124, 125, 126, 200, 400, 1000)] == [255, 257, 260, 401, 782, 1923]
    assert [tm.plan_noise(h) for h in (125, 126)] == [(69, 37), (69, 38)]
    fp = CASES["fpwide"]["ciphers"]
    assert [c["hint"] for c in fp] == [125, 126, 200, 400, 1000] and all(c["kind"] == tm.FP and c["layers"] == 1 for c in fp)
    P = (1 << 127) - 1
    assert fp[1]["v_lo"] | fp[1]["v_hi"] << 64 == P and fp[2]["v_hi"] >> 63 == 1   # non-canonical word pairs
    assert 256 < fp[3]["edges"] <= 674 and fp[4]["edges"] <= 674                 # merged down to at most 2 B
    val = CASES["valwide"]["ciphers"]
    assert [(c["kind"], c["hint"], c["layers"]) for c in val] == [(1, 125, 2), (1, 300, 2), (1, 125, 2)] and val[2]["v_lo"] == 0
    b = CASES["b1875"]
    assert len(bytes.fromhex(b["msg_hex"])) == 1875 and len(b["ciphers"]) == 126
    assert [c["hint"] for c in b["ciphers"][-3:]] == [124, 125, 126]
    st = CASES["steep"]
    noise = tm.case_noise(st)
    assert noise == (120.0, 0.55, 400.0) and [tw.npre(h, noise) for h in (4, 5, 6)][1:] == [257, 307] and tw.npre(4, noise) <= 256
    assert [c["hint"] for c in st["ciphers"]] == [0, 2, 3, 4, 5, 6]
    assert tm.plan_noise(125, tm.case_noise(CASES["t2one"])) == (126, 0)
    assert tm.plan_noise(125, tm.case_noise(CASES["t2zero"])) == (0, 84)
    for c in tw.MAN["cases"]:   # the items a message implies are the ones the reference encrypted
        assert c["sigma"] is False and c["parts"] >= 1
        if c["kind"] == "text":
            assert [(k, v, h) for k, v, h, _, _ in tm.case_items(c)] == tm.text_items(bytes.fromhex(c["msg_hex"]))


# (case, ciphers): a CPU PRF evaluation per noise group, about 10 ms each, bounds what is picked
PICKS = [("fpwide", [0, 1, 2]), ("valwide", [2]), ("b1875", [124, 125]), ("steep", [4, 5]), ("t2one", [0]), ("t2zero", [0])]


@pytest.mark.parametrize("name,pick", PICKS, ids=[p[0] for p in PICKS])
def test_model_reproduces_wide_fixtures(oracle, key, name, pick):
    """Layers, order and weights of ciphers at hints 125, 126 and 200, a wide enc_zero_depth, the two wide
    ciphers of the 1,875-byte message, the wide blocks under the steep slope, and the Z2-only and Z3-only
    plans."""
    sk, canon, powg = key
    case = CASES[name]
    model = tm.Model(oracle, sk, canon, powg, None, tm.case_noise(case))
    draws, refs, items = tw.case_draws(case), tw.case_ciphers(case), tm.case_items(case)
    assert len(refs) == len(items) and len(draws) == case["draws"]
    for i in pick:
        kind, v, hint, off, cnt = items[i]
        assert tw.npre(hint, tm.case_noise(case)) > 256
        c, st = model.enc_item(kind, v, hint, draws[off:off + cnt])
        assert st == 0
        tw.records_equal(c, refs[i], (name, i))
        assert (c.nL, c.nE) == (case["ciphers"][i]["layers"], case["ciphers"][i]["edges"])
        # one word short and the model runs out: the segment is exactly what the reference drew
        assert model.enc_item(kind, v, hint, draws[off:off + cnt - 1])[1] == 1


def test_wide_fixture_messages_decrypt(oracle, key):
    sk, canon, powg = key
    for name in ("b1875", "steep"):
        case = CASES[name]
        vals = []
        for c in tw.case_ciphers(case):
            R = np.zeros(2 * c.nL, np.uint64)
            for i, L in enumerate(c.layers):
                R[2 * i:2 * i + 2] = oracle.prf_R(sk, canon, (int(L["ztag"]), int(L["nonce_lo"]), int(L["nonce_hi"])))
            lo, hi = oracle.dec(Cipher(c.layers, c.meta, c.w_lo, c.w_hi), powg, R)
            vals.append(lo | (hi << 64))
        assert tm.text_unpack(vals) == (bytes.fromhex(case["msg_hex"]), 0), name
