"""Pins tests/drbg_model.py, the model every generator test compares against, to published vectors:
FIPS-197 Appendix C.3 (AES-256) and SP 800-38A F.5.5 (CTR-AES256.Encrypt's counter blocks)."""
import numpy as np

import drbg_model as M

KEY_C3 = bytes(range(32))
KEY_F55 = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
CTR_F55 = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
F55 = ["0bdf7df1591716335e9a8b15c860c502", "5a6e699d536119065433863c8f657b94", "1bc12c9c01610d5d0d8bd6a3378eca62",
       "2956e1c8693536b1bee99c73a31576b6"]


def test_sbox_is_fips197():
    assert M.SBOX[0x00] == 0x63 and M.SBOX[0x01] == 0x7C and M.SBOX[0x53] == 0xED and M.SBOX[0xFF] == 0x16
    assert sorted(M.SBOX.tolist()) == list(range(256))


def test_fips197_c3():
    pt = np.frombuffer(bytes.fromhex("00112233445566778899aabbccddeeff"), dtype=np.uint8).reshape(1, 16)
    ct = M.encrypt_blocks(M.expand_key(KEY_C3), pt)
    assert bytes(ct[0]).hex() == "8ea2b7ca516745bfeafc49904b496089"


def test_sp800_38a_f55_blocks():
    blocks = M.counter_blocks(int.from_bytes(CTR_F55, "big"), 4)
    assert bytes(blocks[0]) == CTR_F55
    assert bytes(blocks[1]).hex() == "f0f1f2f3f4f5f6f7f8f9fafbfcfdff00"   # the byte carry
    assert bytes(blocks[3]).hex() == "f0f1f2f3f4f5f6f7f8f9fafbfcfdff02"
    ks = M.encrypt_blocks(M.expand_key(KEY_F55), blocks)
    assert [bytes(b).hex() for b in ks] == F55


def test_f55_as_one_word_stream():
    w = M.ctr_words(KEY_F55, CTR_F55, 8)
    assert int(w[0]) == 0x33161759F17DDF0B and int(w[1]) == 0x02C560C8158B9A5E
    assert w.astype("<u8").tobytes().hex() == "".join(F55)
    assert np.array_equal(M.ctr_words(KEY_F55, CTR_F55, 7), w[:7])   # an odd request drops the last 8 bytes


def test_counter_wraps_mod_2_128():
    b = M.counter_blocks((1 << 128) - 2, 4)
    assert [bytes(x).hex() for x in b] == ["ff" * 15 + "fe", "ff" * 16, "00" * 16, "00" * 15 + "01"]
    b = M.counter_blocks((5 << 64) | (2**64 - 1), 2)
    assert bytes(b[1]).hex() == "0000000000000006" + "00" * 8


def test_drbg_follows_90a_by_hand():
    """Instantiate and generate spelled out with the block cipher alone, against the class."""
    seed = bytes(range(48))
    enc = lambda K, V, k: M.encrypt_blocks(M.expand_key(K), M.counter_blocks(V, k)).reshape(-1).tobytes()
    xor = lambda a, b: bytes(x ^ y for x, y in zip(a, b))
    t = xor(enc(bytes(32), 1, 3), seed)            # Instantiate: K = 0, V = 0, Update(seed)
    K, V = t[:32], int.from_bytes(t[32:], "big")
    out = enc(K, V + 1, 3)[:40]                    # Generate 5 words: blocks V+1..V+3
    t = enc(K, V + 4, 3)                           # Update(0^48) from V + 3
    K2, V2 = t[:32], int.from_bytes(t[32:], "big")
    g = M.CtrDrbg(seed)
    assert g.generate(5).astype("<u8").tobytes() == out
    assert (g.K, g.V) == (K2, V2) and g.counts() == (1, 3, 0, 0)
    assert len(g.generate(0)) == 0 and (g.K, g.V) == (K2, V2) and g.counts() == (1, 3, 0, 0)
    e = bytes(range(100, 148))
    t = xor(enc(K2, V2 + 1, 3), e)                 # Reseed(e)
    g.reseed(e)
    assert (g.K, g.V) == (t[:32], int.from_bytes(t[32:], "big")) and g.counts() == (1, 3, 1, 0)
