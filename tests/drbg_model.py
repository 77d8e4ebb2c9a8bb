"""An independent model of the library's generator, written from SP 800-90A rev. 1 §10.2.1's
pseudo-code (CTR_DRBG_Update, Instantiate, Reseed, Generate without a derivation function) over a
numpy-vectorised AES-256 written from FIPS-197: the S-box is computed from the GF(2^8) inverse and
the affine map, the cipher works on bytes (SubBytes, ShiftRows, MixColumns), no T-tables. Nothing
here comes from the library's aes256.hpp or drbg.hpp.

Word convention (the reference's csprng_u64 over the keystream bytes): word i of a generate call is
the little-endian u64 of keystream bytes 8i .. 8i+7; an odd request drops the last 8 bytes. The
counter V is the whole 128-bit block, big-endian, mod 2^128. The library's one deviation from 90A is
modelled too: no cap on a request's size.
"""
import numpy as np

MASK128 = (1 << 128) - 1


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11B
        b >>= 1
    return r


def _make_sbox():
    inv = [0] * 256
    for x in range(1, 256):   # x^254 = x^-1 in GF(2^8)
        y, e, b = 1, 254, x
        while e:
            if e & 1:
                y = _gmul(y, b)
            b = _gmul(b, b)
            e >>= 1
        inv[x] = y
    rot = lambda v, k: ((v << k) | (v >> (8 - k))) & 0xFF
    return np.array([b ^ rot(b, 1) ^ rot(b, 2) ^ rot(b, 3) ^ rot(b, 4) ^ 0x63 for b in inv], dtype=np.uint8)


SBOX = _make_sbox()
_X2 = np.array([_gmul(x, 2) for x in range(256)], dtype=np.uint8)
_X3 = np.array([_gmul(x, 3) for x in range(256)], dtype=np.uint8)
# ShiftRows on the FIPS-197 byte order (byte i = row i % 4, column i // 4): out[r + 4c] = in[r + 4((c + r) % 4)]
_SHIFT = np.array([(i % 4) + 4 * (((i // 4) + (i % 4)) % 4) for i in range(16)])


def expand_key(key: bytes):
    """FIPS-197 §5.2, Nk = 8: 15 round keys of 16 bytes."""
    assert len(key) == 32
    w = [list(key[4 * i:4 * i + 4]) for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = t[1:] + t[:1]
            t = [int(SBOX[b]) for b in t]
            t[0] ^= rcon
            rcon = _gmul(rcon, 2)
        elif i % 8 == 4:
            t = [int(SBOX[b]) for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return np.array(w, dtype=np.uint8).reshape(15, 16)


def encrypt_blocks(rk, blocks, piece=1 << 14):
    """AES-256 of (n, 16) u8 blocks under the round keys rk (15, 16), a cache-sized piece at a time."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    if len(blocks) > piece:
        return np.concatenate([_encrypt(rk, blocks[i:i + piece]) for i in range(0, len(blocks), piece)])
    return _encrypt(rk, blocks)


def _encrypt(rk, blocks):
    s = blocks ^ rk[0]
    for r in range(1, 15):
        s = SBOX[s][:, _SHIFT]
        if r < 14:
            c = s.reshape(-1, 4, 4)   # [block, column, row]
            a0, a1, a2, a3 = c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3]
            m = np.stack([_X2[a0] ^ _X3[a1] ^ a2 ^ a3, a0 ^ _X2[a1] ^ _X3[a2] ^ a3, a0 ^ a1 ^ _X2[a2] ^ _X3[a3],
                          _X3[a0] ^ a1 ^ a2 ^ _X2[a3]], axis=2)
            s = m.reshape(-1, 16)
        s = s ^ rk[r]
    return s


def counter_blocks(ctr: int, nb: int):
    """The (nb, 16) big-endian blocks ctr, ctr + 1, .. mod 2^128."""
    ctr &= MASK128
    hi, lo = ctr >> 64, ctr & (2**64 - 1)
    j = np.arange(nb, dtype=np.uint64)
    lo_j = np.uint64(lo) + j   # wraps mod 2^64
    carry = (lo_j < np.uint64(lo)).astype(np.uint64)
    hi_j = np.uint64(hi) + carry
    out = np.empty((nb, 16), dtype=np.uint8)
    out[:, :8] = hi_j.astype(">u8").view(np.uint8).reshape(nb, 8)
    out[:, 8:] = lo_j.astype(">u8").view(np.uint8).reshape(nb, 8)
    return out


def ctr_words(key: bytes, ctr, n: int):
    """n u64 words of the keystream AES_key(ctr + j), j = 0..; ctr an int or 16 big-endian bytes."""
    if isinstance(ctr, (bytes, bytearray)):
        ctr = int.from_bytes(ctr, "big")
    nb = (n + 1) // 2
    if nb == 0:
        return np.zeros(0, dtype=np.uint64)
    ks = encrypt_blocks(expand_key(key), counter_blocks(ctr, nb))
    return ks.reshape(-1).view("<u8")[:n].astype(np.uint64)


class CtrDrbg:
    """CTR_DRBG (AES-256, no df). seed(), reseed(), generate(n words); counts() as the library's."""

    def __init__(self, seed: bytes):
        self.seed(seed)

    def _update(self, data: bytes):
        assert len(data) == 48
        temp = encrypt_blocks(expand_key(self.K), counter_blocks(self.V + 1, 3)).reshape(-1)
        temp = bytes(temp ^ np.frombuffer(data, dtype=np.uint8))
        self.K, self.V = temp[:32], int.from_bytes(temp[32:], "big")

    def seed(self, entropy: bytes):
        self.K, self.V = bytes(32), 0
        self._update(entropy)
        self.calls = self.blocks = self.reseeds = 0

    def reseed(self, entropy: bytes):
        self._update(entropy)
        self.reseeds += 1

    def generate(self, n: int):
        if n == 0:
            return np.zeros(0, dtype=np.uint64)
        nb = (n + 1) // 2
        out = ctr_words(self.K, self.V + 1, n)
        self.V = (self.V + nb) & MASK128
        self._update(bytes(48))
        self.calls += 1
        self.blocks += nb
        return out

    def generate_bytes(self, k: int):
        """generate_host: the first k bytes of a generate call of ceil(k / 8) words."""
        return self.generate((k + 7) // 8).astype("<u8").tobytes()[:k]

    def counts(self):
        return (self.calls, self.blocks, self.reseeds, 0)
