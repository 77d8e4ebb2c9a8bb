"""The model of pvac_hip_batch_gather over lists of HostCipher: plain list indexing, with the ABI's
null-pick rules. What the GPU tests compare Engine.gather / cat / select / split against."""
import numpy as np

EINVAL = -22
MAX_SOURCES = 1024


class GatherError(ValueError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def gather(sources, pick_src=None, pick_idx=None):
    """sources: a list of lists of ciphers. Output k = sources[pick_src[k]][pick_idx[k]] (the same object:
    a gather copies verbatim). pick_src None: every pick from the one source; pick_idx None (then
    pick_src is None too): the concatenation."""
    n_src = len(sources)
    if n_src > MAX_SOURCES:
        raise GatherError(EINVAL, "too many sources")
    if pick_idx is None:
        if pick_src is not None:
            raise GatherError(EINVAL, "pick_src without pick_idx")
        return [c for s in sources for c in s]
    if pick_src is None:
        if n_src != 1:
            raise GatherError(EINVAL, "pick_idx without pick_src takes exactly one source")
        pick_src = [0] * len(pick_idx)
    if len(pick_src) != len(pick_idx):
        raise GatherError(EINVAL, "pick lists differ in length")
    if len(pick_idx) and n_src == 0:
        raise GatherError(EINVAL, "output ciphers without a source")
    out = []
    for j, i in zip(pick_src, pick_idx):
        j, i = int(j), int(i)
        if not 0 <= j < n_src or not 0 <= i < len(sources[j]):
            raise GatherError(EINVAL, "pick out of range")
        out.append(sources[j][i])
    return out


def split(ciphers, sizes):
    assert sum(sizes) == len(ciphers)
    out, at = [], 0
    for s in sizes:
        out.append(ciphers[at:at + s])
        at += s
    return out


def same(a, b, sigma=False):
    """Every field of two host ciphers: the full 40-byte layer records, edge headers, weights, sigma rows."""
    ok = (len(a.layers) == len(b.layers) and len(a.meta) == len(b.meta) and
          np.ascontiguousarray(a.layers).tobytes() == np.ascontiguousarray(b.layers).tobytes() and
          np.array_equal(a.meta, b.meta) and np.array_equal(a.w_lo, b.w_lo) and np.array_equal(a.w_hi, b.w_hi))
    if ok and sigma and len(a.meta):   # a cipher without edges has no rows to compare
        ok = np.array_equal(np.asarray(a.sigma).reshape(len(a.meta), -1), np.asarray(b.sigma).reshape(len(b.meta), -1))
    return ok
