"""The device .ct codec (pvac_hip_ct_image_plan / _write / _parse) on the GPU. In every case the expected
bytes come from the host pvac_ct_write and the expected arrays from the host pvac_ct_parse, never from the
code under test: the golden files, an alignment sweep whose cipher starts and edge regions reach every
byte alignment, a capacity-padded ct_mul output with a guarded tail, ciphers larger than a tile,
degenerate batches, the round trip against batch_pack, and the errors whose offsets stay in bounds."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "**", "*.ct"), recursive=True))
EINVAL, ENOMEM, ERANGE = -22, -12, -34
CANARY = 0x25A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, canon_tag=0x5EED)


@pytest.fixture(scope="module")
def codec():
    from pvac_hfhe_cppbyv_amd import codec
    return codec


# ---------------------------------------------------------------------------------------- helpers
def upload(eng, soa, shift=0):
    """An SoA dict (host arrays; sigma (E, sigma_words) or None) as a DeviceBatch; shift: words by which
    the sigma base is moved off its allocation (1 = an 8-byte-offset base)."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    one = lambda a: a if len(a) else np.zeros(1, a.dtype)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(one(a)).view(np.int64)).to(eng.device)
    lay = torch.from_numpy(np.ascontiguousarray(one(soa["layers"])).view(np.int64).reshape(-1, 5)).to(eng.device)
    sg = None
    if soa["sigma"] is not None:
        s = np.ascontiguousarray(soa["sigma"])
        flat = torch.zeros(s.size + shift + 1, dtype=torch.int64, device=eng.device)
        flat[shift:shift + s.size] = torch.from_numpy(s.view(np.int64).reshape(-1)).to(eng.device)
        sg = flat[shift:shift + s.size].view(s.shape[0], s.shape[1])
        assert sg.data_ptr() % 16 == (8 * shift) % 16
    return DeviceBatch(soa["n"], t(soa["l_off"]), t(soa["l_cnt"]), lay, t(soa["e_off"]), t(soa["e_cnt"]), t(soa["meta"]),
                       t(soa["w_lo"]), t(soa["w_hi"]), sg)


def dev_image(eng, X, bits, slack=0):
    """plan + write into a buffer of pos[n] + slack bytes pre-filled with 0xA5: (whole buffer as numpy, pos[n])."""
    import torch
    pos = torch.empty(X.n + 1, dtype=torch.int64, device=eng.device)
    size = C.c_uint64()
    sx = X.struct()
    rc = eng.lib.pvac_hip_ct_image_plan(eng.ctx, C.byref(sx), bits, C.c_void_p(pos.data_ptr()), C.byref(size))
    assert rc == 0, eng.lib.pvac_hip_last_error(eng.ctx)
    nbytes = int(size.value)
    buf = torch.full(((nbytes + slack + 15) & ~15,), 0xA5, dtype=torch.uint8, device=eng.device)
    rc = eng.lib.pvac_hip_ct_image_write(eng.ctx, C.byref(sx), bits, C.c_void_p(pos.data_ptr()), C.c_void_p(buf.data_ptr()),
                                         nbytes + slack)
    assert rc == 0, eng.lib.pvac_hip_last_error(eng.ctx)
    eng.sync()
    assert int(pos[-1].item()) == nbytes and int(pos[0].item()) == 16
    return buf.cpu().numpy(), nbytes


def canvas(eng, n, lcap, ecap, sw=0, shift=0):
    """A DeviceBatch to parse into, every word a canary."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    f = lambda *shape: torch.full(shape, CANARY, dtype=torch.int64, device=eng.device)
    sg = None
    if sw:
        rows = max(ecap, 1)
        sg = f(rows * sw + shift + 1)[shift:shift + rows * sw].view(rows, sw)
    m = max(n, 1)
    return DeviceBatch(n, f(m), f(m), f(max(lcap, 1), 5), f(m), f(m), f(max(ecap, 1)), f(max(ecap, 1)), f(max(ecap, 1)), sg)


def dev_parse(eng, data, pos, n, bits, lcap, ecap, sw=0, shift=0):
    """Upload the file bytes and pos, parse into a canvas: (code, batch, status)."""
    import torch
    data = np.frombuffer(data, np.uint8)
    padded = np.full((data.size + 15) & ~15, 0x5A, np.uint8)
    padded[:data.size] = data
    image = torch.from_numpy(padded).to(eng.device)[:data.size]
    dpos = torch.from_numpy(np.ascontiguousarray(pos).view(np.int64)).to(eng.device)
    X = canvas(eng, n, lcap, ecap, sw, shift)
    return eng.ct_from_image(image, dpos, n, bits, lcap, ecap, status=True, out=X)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def assert_equals_soa(X, soa, nw):
    """Every array of the parsed batch X against the host parser's SoA, the slots past the totals untouched."""
    from pvac_hfhe_cppbyv_amd import LAYER_DT
    n, nl, ne = soa["n"], soa["total_layers"], soa["total_edges"]
    for f in ("l_off", "l_cnt", "e_off", "e_cnt"):
        assert np.array_equal(u64(getattr(X, f))[:n], soa[f][:n]), f
    lay = X.layers.cpu().numpy().reshape(-1).view(LAYER_DT)
    assert lay[:nl].tobytes() == np.ascontiguousarray(soa["layers"][:nl]).tobytes()   # all 40 bytes, pad included
    assert (X.layers.cpu().numpy()[nl:] == CANARY).all()
    for f in ("meta", "w_lo", "w_hi"):
        got = u64(getattr(X, f))
        assert np.array_equal(got[:ne], soa[f][:ne]), f
        assert (got[ne:] == CANARY).all(), f
    if X.sigma is not None:
        got = u64(X.sigma)
        if nw:
            assert np.array_equal(got[:ne, :nw], soa["sigma"][:ne, :nw])
        assert (got[:ne, nw:] == 0).all()
        assert (got[ne:] == CANARY).all()


def host_parse(codec, data):
    return codec.read_ct_soa(data, threads=1)


def check_both_ways(eng, codec, soa, bits, shift=0):
    """soa imaged on the device == the host writer's bytes; those bytes parsed on the device == the host parser's arrays."""
    expect = codec.write_ct(soa, bits, threads=1)
    X = upload(eng, soa, shift)
    got, nbytes = dev_image(eng, X, bits)
    assert nbytes == len(expect)
    assert got[:nbytes].tobytes() == expect
    assert (got[nbytes:] == 0xA5).all()
    want = host_parse(codec, expect)
    info, pos = codec.index(expect)
    sw = soa["sigma"].shape[1] if soa["sigma"] is not None else 0
    rc, P, st = dev_parse(eng, expect, pos, soa["n"], info.sigma_bits, want["total_layers"], want["total_edges"], sw, shift)
    assert rc == 0 and not st.any()
    assert_equals_soa(P, want, info.sigma_words if sw else 0)


def make_soa(rng, l_cnt, e_cnt, rules, sw=None, with_sigma=True):
    """A random dense SoA batch: per-cipher layer and edge counts, rules(l) the rule of a cipher's layer l."""
    from pvac_hfhe_cppbyv_amd import LAYER_DT
    lc, ec = np.array(l_cnt, np.uint64), np.array(e_cnt, np.uint64)
    n, nl, ne = len(lc), int(lc.sum()), int(ec.sum())
    ex = lambda c: (np.concatenate([[0], np.cumsum(c)[:-1]]) if n else c).astype(np.uint64)
    layers = np.zeros(nl, LAYER_DT)
    for f in ("pa", "pb"):
        layers[f] = rng.integers(0, 2**32, nl, dtype=np.uint64)
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        layers[f] = rng.integers(0, 2**64, nl, dtype=np.uint64)
    layers["rule"] = [rules(l) for c in lc for l in range(int(c))]
    r64 = lambda k: rng.integers(0, 2**64, k, dtype=np.uint64)
    return {"n": n, "l_off": ex(lc), "l_cnt": lc, "e_off": ex(ec), "e_cnt": ec, "layers": layers,
            "meta": r64(ne),   # the top byte is set: the writer must drop it
            "w_lo": r64(ne), "w_hi": r64(ne),
            "sigma": r64(ne * sw).reshape(ne, sw) if with_sigma and sw else None}


# ---------------------------------------------------------------------------------------- 1. fixtures
def test_there_are_fixtures():
    assert len(FILES) >= 40


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.relpath(p, GOLD))
def test_fixture_images_and_parses(eng, codec, path):
    with open(path, "rb") as f:
        data = f.read()
    soa = host_parse(codec, data)
    X = upload(eng, soa)
    got, nbytes = dev_image(eng, X, soa["sigma_bits"])
    assert got[:nbytes].tobytes() == data
    assert (got[nbytes:] == 0xA5).all()
    info, pos = codec.index(data)
    sw = info.sigma_words
    rc, P, st = dev_parse(eng, data, pos, soa["n"], info.sigma_bits, soa["total_layers"], soa["total_edges"], sw)
    assert rc == 0 and not st.any()
    assert_equals_soa(P, soa, sw)


# ---------------------------------------------------------------------------------------- 2. alignment sweep
SWEEP = [(0, 0, 0), (64, 1, 0), (100, 2, 0), (8191, 128, 0), (8192, 128, 0), (8192, 130, 0), (8192, 128, 1)]


def sweep_soa(bits, sw):
    rng = np.random.default_rng(1000 + bits + sw)
    edges = [0, 1, 2, 3, 5, 17]
    return make_soa(rng, [k % 16 for k in range(48)], [edges[k % 6] for k in range(48)], lambda l: (0, 1, 2)[l % 3], sw, sw > 0)


@pytest.mark.parametrize("bits,sw,shift", SWEEP)
def test_alignment_sweep(eng, codec, bits, sw, shift):
    soa = sweep_soa(bits, sw)
    # on the CPU first: cipher starts and edge-region starts each cover all 16 residues mod 16
    nw = (bits + 63) // 64 if sw else 0
    eb = 28 + 8 * nw
    pos = [16]
    for k in range(48):
        pos.append(pos[-1] + 8 + sum(9 if (l % 3) == 1 else 25 for l in range(k % 16)) + int(soa["e_cnt"][k]) * eb)
    assert {p % 16 for p in pos[:-1]} == set(range(16))
    assert {(pos[k + 1] - int(soa["e_cnt"][k]) * eb) % 16 for k in range(48)} == set(range(16))
    before = eng.ct_image_path_counts()
    check_both_ways(eng, codec, soa, bits, shift)
    after = eng.ct_image_path_counts()
    wide = nw > 0 and nw % 2 == 0 and sw % 2 == 0 and shift == 0
    assert after["write_wide"] - before["write_wide"] == int(wide)
    assert after["write_narrow"] - before["write_narrow"] == int(not wide)
    assert after["parse_wide"] - before["parse_wide"] == int(wide)
    assert after["parse_narrow"] - before["parse_narrow"] == int(not wide)


def test_sweep_settings_take_both_sigma_paths():
    kinds = {(b + 63) // 64 % 2 == 0 and s % 2 == 0 and sh == 0 and s > 0 for b, s, sh in SWEEP}
    assert kinds == {True, False}


# ---------------------------------------------------------------------------------------- 3. padded CSR and the tail
@pytest.fixture(scope="module")
def padded(eng):
    """A ct_mul_exec output on gen_fresh for 64 pairs: capacity-padded CSR, weights only."""
    A = eng.gen_fresh(64, 11, 20)
    B = eng.gen_fresh(64, 12, 20)
    Cb = eng.ct_mul(A, B, nonce_seed=13)
    eng.sync()
    eo, ec = u64(Cb.e_off), u64(Cb.e_cnt)
    assert (eo[1:] > eo[:-1] + ec[:-1]).any()   # padded: some cipher ends before the next one's slots
    return Cb


def host_bytes(codec, X, bits=8192):
    return codec.write_ct(X.to_host(), bits, threads=1)


def test_padded_batch_is_imaged_directly_and_the_tail_is_kept(eng, codec, padded):
    got, nbytes = dev_image(eng, padded, 8192, slack=64)
    assert got.size >= nbytes + 64
    assert got[:nbytes].tobytes() == host_bytes(codec, padded)
    assert (got[nbytes:] == 0xA5).all()


def test_padded_batch_ending_at_every_residue(eng, codec, padded):
    """pos[n] forced to each residue class mod 16. An edge record is 28 bytes here, so dropping edges of
    the last cipher reaches four classes; dropping its trailing 9-byte PROD layers as well reaches all."""
    last = padded.n - 1
    L0, E0 = int(padded.l_cnt[last].item()), int(padded.e_cnt[last].item())
    lay = padded.layers.cpu().numpy()[int(padded.l_off[last].item()):][:L0, 0] & 0xFFFFFFFF
    assert L0 >= 4 and (lay[-3:] == 1).all() and E0 > 16
    seen = set()
    try:
        for dl in range(4):
            for de in range(4):
                padded.l_cnt[last] = L0 - dl
                padded.e_cnt[last] = E0 - de
                got, nbytes = dev_image(eng, padded, 8192, slack=64)
                assert got[:nbytes].tobytes() == host_bytes(codec, padded), (dl, de)
                assert (got[nbytes:] == 0xA5).all(), (dl, de)
                seen.add(nbytes % 16)
    finally:
        padded.l_cnt[last] = L0
        padded.e_cnt[last] = E0
    assert seen == set(range(16))


# ---------------------------------------------------------------------------------------- 4. tiles
@pytest.mark.parametrize("edges,sw", [(2053, 128), (70001, 0)])
def test_a_cipher_larger_than_a_tile(eng, codec, edges, sw):
    rng = np.random.default_rng(edges)
    soa = make_soa(rng, [3, 5, 2], [1, edges, 1], lambda l: l % 2, sw, sw > 0)
    check_both_ways(eng, codec, soa, 8192)


# ---------------------------------------------------------------------------------------- 5. degenerate batches
@pytest.mark.parametrize("l_cnt,e_cnt", [([], []), ([0] * 5, [0] * 5), ([2, 0, 0, 3, 0], [40, 0, 0, 7, 0]),
                                         ([0, 4, 0], [0, 0, 0])])
@pytest.mark.parametrize("sw", [0, 128])
def test_degenerate_batches(eng, codec, l_cnt, e_cnt, sw):
    rng = np.random.default_rng(7)
    soa = make_soa(rng, l_cnt, e_cnt, lambda l: l % 2, sw, sw > 0)
    check_both_ways(eng, codec, soa, 8192)


def test_the_empty_image_is_the_header(eng, codec):
    soa = make_soa(np.random.default_rng(1), [], [], lambda l: 0, 0, False)
    got, nbytes = dev_image(eng, upload(eng, soa), 8192)
    assert nbytes == 16 and got[:16].tobytes() == codec.write_ct(soa, 8192)


# ---------------------------------------------------------------------------------------- 6. round trip
@pytest.mark.parametrize("with_sigma", [False, True])
def test_round_trip_equals_batch_pack(eng, codec, padded, with_sigma):
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    X = DeviceBatch(padded.n, padded.l_off, padded.l_cnt, padded.layers, padded.e_off, padded.e_cnt, padded.meta,
                    padded.w_lo, padded.w_hi)
    if with_sigma:
        X.sigma = torch.empty((padded.meta.shape[0], 128), dtype=torch.int64, device=eng.device)
        eng.fill_random(X.sigma, 99)
    Pk = eng.pack(X)
    nl, ne = Pk.layers.shape[0], Pk.meta.shape[0]
    image, pos = eng.ct_image(X, 8192, return_pos=True)
    Y = eng.ct_from_image(image, pos, X.n, 8192 if with_sigma else 0, nl, ne, sigma=with_sigma)
    eng.sync()
    for f in ("l_off", "l_cnt", "e_off", "e_cnt"):
        assert torch.equal(getattr(Y, f)[:X.n], getattr(Pk, f)[:X.n]), f
    # PROD layers carry no seed in a file: compare what the format keeps
    ly, lp = Y.layers[:nl].clone(), Pk.layers[:nl].clone()
    prod = (lp[:, 0] & 0xFFFFFFFF) == 1
    lp[prod, 2:] = 0
    lp[:, 1] &= 0xFFFFFFFF          # pad is written as 0
    lp[~prod, 0] &= 0xFFFFFFFF      # BASE keeps no pa
    lp[~prod, 1] = 0                # ... and no pb
    assert torch.equal(ly, lp)
    assert torch.equal(Y.meta[:ne], Pk.meta[:ne]) and torch.equal(Y.w_lo[:ne], Pk.w_lo[:ne]) and torch.equal(Y.w_hi[:ne], Pk.w_hi[:ne])
    if with_sigma:
        assert torch.equal(Y.sigma[:ne], Pk.sigma[:ne])


# ---------------------------------------------------------------------------------------- 7. errors, offsets in bounds
@pytest.fixture(scope="module")
def small(codec):
    rng = np.random.default_rng(5)
    soa = make_soa(rng, [2, 3, 1, 4], [6, 1, 9, 3], lambda l: l % 2, 128, True)
    data = codec.write_ct(soa, 8192, threads=1)
    info, pos = codec.index(data)
    return soa, data, pos


def test_an_altered_nbits_field_is_refused_with_status_2(eng, codec, small):
    soa, data, pos = small
    bad = bytearray(data)
    eb = 28 + 8 * 128
    at = int(pos[3]) - 4 * eb + 24   # cipher 2's edge 5: the nbits field
    assert int.from_bytes(bad[at:at + 4], "little") == 8192
    bad[at:at + 4] = (8191).to_bytes(4, "little")
    rc, _, st = dev_parse(eng, bytes(bad), pos, 4, 8192, 10, 19, 128)
    assert rc == EINVAL and st.tolist() == [0, 0, 2, 0]
    rc, P, st = dev_parse(eng, data, pos, 4, 8192, 10, 19, 128)
    assert rc == 0 and not st.any()
    assert_equals_soa(P, host_parse(codec, data), 128)


@pytest.mark.parametrize("lcap,ecap", [(9, 19), (10, 18)])
def test_a_cap_one_too_small_is_enomem_and_nothing_is_written(eng, small, lcap, ecap):
    soa, data, pos = small
    rc, X, st = dev_parse(eng, data, pos, 4, 8192, lcap, ecap, 128)
    assert rc == ENOMEM and not st.any()
    for t in (X.l_off, X.l_cnt, X.e_off, X.e_cnt, X.layers, X.meta, X.w_lo, X.w_hi, X.sigma):
        assert (t == CANARY).all()


def test_host_side_refusals(eng, codec, small):
    import torch
    soa, data, pos = small
    X = upload(eng, soa)
    sx = X.struct()
    dpos = torch.empty(5, dtype=torch.int64, device=eng.device)
    size = C.c_uint64()
    lib = eng.lib
    # nw > sigma_words
    assert lib.pvac_hip_ct_image_plan(eng.ctx, C.byref(sx), 8193, C.c_void_p(dpos.data_ptr()), C.byref(size)) == EINVAL
    assert lib.pvac_hip_ct_image_plan(eng.ctx, C.byref(sx), 8192, C.c_void_p(dpos.data_ptr()), C.byref(size)) == 0
    assert size.value == len(data)
    buf = torch.full((len(data) + 32,), 0xA5, dtype=torch.uint8, device=eng.device)
    # a misaligned image pointer, then a cap one byte short
    assert lib.pvac_hip_ct_image_write(eng.ctx, C.byref(sx), 8192, C.c_void_p(dpos.data_ptr()), C.c_void_p(buf.data_ptr() + 8),
                                       len(data)) == EINVAL
    assert lib.pvac_hip_ct_image_write(eng.ctx, C.byref(sx), 8192, C.c_void_p(dpos.data_ptr()), C.c_void_p(buf.data_ptr()),
                                       len(data) - 1) == ERANGE
    eng.sync()
    assert (buf == 0xA5).all()
    assert lib.pvac_hip_ct_image_write(eng.ctx, C.byref(sx), 8192, C.c_void_p(dpos.data_ptr()), C.c_void_p(buf.data_ptr()),
                                       len(data)) == 0
    eng.sync()
    assert buf.cpu().numpy()[:len(data)].tobytes() == data
    # the parser: a misaligned image, and sigma rows narrower than the file's
    img = torch.zeros(len(data) + 32, dtype=torch.uint8, device=eng.device)
    P = canvas(eng, 4, 10, 19, 128)
    dp = torch.from_numpy(pos.view(np.int64)).to(eng.device)
    rc, _, _ = eng.ct_from_image(img[8:8 + len(data)], dp, 4, 8192, 10, 19, status=True, out=P)
    assert rc == EINVAL
    P = canvas(eng, 4, 10, 19, 127)
    rc, _, _ = eng.ct_from_image(img[:len(data)], dp, 4, 8192, 10, 19, status=True, out=P)
    assert rc == EINVAL
    assert (P.meta == CANARY).all()


def test_a_rule_of_256_or_more_is_refused_by_the_plan(eng, small):
    import torch
    soa, data, pos = small
    bad = dict(soa)
    bad["layers"] = soa["layers"].copy()
    bad["layers"]["rule"][4] = 257
    X = upload(eng, bad)
    sx = X.struct()
    dpos = torch.empty(5, dtype=torch.int64, device=eng.device)
    size = C.c_uint64()
    assert eng.lib.pvac_hip_ct_image_plan(eng.ctx, C.byref(sx), 8192, C.c_void_p(dpos.data_ptr()), C.byref(size)) == EINVAL


# ---------------------------------------------------------------------------------------- the file-level wrappers
def test_save_and_load_on_the_device_agree_with_the_host_codec(eng, codec, tmp_path):
    import torch
    path = os.path.join(GOLD, "bounty", "seed3.ct")
    with open(path, "rb") as f:
        data = f.read()
    X = codec.load_ct_device(eng, path)
    H = codec.load_ct(path, eng.device)
    for f in ("l_off", "l_cnt", "e_off", "e_cnt", "layers", "meta", "w_lo", "w_hi", "sigma"):
        assert torch.equal(getattr(X, f), getattr(H, f)), f
    out = str(tmp_path / "out.ct")
    assert codec.save_ct_device(eng, X, out) == len(data)
    with open(out, "rb") as f:
        assert f.read() == data
